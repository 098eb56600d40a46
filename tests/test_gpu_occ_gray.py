"""Gray / resized / unnormalised output of the device input pipeline on the GPU (msml_occ_draw_out, msml_occ_apply_out)
against the CPU restatement of tests/occ_gray_cases.py, which tests/test_occ_gray_cpu.py pins to Pillow.

Bounds.  Descriptors and masks are integers: exact.  Without the normalisation img (light off) and ori are u8 / 255 in
f32, one correctly rounded division on both sides: exact; with it, 1e-7 as tests/test_occ.py allows its unlit images.
With the light on, exp() differs between the device and numpy by float rounding and the map is a float16: 2e-3 on
[-1, 1] as tests/test_occ.py, and 1e-3 on [0, 1] because the normalisation doubles the scale."""
import numpy as np
import pytest
import torch

from tests import occ_gray_cases as G

pytestmark = pytest.mark.gpu

GEOMETRIC = ["train", "rect", "block", "none", "polygon"]
TEXTURE = ["ms1m", "casia", "glasses", "scarf", "object"]
_ATLAS = {}


def atlas_and_sets(seed=3):
    from msml_amd import data
    if seed not in _ATLAS:
        sets = G.synthetic_sets(seed)
        _ATLAS[seed] = (data.OccluderAtlas(sets, 112, "cuda"), G.oracle_sets(sets))
    return _ATLAS[seed]


def faces(n, seed=11):
    src = np.random.RandomState(seed).randint(0, 256, (n, 112, 112, 3)).astype(np.uint8)
    return src, torch.from_numpy(src).cuda()


def check(got, ref, light, use_norm, want_ori=True):
    img, msk, ori = (None if t is None else t.cpu().numpy() for t in got)
    rimg, rmsk, rori = ref
    assert img.shape == rimg.shape and msk.shape == rmsk.shape and msk.dtype == np.int64
    assert np.array_equal(msk, rmsk)                                              # masks: exact
    if want_ori:
        err = np.abs(ori - rori).max()
        print("ori err", err)
        assert (err < 1e-7) if use_norm else np.array_equal(ori, rori), err
    else:
        assert ori is None
    err = np.abs(img - rimg).max()
    print("img err", err, "light", light, "norm", use_norm)
    if light:
        assert err < (2e-3 if use_norm else 1e-3), err
    else:
        assert (err < 1e-7) if use_norm else np.array_equal(img, rimg), err
    lo = -1.0 if use_norm else 0.0
    assert img.min() >= lo - 1e-6 and img.max() <= 1 + 1e-6
    assert ori is None or (ori.min() >= lo - 1e-6 and ori.max() <= 1 + 1e-6)


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("gray,out_size,use_norm", G.SWITCHES)
@pytest.mark.parametrize("mode", GEOMETRIC + TEXTURE)
def test_gray_resized_pipeline_matches_restatement(mode, gray, out_size, use_norm, light):
    from msml_amd import data
    n = 64
    lo, hi = (40, 41) if mode == "block" else (0, 36)
    src, dsrc = faces(n)
    atlas, osets = atlas_and_sets() if mode in TEXTURE else (None, ())
    img, msk, ori, desc = data.augment(dsrc, 1234, 5000, mode, lo, hi, True, light, True, atlas, gray=gray,
                                       out_size=out_size, use_norm=use_norm)
    ref_desc = G.draw(1234, 5000, n, 112, 112, data.MODES[mode], lo, hi, True, sets=osets, out_size=out_size)
    assert np.array_equal(desc.cpu().numpy(), ref_desc)                           # integer draws: exact
    check((img, msk, ori), G.apply(src, ref_desc, light, True, osets, gray, out_size, use_norm), light, use_norm)
    if mode not in ("none", "casia", "train", "ms1m"):
        assert (msk == 0).any()


@pytest.mark.parametrize("mode", ["rect", "glasses"])
def test_vertical_pass_alone(mode):
    """out_size = (96, 112): the width stays, so the kernel runs its vertical pass and no horizontal one (SWITCHES has
    the other half, (112, 96)); gray, with ori, a geometric and a texture occluder."""
    from msml_amd import data
    n, out_size = 8, (96, 112)
    src, dsrc = faces(n)
    atlas, osets = atlas_and_sets() if mode in TEXTURE else (None, ())
    img, msk, ori, desc = data.augment(dsrc, 1234, 5000, mode, 0, 36, True, True, True, atlas, gray=True, out_size=out_size,
                                       use_norm=False)
    ref_desc = G.draw(1234, 5000, n, 112, 112, data.MODES[mode], 0, 36, True, sets=osets, out_size=out_size)
    assert np.array_equal(desc.cpu().numpy(), ref_desc)
    assert img.shape == (n, 1, 96, 112)
    check((img, msk, ori), G.apply(src, ref_desc, True, True, osets, True, out_size, False), True, False)
    assert (msk == 0).any()


def test_mask_is_interpolated_on_the_device():
    """The 40 x 70 rectangle of the CPU test: 3 807 occluded pixels at 128, as Pillow's interpolated mask -- a kernel that
    rescaled the rectangle instead (3 657) fails here."""
    from msml_amd import data
    from oracle import occ as oo
    d = np.zeros((2, oo.DESC_WORDS), np.int32)
    d[:, :8] = [oo.OCC_RECT, 30, 20, 40, 70, 9, 99, 199]
    d[1, 8] = 1
    src, dsrc = faces(2, 2)
    for gray in (True, False):
        _, msk, _ = data.apply(dsrc, torch.from_numpy(d).cuda(), False, False, None, gray=gray, out_size=128, use_norm=False)
        assert (msk == 0).sum(dim=(1, 2)).tolist() == [3807, 3807]
        assert torch.equal(msk[1], msk[0].flip(1))
        assert np.array_equal(msk.cpu().numpy(), G.apply(src, d, False, False, (), gray, 128, False)[1])


def test_without_ori():
    """want_ori=False: no clean planes are resampled, ori is None, img and msk are what they are with it."""
    from msml_amd import data
    src, dsrc = faces(16, 4)
    atlas, osets = atlas_and_sets()
    img, msk, ori, desc = data.augment(dsrc, 9, 64, "ms1m", 0, 36, True, True, False, atlas, gray=True, out_size=128,
                                       use_norm=False)
    ref = G.apply(src, desc.cpu().numpy(), True, False, osets, True, 128, False)
    check((img, msk, ori), ref, True, False, want_ori=False)


def test_defaults_are_untouched():
    """With the three switches at their defaults augment goes through msml_occ_draw[_tex] / msml_occ_apply[_tex] as
    before; and the new kernel asked for the source size, RGB, normalised computes what the old one does."""
    from msml_amd import data
    src, dsrc = faces(64)
    atlas, _ = atlas_and_sets()
    for mode, at in (("train", None), ("ms1m", atlas)):
        for light in (False, True):
            a = data.augment(dsrc, 1234, 5000, mode, 0, 36, True, light, True, at)
            b = data.augment(dsrc, 1234, 5000, mode, 0, 36, True, light, True, at, gray=False, out_size=None, use_norm=True)
            c = data.augment(dsrc, 1234, 5000, mode, 0, 36, True, light, True, at, out_size=112)
            for x, y in zip(a, b):
                assert torch.equal(x, y)
            # the same operations in the same order: integers and unlit values exact, lit ones to tests/test_occ.py's bound
            assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]) and torch.equal(a[3], c[3])
            err = (a[0] - c[0]).abs().max().item()
            print("old vs new kernel, light", light, "err", err)
            assert err < 2e-3 if light else err == 0, err
    assert a[0].shape == (64, 3, 112, 112) and a[1].shape == (64, 112, 112)


def test_beyond_the_lds_limit_raises_before_launching():
    """RGB 112 -> 224: header 512 + tables 2 x 8 960 + raw 37 632 + mask and work plane 2 x 12 544 + horizontal
    intermediate 112 x 224 + the staged image 3 x 224 x 224 = 256 768 bytes > 160 KB; gray 224 (156 416) fits."""
    from msml_amd import data
    src, dsrc = faces(4)
    need = 512 + 2 * 224 * 40 + 112 * 112 * 3 + 2 * 112 * 112 + 112 * 224 + 3 * 224 * 224
    assert need == 256768 and need > 160 * 1024 >= need - 2 * 224 * 224
    for want_ori in (True, False):
        with pytest.raises(RuntimeError, match=r"needs 256768 bytes of LDS"):
            data.augment(dsrc, 1, 0, "train", want_ori=want_ori, out_size=224)
    torch.cuda.synchronize()
    img, msk, ori, desc = data.augment(dsrc, 1, 0, "train", light=False, gray=True, out_size=224, use_norm=False)
    check((img, msk, ori), G.apply(src, desc.cpu().numpy(), False, True, (), True, 224, False), False, False)
    with pytest.raises(RuntimeError, match=r"not a multiple of 4"):
        data.augment(dsrc, 1, 0, "train", gray=True, out_size=(128, 126))


def lightcnn_loader(batch, steps, mode="casia", seed=77, pool=3):
    from msml_amd import data
    atlas, osets = atlas_and_sets(9)
    src = data.SynthFaceSource(batch, 1000, steps=steps, pool=pool, seed=9)
    return src, osets, data.DeviceLoaderX(src, 0, seed=seed, mode=mode, atlas=atlas, gray=True, out_size=128, use_norm=False)


def test_device_loader_lightcnn_recipe():
    """DeviceLoaderX in the LightCNN recipe (casia mix with an atlas, gray, 128, no Normalize): five batches in order,
    each reproducible from (seed, k * batch), labels with their images."""
    from msml_amd import data
    B = 32
    src, osets, loader = lightcnn_loader(B, 5)
    seen = []
    for img, msk, ori, lab in loader:
        seen.append((img.clone(), msk.clone(), ori.clone(), lab.clone()))
        torch.cuda.synchronize()
    assert len(seen) == 5
    kinds = set()
    for k, (img, msk, ori, lab) in enumerate(seen):
        assert img.shape == (B, 1, 128, 128) and msk.shape == (B, 128, 128) and ori.shape == (B, 1, 128, 128)
        faces_k, labels = src.pool[k % 3]
        assert torch.equal(lab.cpu(), labels)
        ref_desc = G.draw(77, k * B, B, 112, 112, data.MODES["casia"], sets=osets, out_size=128)
        kinds |= set(ref_desc[:, 0].tolist())
        check((img, msk, ori), G.apply(faces_k.numpy(), ref_desc, True, True, osets, True, 128, False), True, False)
    assert kinds & {5, 6, 7} and 0 in kinds


def test_lightcnn_trains_from_the_device_loader():
    """Plumbing: three bf16 training steps of the LightCNN MSML (the construction of tools/bench_lightcnn.py) fed by the
    loader; finite losses, a positive segmentation loss, and an all-ones mask from batches without an occluder."""
    from msml_amd import ops
    from msml_amd.backbones import MSML
    from msml_amd.optim import FlatSGD, reference_param_groups
    from msml_amd.tricks.consensus_loss import StructureConsensuLossFunction
    B, classes = 16, 1000
    torch.manual_seed(1234)
    model = MSML("lightcnn", "unet", (1, 1, 1, 1), classes, fp16=True, fm_params=(3, 2, "sigmoid", "mul"),
                 header_type="Softmax",
                 peer_params={"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}).cuda().train()
    opt = FlatSGD(reference_param_groups(model, B, 1), 0.9, 5e-4, 5.0)
    seg_crit = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")
    saved = ops.WGRAD_STREAM, ops.OSB_STREAM
    ops.WGRAD_STREAM, ops.OSB_STREAM = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        steps = 0
        for img, msk, ori, lab in lightcnn_loader(B, 3)[2]:
            opt.zero_grad()
            final_cls, final_seg, _ = model(img, lab)
            cls_loss = torch.nn.functional.cross_entropy(final_cls, lab)
            seg_loss = seg_crit(final_seg, msk, msk)
            (cls_loss + seg_loss).backward()
            opt.step()
            torch.cuda.synchronize()
            assert torch.isfinite(cls_loss).item() and torch.isfinite(seg_loss).item()
            assert seg_loss.item() > 0
            assert (msk == 0).any() and (msk == 1).any()
            steps += 1
        assert steps == 3
        for img, msk, ori, lab in lightcnn_loader(B, 2, mode="none")[2]:
            assert (msk == 1).all()
            assert torch.isfinite(img).all() and img.shape == ori.shape
    finally:
        ops.WGRAD_STREAM, ops.OSB_STREAM = saved
        torch.cuda.synchronize()
