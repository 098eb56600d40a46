"""The facial-mask branch of the device input pipeline on the GPU (msml_occ_draw_mask, msml_occ_apply_mask) against the
numpy restatement of tests/maskaug_cases.py, which tests/test_maskaug_cpu.py pins bit for bit to the reference's
_add_gauss_to_mask and to Pillow.

Bounds.  Descriptors (integer words, and float words as bits) and masks: exact.  ori: the bound of
tests/test_gpu_occ_gray.py.  img: for the block type, with the light off, and for every sample that is not a mask sample,
that file's bound and nothing more -- equality, 1e-7 with Normalize, 1e-3 / 2e-3 with the light; for Gaussian light and
noise the float16 map value is where exp / log / cos of the device and of numpy may round to neighbouring float16
values, so the restatement is evaluated with the map value one float16 step down and one up and a pixel must lie between
the two results, widened by that same bound.  The envelope comes from the restatement alone."""
import numpy as np
import pytest
import torch

from tests import maskaug_cases as MC
from tests import occ_gray_cases as G
from tests.test_gpu_occ_gray import atlas_and_sets

pytestmark = pytest.mark.gpu

SEED, OFFSET, N = MC.GPU_DRAWS
CONFIGS = [s for s in G.SWITCHES if min(G.out_hw(s[1], 112, 112)[0] - 111, G.out_hw(s[1], 112, 112)[1] - 110) >= 0]
CONFIGS += [(False, None, True), (True, (111, 112), False), (False, (111, 112), True)]
_DATA = {}


def batch(n=N, seed=11):
    """(src, masked, mask) as numpy and on the device, made once."""
    if (n, seed) not in _DATA:
        src = np.random.RandomState(seed).randint(0, 256, (n, 112, 112, 3)).astype(np.uint8)
        masked, mask = MC.synthetic_renders(src)
        _DATA[(n, seed)] = (src, masked, mask) + tuple(torch.from_numpy(a).cuda() for a in (src, masked, mask))
    return _DATA[(n, seed)]


def bound(light, use_norm):
    if light:
        return 2e-3 if use_norm else 1e-3
    return 1e-7 if use_norm else 0.0


def check(got, ref, light, use_norm):
    img, msk, ori = (t.cpu().numpy() for t in got)
    (r0, rdn, rup), rmsk, rori = ref
    assert img.shape == r0.shape and msk.dtype == np.int64 and np.array_equal(msk, rmsk)          # masks: exact
    err = np.abs(ori - rori).max()
    assert (err < 1e-7) if use_norm else np.array_equal(ori, rori), err
    b = bound(light, use_norm)
    lo, hi = np.minimum(rdn, rup), np.maximum(rdn, rup)
    assert np.all(lo <= r0) and np.all(r0 <= hi)
    out = np.maximum(lo - img, img - hi).max()
    print("img: outside the envelope by", out, "(bound %g)" % b, "| from the restatement", np.abs(img - r0).max(),
          "| envelope width", (hi - lo).max())
    assert out <= b, out
    assert np.isfinite(img).all()


def test_descriptors_equal_the_restatement():
    from msml_amd import data
    atlas, osets = atlas_and_sets()
    for mode, at, sets, out_size in (("train", None, (), None), ("train", None, (), 128), ("ms1m", atlas, osets, (111, 112))):
        for p in (1.0, 0.2):
            desc = data.draw(N, SEED, OFFSET, mode, atlas=at, out_size=out_size, p_mask=p).cpu().numpy()
            ref = MC.draw(SEED, OFFSET, N, 112, 112, data.MODES[mode], sets=sets, out_size=out_size, p_mask=p)
            assert desc.dtype == ref.dtype == np.int32 and np.array_equal(desc, ref), (mode, p)
    assert (desc[:, 0] == MC.OCC_MASK).sum() not in (0, N)
    types = set(ref[ref[:, 0] == MC.OCC_MASK, 16].tolist())
    assert types <= {0, 1, 2}


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("gray,out_size,use_norm", CONFIGS)
def test_mask_samples_match_restatement(gray, out_size, use_norm, light):
    from msml_amd import data
    src, masked, mask, dsrc, dmasked, dmask = batch()
    img, msk, ori, desc = data.augment(dsrc, SEED, OFFSET, "train", 0, 36, True, light, True, None, gray, out_size, use_norm,
                                       1.0, dmasked, dmask)
    ref_desc = MC.draw(SEED, OFFSET, N, 112, 112, 0, out_size=out_size, p_mask=1.0)
    assert np.array_equal(desc.cpu().numpy(), ref_desc)
    ref = MC.apply(src, masked, mask, ref_desc, light, (), gray, out_size, use_norm, steps=(0, -1, 1))
    check((img, msk, ori), ref, light, use_norm)
    assert (msk == 0).any(dim=2).any(dim=1).all() and (msk == 1).any()
    lo = -1.0 if use_norm else 0.0
    assert img.min().item() < lo and img.max().item() > 1.0            # not clamped (:271)


@pytest.mark.parametrize("light", [False, True])
@pytest.mark.parametrize("gray,use_norm", [(True, False), (False, True)])
def test_mask_samples_horizontal_pass_alone(gray, use_norm, light):
    """out_size = (112, 116): the height stays, so the overlay runs its horizontal pass and no vertical one (CONFIGS has
    the other half, (111, 112)).  116 is the smallest multiple of 4 that holds the 110-pixel rectangle."""
    from msml_amd import data
    n, out_size = 8, (112, 116)
    src, masked, mask, dsrc, dmasked, dmask = batch(n)
    img, msk, ori, desc = data.augment(dsrc, SEED, OFFSET, "train", 0, 36, True, light, True, None, gray, out_size, use_norm,
                                       1.0, dmasked, dmask)
    ref_desc = MC.draw(SEED, OFFSET, n, 112, 112, 0, out_size=out_size, p_mask=1.0)
    assert np.array_equal(desc.cpu().numpy(), ref_desc)
    assert img.shape == (n, 1 if gray else 3, 112, 116)
    check((img, msk, ori), MC.apply(src, masked, mask, ref_desc, light, (), gray, out_size, use_norm, steps=(0, -1, 1)),
          light, use_norm)


@pytest.mark.parametrize("mode", ["train", "ms1m"])
def test_flag_consistency(mode):
    """p_mask = 0.2: the flagged set is mask_flags'; unflagged samples are the p_mask = 0 run's bits, flagged ones the
    p_mask = 1 run's."""
    from msml_amd import data
    src, masked, mask, dsrc, dmasked, dmask = batch()
    atlas = atlas_and_sets()[0] if mode == "ms1m" else None
    for kw in ({}, {"gray": True, "out_size": 128, "use_norm": False}):
        run = lambda p: data.augment(dsrc, SEED, OFFSET, mode, atlas=atlas, p_mask=p, masked=dmasked, mask=dmask, **kw)
        zero, part, full = run(0.0), run(0.2), run(1.0)
        fl = torch.from_numpy(data.mask_flags(SEED, OFFSET, N, 0.2)).cuda()
        assert 0 < fl.sum().item() < N
        assert torch.equal(part[3][:, 0] == MC.OCC_MASK, fl)
        assert not (zero[3][:, 0] == MC.OCC_MASK).any() and (full[3][:, 0] == MC.OCC_MASK).all()
        for z, p, f in zip(zero, part, full):
            assert torch.equal(p[~fl], z[~fl]) and torch.equal(p[fl], f[fl])
        assert not torch.equal(part[0][fl], zero[0][fl])
        assert torch.equal(part[2], zero[2]) and torch.equal(part[2], full[2])      # ori: the clean src face, always


def test_default_is_unchanged():
    """p_mask = 0, with and without the renders, is today's call."""
    from msml_amd import data
    src, masked, mask, dsrc, dmasked, dmask = batch()
    atlas = atlas_and_sets()[0]
    for mode, at in (("train", None), ("ms1m", atlas)):
        for kw in ({}, {"gray": True, "out_size": 128, "use_norm": False}):
            a = data.augment(dsrc, SEED, OFFSET, mode, atlas=at, **kw)
            b = data.augment(dsrc, SEED, OFFSET, mode, atlas=at, p_mask=0.0, **kw)
            c = data.augment(dsrc, SEED, OFFSET, mode, atlas=at, p_mask=0.0, masked=dmasked, mask=dmask, **kw)
            for x, y, z in zip(a, b, c):
                assert torch.equal(x, y) and torch.equal(x, z)
            # apply() alone on descriptors without a mask sample: the overlay returns at once
            d = data.apply(dsrc, a[3], atlas=at, masked=dmasked, mask=dmask, **kw)
            for x, y in zip(a[:3], d):
                assert torch.equal(x, y)


def test_rows():
    """Packed renders with rows give the bits of the full arrays; a flagged sample whose row is -1 or M is the clean one."""
    from msml_amd import data
    src, masked, mask, dsrc, dmasked, dmask = batch()
    fl = data.mask_flags(SEED, OFFSET, N, 0.2)
    idx = np.nonzero(fl)[0]
    assert len(idx) >= 3
    for kw in ({}, {"gray": True, "out_size": 128, "use_norm": False}):
        full = data.augment(dsrc, SEED, OFFSET, p_mask=0.2, masked=dmasked, mask=dmask, **kw)
        rows = np.full(N, -1, np.int32)
        rows[idx] = np.arange(len(idx))[::-1]                  # packed, in another order
        sel = torch.from_numpy(idx[::-1].copy()).cuda()
        packed = data.augment(dsrc, SEED, OFFSET, p_mask=0.2, masked=dmasked[sel].contiguous(), mask=dmask[sel].contiguous(),
                              rows=torch.from_numpy(rows).cuda(), **kw)
        for x, y in zip(full, packed):
            assert torch.equal(x, y)
        clean = data.augment(dsrc, SEED, OFFSET, "none", **kw)
        train = data.augment(dsrc, SEED, OFFSET, **kw)
        M = len(idx)
        bad = rows.copy()
        bad[idx[0]], bad[idx[1]] = -1, M
        out = data.augment(dsrc, SEED, OFFSET, p_mask=0.2, masked=dmasked[sel].contiguous(), mask=dmask[sel].contiguous(),
                           rows=torch.from_numpy(bad).cuda(), **kw)
        for i in idx[:2]:
            assert out[3][i, 0].item() == MC.OCC_MASK
            for k in range(3):          # same flip and light draws, no occluder: the "none" mode's sample
                assert torch.equal(out[k][i], clean[k][i])
        keep = np.ones(N, bool)
        keep[idx[:2]] = False
        keep = torch.from_numpy(keep).cuda()
        for x, y in zip(out[:3], full[:3]):
            assert torch.equal(x[keep], y[keep])
        assert torch.equal(out[0][~torch.from_numpy(fl).cuda()], train[0][~torch.from_numpy(fl).cuda()])


def test_batch_split():
    from msml_amd import data
    src, masked, mask, dsrc, dmasked, dmask = batch()
    for kw in ({}, {"gray": True, "out_size": 128, "use_norm": False}):
        one = data.augment(dsrc[:16], SEED, 0, p_mask=1.0, masked=dmasked[:16], mask=dmask[:16], **kw)
        a = data.augment(dsrc[:8], SEED, 0, p_mask=1.0, masked=dmasked[:8], mask=dmask[:8], **kw)
        b = data.augment(dsrc[8:16], SEED, 8, p_mask=1.0, masked=dmasked[8:16], mask=dmask[8:16], **kw)
        for x, y, z in zip(one, a, b):
            assert torch.equal(x, torch.cat([y, z]))
        assert {0, 1, 2} <= set(one[3][:, 16].tolist())


def test_refusals_of_the_entry_points():
    """The library's own checks, as msml_occ_apply_out's: a width that is no multiple of 4 and more LDS than there is."""
    from msml_amd import data
    src, masked, mask, dsrc, dmasked, dmask = batch()
    with pytest.raises(RuntimeError, match=r"not a multiple of 4"):
        data.augment(dsrc, 1, 0, p_mask=0.2, masked=dmasked, mask=dmask, gray=True, out_size=(128, 126))
    with pytest.raises(RuntimeError, match=r"bytes of LDS"):
        data.augment(dsrc, 1, 0, p_mask=0.2, masked=dmasked, mask=dmask, out_size=224)
    # the overlay's own refusals (above, msml_occ_apply_out speaks first): MSML_ERR_UNSUPPORTED, nothing launched
    from msml_amd._lib import UNSUPPORTED, call_status, load
    desc = data.draw(N, SEED, OFFSET, p_mask=1.0)
    img, msk = torch.zeros(N, 3, 128, 128, device="cuda"), torch.zeros(N, 128, 128, dtype=torch.int64, device="cuda")
    tw, th = data._out_table(112, 126, "cuda"), data._out_table(112, 128, "cuda")
    assert call_status("msml_occ_apply_mask", dmasked, dmask, None, N, desc, tw, th, img, msk, N, 112, 112, 128, 126, 0, 1,
                       1) == UNSUPPORTED
    assert "not a multiple of 4" in load().msml_last_error().decode()
    t224 = data._out_table(112, 224, "cuda")
    assert call_status("msml_occ_apply_mask", dmasked, dmask, None, N, desc, t224, t224, img, msk, N, 112, 112, 224, 224, 0,
                       1, 1) == UNSUPPORTED
    assert "needs 306944 bytes of LDS" in load().msml_last_error().decode()
    torch.cuda.synchronize()
    assert not img.any() and not msk.any()


RECIPES = [({}, (3, 112, 112)), ({"gray": True, "out_size": 128, "use_norm": False}, (1, 128, 128))]


@pytest.mark.parametrize("kw,shape", RECIPES)
def test_device_loader(kw, shape):
    from msml_amd import data
    B = 16
    source = data.SynthFaceSource(B, 1000, steps=3, pool=2, seed=9, masks=True)
    assert len(source.pool[0]) == 4
    mk = source.pool[0][2]
    assert ((mk > 0) & (mk <= 128)).any() and ((mk > 128) & (mk < 255)).any()
    seen = 0
    for k, (img, msk, ori, lab) in enumerate(data.DeviceLoaderX(source, 0, seed=77, p_mask=0.2, **kw)):
        torch.cuda.synchronize()
        assert img.shape == (B,) + shape and ori.shape == img.shape and msk.shape == (B,) + shape[1:]
        assert torch.isfinite(img).all() and torch.equal(lab.cpu(), source.pool[k % 2][3])
        fl = data.mask_flags(77, k * B, B, 0.2)
        for i in np.nonzero(fl)[0]:
            assert (msk[i] == 0).any() and (msk[i] == 1).any()
        seen += int(fl.sum())
    assert k == 2 and seen > 0


def test_loader_feeds_a_training_step():
    """Plumbing, as tests/test_gpu_occ_gray.py: one bf16 training step of the LightCNN MSML on a batch with mask samples."""
    from msml_amd import data, ops
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
        source = data.SynthFaceSource(B, classes, steps=1, pool=1, seed=9, masks=True)
        assert data.mask_flags(77, 0, B, 0.2).any()
        for img, msk, ori, lab in data.DeviceLoaderX(source, 0, seed=77, p_mask=0.2, gray=True, out_size=128, use_norm=False):
            opt.zero_grad()
            final_cls, final_seg, _ = model(img, lab)
            cls_loss = torch.nn.functional.cross_entropy(final_cls, lab)
            seg_loss = seg_crit(final_seg, msk, msk)
            (cls_loss + seg_loss).backward()
            opt.step()
            torch.cuda.synchronize()
            assert torch.isfinite(cls_loss).item() and torch.isfinite(seg_loss).item() and seg_loss.item() > 0
    finally:
        ops.WGRAD_STREAM, ops.OSB_STREAM = saved
        torch.cuda.synchronize()
