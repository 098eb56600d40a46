"""GPU tests of the face alignment in front of the template evaluation (msml_amd/ijb.py, csrc/align.hip) against the
numpy restatement of tests/align_cases.py: the warp and the input pairs bit for bit, the chain from decoded images and
landmarks to the [N][2E] features against the model run on the oracle's input pairs.  What is NOT shown here: equality
with a real OpenCV / skimage build (neither was available; see tests/align_cases.py)."""
import numpy as np
import pytest
import torch

from tests import align_cases as A
from tests import ijb_cases as C

pytestmark = pytest.mark.gpu
UNSUPPORTED = -4


def _draws(content, seed=1):
    """48 sources: the six sizes of align_cases.SIZES x 8 random similarity draws each, shuffled so that sizes mix in
    the buffer.  content: "random" uint8 noise or the "smooth" image."""
    rng = np.random.default_rng(seed)
    imgs, minv = [], []
    for h, w in A.SIZES:
        lm, _ = A.random_landmarks(rng, 8, (h, w))
        for i in range(8):
            imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if content == "random" else A.smooth_image(h, w))
            minv.append(A.invert(A.umeyama(lm[i], A.DST112)[:2]))
    order = rng.permutation(len(imgs))
    return [imgs[i] for i in order], np.stack([minv[i] for i in order])


_CACHE = {}


def _case(content, oh, ow):
    """(images, minv, oracle output without the colour swap), computed once per process."""
    key = (content, oh, ow)
    if key not in _CACHE:
        imgs, minv = _draws(content)
        _CACHE[key] = (imgs, minv, np.stack([A.warp(im, m, oh, ow, swap_rb=False) for im, m in zip(imgs, minv)]))
    return _CACHE[key]


def _warp(imgs, minv, oh, ow, swap, pitch_extra=0):
    from msml_amd._lib import call
    flat, meta = A.pack(imgs, pitch_extra)
    src = torch.from_numpy(flat).cuda()
    dst = torch.full((len(imgs), oh, ow, 3), 0x77, dtype=torch.uint8, device="cuda")
    call("msml_align_warp", src, torch.from_numpy(meta).cuda(), torch.from_numpy(np.ascontiguousarray(minv)).cuda(), dst,
         len(imgs), oh, ow, swap)
    return dst.cpu().numpy()


def _same(got, want, name):
    bad = int((got != want).sum())
    print("%s: %d of %d bytes differ" % (name, bad, want.size))
    return bad == 0


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("content", ["random", "smooth"])
def test_warp_equals_the_oracle_bit_for_bit(content, swap):
    imgs, minv, want = _case(content, 112, 112)
    got = _warp(imgs, minv, 112, 112, swap)
    assert _same(got, want[..., ::-1] if swap else want, "warp 112 %s swap=%d" % (content, swap))
    if content == "random" and swap == 0:
        inside = float((want != 0).any(-1).mean())
        print("share of output pixels that see the source: %.2f" % inside)
        assert 0.2 < inside < 0.95                         # the cases hold both inside and border pixels


@pytest.mark.parametrize("oh,ow", [(128, 128), (8, 12)])
def test_warp_other_output_sizes(oh, ow):
    imgs, minv, want = _case("random", oh, ow)
    assert _same(_warp(imgs, minv, oh, ow, 1), want[..., ::-1], "warp %dx%d" % (oh, ow))


def test_warp_row_pitch_single_image_and_exact_geometry():
    rng = np.random.default_rng(4)
    imgs, minv, want = _case("random", 112, 112)
    # a pitch larger than 3 W (and not a multiple of 4), one image per size
    first = [next(i for i, im in enumerate(imgs) if im.shape[:2] == hw) for hw in A.SIZES]
    sub, sub_m = [imgs[i] for i in first], minv[first]
    assert _same(_warp(sub, sub_m, 112, 112, 0, pitch_extra=7), want[first], "pitch 3W+7")
    # N = 1
    assert _same(_warp(imgs[:1], minv[:1], 112, 112, 1), want[:1, ..., ::-1], "N=1")
    face = rng.integers(0, 256, (112, 112, 3), dtype=np.uint8)
    # identity: the output is the input
    eye = A.invert([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert _same(_warp([face], eye[None], 112, 112, 0)[0], face, "identity")
    assert _same(_warp([face], eye[None], 112, 112, 1)[0], face[..., ::-1], "identity, swapped")
    # an integer shift by 56 to the right: the left half is exactly 0, the right half the left half of the source
    shift = A.invert([[1.0, 0.0, 56.0], [0.0, 1.0, 0.0]])
    got = _warp([face], shift[None], 112, 112, 0)[0]
    assert (got[:, :56] == 0).all() and np.array_equal(got[:, 56:], face[:, :56])
    assert np.array_equal(got, A.warp(face, shift, 112, 112, swap_rb=False))


def test_warp_degenerate_and_saturating_matrices():
    """D == 0 (the inverse map is all zero: every pixel reads source pixel (0, 0)) and coefficients of 1e12, whose
    fixed-point terms saturate: the int16 clamp and the per-tap bounds keep every read inside the image."""
    rng = np.random.default_rng(8)
    imgs = [rng.integers(1, 256, (37, 53, 3), dtype=np.uint8) for _ in range(6)]
    mats = [A.invert([[2.0, 4.0, 1.0], [1.0, 2.0, 5.0]]),
            np.array([1e12, 0.0, 0.0, 0.0, 1e12, 0.0]), np.array([-1e12, 3.0, 7.0, 2.0, -1e12, 1e12]),
            np.array([0.5, 1e12, -1e12, 1e12, 0.25, 5.0]), np.array([1e-3, 0.0, 1e12, 0.0, 1e-3, -1e12]),
            np.array([2097151.9, 0.0, 0.0, 0.0, 2097151.9, 0.0])]
    minv = np.stack(mats)
    assert np.array_equal(minv[0][[0, 1, 3, 4]], np.zeros(4))
    want = np.stack([A.warp(im, m, 112, 112, swap_rb=False) for im, m in zip(imgs, minv)])
    got = _warp(imgs, minv, 112, 112, 0)
    assert _same(got, want, "degenerate / saturating")
    assert (got[0] == imgs[0][0, 0]).all()
    assert (got[1][1:, 1:] == 0).all() and np.array_equal(got[1][0, 0], imgs[1][0, 0])


def test_warp_refusals_leave_dst_alone():
    from msml_amd import _lib
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    meta = torch.tensor([[0, 8, 8, 24]], dtype=torch.int64, device="cuda")
    minv = torch.tensor([[1.0, 0, 0, 0, 1, 0]], dtype=torch.float64, device="cuda")
    dst = torch.full((300 * 256 * 3,), 0x77, dtype=torch.uint8, device="cuda")
    for n, oh, ow in ((1, 112, 10), (1, 300, 112), (0, 112, 112), (1, 2, 112), (1, 112, 260)):
        assert _lib.call_status("msml_align_warp", src, meta, minv, dst, n, oh, ow, 1) == UNSUPPORTED, (n, oh, ow)
    torch.cuda.synchronize()
    assert bool((dst == 0x77).all())
    assert _lib.call_status("msml_align_warp", src, meta, minv, dst, 1, 8, 8, 1) == 0


def test_align_faces_python_path():
    """pack_images + align_matrices + align_faces against the oracle fed with the same matrices (their agreement with
    the restated estimate is the CPU tests' subject); strided inputs, out_size 112 and 128, bgr on and off."""
    from msml_amd import ijb
    rng = np.random.default_rng(12)
    imgs, lms = [], []
    for h, w in A.SIZES:
        lm, _ = A.random_landmarks(rng, 1, (h, w))
        big = rng.integers(0, 256, (h + 3, w + 5, 3), dtype=np.uint8)
        imgs.append(big[2:h + 2, 1:w + 1])                     # a view with a pitch of its own
        lms.append(lm[0])
    buf, meta = ijb.pack_images(imgs)
    for size, bgr in ((112, True), (128, False)):
        m = ijb.align_matrices(np.stack(lms), size)
        got = ijb.align_faces(buf, meta, m, size, bgr=bgr)
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (6, size, size, 3)
        want = np.stack([A.warp(im, A.invert(mm), size, size, swap_rb=bgr) for im, mm in zip(imgs, m)])
        assert _same(got.cpu().numpy(), want, "align_faces %d" % size)
    with pytest.raises(ValueError):                            # the last image no longer fits
        ijb.align_faces(buf[:-4], meta, m, 112)


def _faces(n, s, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, s, s, 3), dtype=np.uint8)


@pytest.mark.parametrize("n,s", [(5, 112), (3, 128)])
@pytest.mark.parametrize("lo,hi", [(0, 1), (40, 41), (90, 91), (None, None)])
def test_pairs_equal_the_restatement_bit_for_bit(n, s, lo, hi):
    from msml_amd import data, ijb
    faces = _faces(n, s, 20 + n)
    dev = torch.from_numpy(faces).cuda()
    desc = None if lo is None else data.draw(n, 5, 100, mode="block", lo=lo, hi=hi, flip=False, size=s)
    got = ijb.pair_inputs(dev, desc)
    d = None if desc is None else desc.cpu().numpy()
    if lo == 0 or lo is None:
        assert d is None or (d[:, 0] == 0).all()
    else:
        assert (d[:, 0] == 3).all() and (d[:, 3] == d[:, 4]).all() and (d[:, 3] > s // 2).all()
    want = A.pairs(faces, d)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2 * n, 3, s, s)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(got[1::2], got[0::2].flip(-1))
    if lo is not None:                                     # eval_inputs is draw + pair_inputs
        assert torch.equal(ijb.eval_inputs(dev, 5, 100, lo, hi), got)
    else:
        assert torch.equal(ijb.eval_inputs(dev, lo=None, hi=None), got)


def test_pairs_refuse_other_descriptor_kinds():
    from msml_amd import _lib, data, ijb
    faces = torch.from_numpy(_faces(4, 112, 3)).cuda()
    desc = data.draw(4, 1, 0, mode="block", lo=40, hi=41, flip=False, size=112)
    desc[2, 0] = 1                                         # a rectangle of the training mix
    with pytest.raises(ValueError):
        ijb.pair_inputs(faces, desc)
    # the entry point itself never hands such an image on as if it were clean
    out = torch.zeros(8, 3, 112, 112, device="cuda")
    assert _lib.call_status("msml_align_pairs", faces, desc, out, 4, 112, 112) == 0
    assert bool(torch.isnan(out[4:6]).all()) and bool(torch.isfinite(out[:4]).all()) and bool(torch.isfinite(out[6:]).all())
    assert _lib.call_status("msml_align_pairs", faces, desc, out, 4, 112, 110) == UNSUPPORTED


def test_chain_from_images_and_landmarks_to_template_scores():
    """align_and_embed on 12 synthetic sources, iresnet18 MSML in exact f32: equal to the model run on the oracle's
    input pairs within ijb_cases.tolerance (the f64-accumulation bound of the template tests, here for one row of E
    values: the inputs are bit-equal and the model is the same, so the features should be too); two calls give the
    same bits; batches of 5 and of 12 give the same rows; the features go through evaluate_templates on the device."""
    from msml_amd import data, ijb
    from msml_amd.backbones import MSML
    from oracle.fill import fill_module
    peer = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
    torch.manual_seed(0)
    model = fill_module(MSML("iresnet18", "unet", (1, 1, 1, 1), 8, fp16=False, fm_params=(3, 2, "sigmoid", "mul"),
                             header_type="AMArcFace", peer_params=peer)).cuda().eval()
    rng = np.random.default_rng(31)
    sizes = [(250, 250), (112, 112), (480, 640), (37, 53)] * 3
    imgs = [A.smooth_image(h, w) ^ rng.integers(0, 16, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    lms = np.concatenate([A.random_landmarks(rng, 1, hw)[0] for hw in sizes])
    feats = ijb.align_and_embed(model, imgs, lms, batch=12, lo=40, hi=41, seed=9)
    assert feats.is_cuda and feats.dtype == torch.float32 and feats.shape[0] == 12 and feats.shape[1] % 2 == 0
    e = feats.shape[1] // 2
    # the oracle's input pairs through the same model
    m = ijb.align_matrices(lms)
    faces = np.stack([A.warp(im, A.invert(A.umeyama(l, A.DST112)[:2]), 112, 112) for im, l in zip(imgs, lms)])
    assert np.array_equal(faces, np.stack([A.warp(im, A.invert(mm), 112, 112) for im, mm in zip(imgs, m)]))
    desc = data.draw(12, 9, 0, mode="block", lo=40, hi=41, flip=False, size=112).cpu().numpy()
    x = torch.from_numpy(A.pairs(faces, desc)).cuda()
    with torch.no_grad():
        want = model(x)[0].float().reshape(12, 2 * e)
    tol = C.tolerance(1, e)
    err = float((feats - want).abs().max())
    print("chain vs model on the oracle's pairs: max abs diff %.3e (bound %.3e), |f| max %.3f"
          % (err, tol, float(want.abs().max())))
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 1e-3
    assert err <= tol
    again = ijb.align_and_embed(model, imgs, lms, batch=12, lo=40, hi=41, seed=9)
    assert torch.equal(again, feats)
    by5 = ijb.align_and_embed(model, imgs, lms, batch=5, lo=40, hi=41, seed=9)
    err5 = float((by5 - feats).abs().max())
    print("batch 5 vs batch 12: max abs diff %.3e" % err5)
    assert err5 <= tol
    # on to the template protocol without leaving the device
    templates = np.array([1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4])
    medias = np.arange(12)
    p1, p2, label = np.array([1, 1, 2, 3]), np.array([2, 3, 4, 4]), np.array([1, 0, 0, 1])
    out = ijb.evaluate_templates(feats, templates, medias, p1, p2, label)
    assert out["scores"].is_cuda and out["scores"].shape == (4,) and bool(torch.isfinite(out["scores"]).all())
    assert out["template_feats"].shape == (4, e) and 0.0 <= out["auc"] <= 1.0
