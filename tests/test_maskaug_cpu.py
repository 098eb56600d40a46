"""The facial-mask branch of the input pipeline without a GPU: tests/maskaug_cases.py (the restatement the GPU tests
compare the device with) is pinned bit for bit to the reference's own _add_gauss_to_mask (tests/golden/g12_maskaug.npz,
written by tools/make_golden_maskaug.py with every random draw logged) and to Pillow; the host-side flag draw, the normal
generator, the coverage of the GPU tests' draws and the host-side refusals are checked here too."""
import os

import numpy as np
import pytest
import torch

from oracle import occ as oo
from tests import maskaug_cases as MC
from tests import occ_gray_cases as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_maskaug.npz")


def golden_cases():
    g = np.load(GOLDEN)
    for i in range(int(g["cases"])):
        p = "c%d_" % i
        yield i, {k[len(p):]: g[k] for k in g.files if k.startswith(p)}


def test_restatement_equals_the_reference_bit_for_bit():
    """Fed with the draws the reference made, the restatement gives the reference's face (f32) and mask, every bit."""
    seen = set()
    for i, c in golden_cases():
        dr = MC.draws_from_log(c["log_names"], c["log_vals"], c.get("randn"))
        gray, size = bool(c["gray"]), int(c["size"])
        face = c["face"].astype(np.float32) / np.float32(255.0)
        out, msk = MC.add_gauss_to_mask(face, c["mask"], gray, dr)
        assert out.dtype == np.float32 and out.shape == c["out_face"].shape == (1 if gray else 3, size, size)
        assert np.array_equal(out.view(np.int32), c["out_face"].view(np.int32)), i
        assert msk.dtype == c["out_mask"].dtype == np.int32 and np.array_equal(msk, c["out_mask"]), i
        assert (msk == 0).any() and (msk == 1).any()
        assert not np.array_equal(out, face)                       # the case changes something
        seen.add((dr["type"], dr["sign"] if dr["type"] != MC.NOISE else 0, gray, size))
    assert {s[0] for s in seen} == {MC.LIGHT, MC.NOISE, MC.BLOCK}
    assert {(MC.LIGHT, 1), (MC.LIGHT, -1), (MC.BLOCK, 1), (MC.BLOCK, -1)} <= {s[:2] for s in seen}
    assert {s[2:] for s in seen} == {(False, 112), (True, 128)}


def test_golden_values_leave_the_unit_interval():
    """:271 does not clamp: the noise and the white block take values outside [0, 1]."""
    lo = min(float(c["out_face"].min()) for _, c in golden_cases())
    hi = max(float(c["out_face"].max()) for _, c in golden_cases())
    assert lo < 0 and hi > 1


@pytest.mark.parametrize("oh,ow", [(112, 112), (128, 128), (111, 112), (120, 110)])
def test_resized_binarised_mask_equals_pillow(oh, ow):
    from PIL import Image
    src = np.random.RandomState(3).randint(0, 256, (4, 112, 112, 3)).astype(np.uint8)
    _, mask = MC.synthetic_renders(src)
    assert ((mask > 0) & (mask <= 128)).any() and ((mask > 128) & (mask < 255)).any()     # both sides of 128 on the edge
    for m in mask:
        pil = np.array(Image.fromarray(m).resize((ow, oh), Image.BILINEAR))
        mine = G.resize_bilinear(m, oh, ow)
        assert np.array_equal(mine, pil)
        assert np.array_equal(MC.binarise(mine), np.where(pil <= 128, 0, 255))
        if (oh, ow) != (112, 112):
            assert not np.array_equal(MC.binarise(mine) == 255, mine == 255)    # not the != 255 rule of the occluders


def test_mask_flags_is_the_restated_draw():
    from msml_amd import data
    for seed, offset, p in ((1234, 5000, 0.2), (7, 0, 0.5), (2 ** 40 + 3, 10 ** 9, 0.2), (1, 0, 1.0)):
        got = data.mask_flags(seed, offset, 300, p)
        want = np.array([MC.flagged(seed, offset + i, p) for i in range(300)])
        assert got.dtype == bool and np.array_equal(got, want)
    assert not data.mask_flags(1, 0, 50, 0.0).any() and data.mask_flags(1, 0, 50, 1.0).all()


def test_flagged_share():
    """100 000 indices at p = 0.2: 5 sigma of the binomial is 5 * sqrt(0.2 * 0.8 / 1e5) = 0.0063."""
    from msml_amd import data
    share = data.mask_flags(1234, 0, 100000, 0.2).mean()
    print("flagged share", share)
    assert abs(share - 0.2) < 0.0063


def test_normal_generator_is_normal():
    from scipy import stats
    ys, xs = np.mgrid[0:250, 0:400]
    z = MC.normals(int(MC.noise_key(1234, 5000)), xs, ys).astype(np.float64).ravel()
    assert z.size == 100000
    p = stats.kstest(z, "norm").pvalue
    print("KS p", p, "mean", z.mean(), "std", z.std())
    assert p > 1e-3
    # another image, another stream
    z2 = MC.normals(int(MC.noise_key(1234, 5001)), xs, ys).astype(np.float64).ravel()
    assert abs(np.corrcoef(z, z2)[0, 1]) < 0.02


def test_gpu_draws_cover_every_path():
    types, signs, jit = MC.coverage(*MC.GPU_DRAWS)
    assert types == {MC.LIGHT, MC.NOISE, MC.BLOCK}
    assert signs == {(MC.LIGHT, 1), (MC.LIGHT, -1), (MC.BLOCK, 1), (MC.BLOCK, -1)}
    assert (0, 0, 0) in jit and any(sum(j) >= 1 for j in jit)


def test_restated_descriptor_layout():
    """Words 1-7 and 12-15 of a mask descriptor are zero (the apply kernels index the patch buffer with words 1-4), the
    rectangle lies inside 110 x 111, and a flagged descriptor does not depend on p_mask."""
    seed, offset, n = MC.GPU_DRAWS
    a = MC.draw(seed, offset, n, 112, 112, 0, p_mask=1.0)
    b = MC.draw(seed, offset, n, 112, 112, 0, p_mask=0.2)
    base = MC.draw(seed, offset, n, 112, 112, 0)
    assert (a[:, 0] == MC.OCC_MASK).all() and not (a[:, 1:8] != 0).any() and not (a[:, 12:16] != 0).any()
    assert (a[:, 17] >= 20).all() and (a[:, 19] <= 110).all() and (a[:, 18] >= 1).all() and (a[:, 20] <= 111).all()
    assert (a[:, 17] < a[:, 19]).all() and (a[:, 18] < a[:, 20]).all()
    fl = b[:, 0] == MC.OCC_MASK
    assert 0 < fl.sum() < n
    assert np.array_equal(b[fl], a[fl]) and np.array_equal(b[~fl], base[~fl])
    assert np.array_equal(base, G.draw(seed, offset, n, 112, 112, 0))
    assert oo.OCC_OBJECT < MC.OCC_MASK


def test_host_side_refusals():
    """ValueError before any launch (CPU tensors never reach one): no renders, mismatched shapes, an output too small."""
    from msml_amd import data
    src = torch.zeros(4, 112, 112, 3, dtype=torch.uint8)
    masked, mask = torch.zeros(4, 112, 112, 3, dtype=torch.uint8), torch.zeros(4, 112, 112, dtype=torch.uint8)
    with pytest.raises(ValueError, match="needs the rendered faces"):
        data.augment(src, 1, 0, p_mask=0.2)
    with pytest.raises(ValueError, match="come together"):
        data.augment(src, 1, 0, p_mask=0.2, masked=masked)
    with pytest.raises(ValueError, match="masked must be"):
        data.augment(src, 1, 0, p_mask=0.2, masked=masked[:, :100], mask=mask)
    with pytest.raises(ValueError, match="mask must be"):
        data.augment(src, 1, 0, p_mask=0.2, masked=masked, mask=mask[:, :, :100])
    with pytest.raises(ValueError, match="mask must be"):
        data.augment(src, 1, 0, p_mask=0.2, masked=masked, mask=mask.float())
    with pytest.raises(ValueError, match="one render per sample"):
        data.augment(src, 1, 0, p_mask=0.2, masked=masked[:3], mask=mask[:3])
    with pytest.raises(ValueError, match="rows must be"):
        data.augment(src, 1, 0, p_mask=0.2, masked=masked[:3], mask=mask[:3], rows=torch.zeros(4, dtype=torch.int64))
    for out_size in (96, (110, 112), (112, 108), (112, 96)):
        with pytest.raises(ValueError, match="at least 111 x 110"):
            data.augment(src, 1, 0, p_mask=0.2, masked=masked, mask=mask, out_size=out_size)
        with pytest.raises(ValueError, match="at least 111 x 110"):
            data.draw(4, 1, 0, p_mask=0.2, out_size=out_size, device="cpu")
    with pytest.raises(ValueError, match="not a probability"):
        data.augment(src, 1, 0, p_mask=1.5, masked=masked, mask=mask)
    with pytest.raises(ValueError, match="must yield"):
        loader = data.DeviceLoaderX.__new__(data.DeviceLoaderX)
        loader.p_mask, loader.cfg, loader.iter = 0.2, (1, "train", 0, 36, True, True, True), iter([(src, torch.zeros(4))])
        loader.preload()
