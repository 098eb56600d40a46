"""Gray / resized / unnormalised output of the device input pipeline, CPU side: the restatement of the new stages
(tests/occ_gray_cases.py) pinned bit for bit to Pillow -- the library the reference's dataset class calls
(convert('L'), transforms.Resize -> Image.resize(BILINEAR)) -- and the host-side tables of the product pinned to the
restatement.  tests/test_gpu_occ_gray.py then compares the kernels with the restatement."""
import numpy as np
import pytest
from PIL import Image

from oracle import occ as oo
from tests import occ_gray_cases as G

SIZES = [128, 96, 144, (112, 96), (128, 112), 112]


def test_rgb_to_l_is_pil_convert():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (64, 97, 3), dtype=np.uint8)
    assert np.array_equal(G.rgb_to_l(a), np.array(Image.fromarray(a, mode="RGB").convert("L")))
    levels = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)[None]          # the 256 gray levels
    assert np.array_equal(G.rgb_to_l(levels), np.array(Image.fromarray(levels, mode="RGB").convert("L")))
    assert np.array_equal(G.rgb_to_l(levels)[0], np.arange(256))
    prim = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0],
                      [255, 255, 255]]], np.uint8)
    assert np.array_equal(G.rgb_to_l(prim), np.array(Image.fromarray(prim, mode="RGB").convert("L")))
    assert G.rgb_to_l(prim)[0].tolist() == [76, 150, 29, 226, 179, 105, 0, 255]


@pytest.mark.parametrize("out_size", SIZES)
def test_resize_bilinear_is_pil_resize(out_size):
    oh, ow = G.out_hw(out_size, 112, 112)
    rng = np.random.default_rng(1)
    for trial in range(3):
        lum = rng.integers(0, 256, (112, 112), dtype=np.uint8)
        rgb = rng.integers(0, 256, (112, 112, 3), dtype=np.uint8)
        if trial == 2:                                    # a 0 / 255 mask, as the pipeline resizes it
            lum = np.where(rng.random((112, 112)) < 0.3, 0, 255).astype(np.uint8)
        assert np.array_equal(G.resize_bilinear(lum, oh, ow),
                              np.array(Image.fromarray(lum, mode="L").resize((ow, oh), Image.BILINEAR)))
        assert np.array_equal(G.resize_bilinear(rgb, oh, ow),
                              np.array(Image.fromarray(rgb, mode="RGB").resize((ow, oh), Image.BILINEAR)))
    if (oh, ow) == (112, 112):
        assert np.array_equal(G.resize_bilinear(lum, oh, ow), lum)                   # a copy


def test_product_tables():
    """data.resample_table(filter="bilinear") equals the restatement's tables (at most 3 taps for the sizes in use);
    the bicubic default is what it was."""
    from msml_amd import data
    for insz, outsz in [(112, 128), (112, 96), (112, 144), (112, 224), (112, 100), (128, 112), (96, 128)]:
        tab = data.resample_table(insz, outsz, filter="bilinear")
        assert tab.shape == (outsz, data.RT_WORDS) and tab.dtype == np.int32
        rows = G.bilinear_coeffs(insz, outsz)
        for xx, (xmin, cnt, k) in enumerate(rows):
            assert tab[xx, 0] == xmin and tab[xx, 1] == cnt and list(tab[xx, 2:2 + cnt]) == k
            assert not tab[xx, 2 + cnt:].any() and xmin + cnt <= insz
        if (insz, outsz) in [(112, 128), (112, 96), (112, 144)]:
            assert max(r[1] for r in rows) <= 3
    for insz, outsz in [(80, 67), (80, 82), (40, 33), (40, 41), (90, 81), (55, 110), (55, 56)]:
        tab = data.resample_table(insz, outsz)
        assert np.array_equal(tab, data.resample_table(insz, outsz, filter="bicubic"))
        for xx, (xmin, cnt, k) in enumerate(oo.resize_coeffs(insz, outsz)):
            assert tab[xx, 0] == xmin and tab[xx, 1] == cnt and list(tab[xx, 2:2 + cnt]) == k
    with pytest.raises(KeyError):
        data.resample_table(112, 128, filter="nearest")


def _descriptors():
    """One descriptor of every kind the device draws, flipped and not: rect, ellipse, polygon, block, none and the
    three texture kinds (from the draws of the generator, so geometry and texture sizes are real ones)."""
    sets = G.oracle_sets(G.synthetic_sets())
    pool = np.concatenate([oo.draw(21, 0, 200, 112, 112, 5, sets=sets), oo.draw(21, 500, 40, 112, 112, 2, 20, 41)])
    out = []
    for kind in (oo.OCC_RECT, oo.OCC_ELLIPSE, oo.OCC_POLY, oo.OCC_BLOCK, oo.OCC_NONE, oo.OCC_GLASSES, oo.OCC_SCARF,
                 oo.OCC_OBJECT):
        for fl in (0, 1):
            rows = pool[(pool[:, 0] == kind) & (pool[:, 8] == fl)]
            assert len(rows), (kind, fl)
            out.append(rows[0])
    return np.stack(out), sets


@pytest.mark.parametrize("gray,out_size,use_norm", G.SWITCHES + [(True, 144, False), (False, (128, 112), False)])
def test_whole_sample_against_pil(gray, out_size, use_norm):
    """The reference's literal sequence with PIL calls on the occluded face and 0 / 255 mask that oracle.occ builds:
    convert('L'), resize, transpose(FLIP_LEFT_RIGHT), np.array(...) / 255, mask != 255 -> 0 -- against the
    restatement, exact with the light off."""
    desc, sets = _descriptors()
    n = len(desc)
    src = np.random.RandomState(5).randint(0, 256, (n, 112, 112, 3)).astype(np.uint8)
    oh, ow = G.out_hw(out_size, 112, 112)
    img, msk, ori = G.apply(src, desc, False, True, sets, gray, out_size, use_norm)
    assert img.shape == (n, 1 if gray else 3, oh, ow) and msk.shape == (n, oh, ow) and ori.shape == img.shape
    for i in range(n):
        pix, m = G.occlude(src[i], desc[i], sets)
        ims = [Image.fromarray(pix, mode="RGB"), Image.fromarray(m, mode="L"), Image.fromarray(src[i], mode="RGB")]
        if gray:
            ims[0], ims[2] = ims[0].convert("L"), ims[2].convert("L")
        ims = [im.resize((ow, oh), Image.BILINEAR) for im in ims]
        if desc[i, 8]:
            ims = [im.transpose(Image.FLIP_LEFT_RIGHT) for im in ims]
        face, mask, clean = (np.array(im) for im in ims)
        t = (face.astype(np.float32) / np.float32(255.0)).reshape(oh, ow, -1).transpose(2, 0, 1)
        c = (clean.astype(np.float32) / np.float32(255.0)).reshape(oh, ow, -1).transpose(2, 0, 1)
        if use_norm:
            t, c = (t - np.float32(0.5)) / np.float32(0.5), (c - np.float32(0.5)) / np.float32(0.5)
        assert np.array_equal(img[i], t), (i, desc[i, 0])
        assert np.array_equal(ori[i], c), (i, desc[i, 0])
        assert np.array_equal(msk[i], np.where(mask != 255, 0, 1)), (i, desc[i, 0])
        if desc[i, 0] != oo.OCC_NONE:
            assert (msk[i] == 0).any()
        else:
            assert (msk[i] == 1).all()                    # an all-clean neighbourhood stays exactly 255


def test_mask_is_interpolated_not_rescaled():
    """A 40 x 70 rectangle at 112 (2 800 px) covers 3 807 px at 128 -- every output pixel the triangle filter mixes with an
    occluded one -- not the 3 657 of the rectangle's area rescaled by (128 / 112)^2, nor the count of a nearest-neighbour scaling of the mask."""
    d = np.zeros((1, oo.DESC_WORDS), np.int32)
    d[0, :8] = [oo.OCC_RECT, 30, 20, 40, 70, 9, 99, 199]
    src = np.random.RandomState(2).randint(0, 256, (1, 112, 112, 3)).astype(np.uint8)
    _, m = G.occlude(src[0], d[0])
    assert (m == 0).sum() == 2800
    _, msk, _ = G.apply(src, d, False, False, (), True, 128, False)
    pil = np.array(Image.fromarray(m, mode="L").resize((128, 128), Image.BILINEAR))
    nearest = np.array(Image.fromarray(m, mode="L").resize((128, 128), Image.NEAREST))
    assert (msk[0] == 0).sum() == (pil != 255).sum() == 3807
    assert (msk[0] == 0).sum() > (nearest != 255).sum() >= 45 * 80          # strictly more than nearest-neighbour scaling
    assert (msk[0] == 0).sum() > 3657 == int(2800 * (128 / 112) ** 2)       # ... and than the rescaled geometry's area
    assert not (msk[0][nearest != 255] == 1).any()        # a superset of the nearest-neighbour mask


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5, 6])
def test_descriptors_with_an_output_size(mode):
    sets = G.oracle_sets(G.synthetic_sets())
    ref = oo.draw(31, 900, 120, 112, 112, mode, sets=sets)
    assert np.array_equal(G.draw(31, 900, 120, 112, 112, mode, sets=sets, out_size=112), ref)      # word for word
    assert np.array_equal(G.draw(31, 900, 120, 112, 112, mode, sets=sets), ref)
    for out_size in (128, (112, 96), (96, 144)):
        oh, ow = G.out_hw(out_size, 112, 112)
        d = G.draw(31, 900, 120, 112, 112, mode, sets=sets, out_size=out_size)
        same = np.ones(oo.DESC_WORDS, bool)
        same[9:11] = False
        assert np.array_equal(d[:, same], ref[:, same])
        c = np.ascontiguousarray(d[:, 9:11]).view(np.float32)
        assert (c[:, 0] >= 0).all() and (c[:, 0] < ow).all() and (c[:, 1] >= 0).all() and (c[:, 1] < oh).all()
        if ow != 112:
            assert (d[:, 9] != ref[:, 9]).any()
        assert np.allclose(c[:, 0] / ow, np.ascontiguousarray(ref[:, 9:10]).view(np.float32)[:, 0] / 112, atol=1e-6)
