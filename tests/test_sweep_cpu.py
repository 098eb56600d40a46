"""CPU tests of the test.py evaluation inputs: the restatement of tests/sweep_cases.py against hand-computed answers and
against PIL, the host-side refusals of msml_amd.verification.eval_pairs and the sweep's seed mix.  No GPU."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import sweep_cases as S


def test_crop_origins_and_pad_split_by_hand():
    assert [S.crop_origin(d) for d in (0, 1, 2, 3, 4, 5, 7)] == [0, 0, 1, 2, 2, 2, 4]
    assert S.center_crop_geometry(112, 128) == (8, 8, 0)
    assert S.center_crop_geometry(113, 128) == (7, 8, 0)
    assert S.center_crop_geometry(115, 128) == (6, 7, 0)
    assert S.center_crop_geometry(117, 112) == (0, 0, 2) and S.center_crop_geometry(115, 112) == (0, 0, 2)
    assert S.center_crop_geometry(112, 112) == (0, 0, 0)


def test_center_crop_against_a_brute_force_table():
    """Every (in, out) in 1..40: the cropped row of a ramp image equals the ramp indexed by the stated arithmetic."""
    for insz in range(1, 41):
        ramp = np.arange(1, insz + 1, dtype=np.uint8)                 # 0 is the padding's colour
        img = Image.fromarray(np.repeat(ramp[None, :, None], 3, 2).repeat(2, 0))
        for outsz in range(1, 41):
            got = np.asarray(S.center_crop(img, 2, outsz))[0, :, 0]
            if outsz > insz:
                lo = (outsz - insz) // 2
                want = np.zeros(outsz, np.uint8)
                want[lo:lo + insz] = ramp
                assert outsz - insz - lo == (outsz - insz + 1) // 2
            else:
                d = insz - outsz
                origin = d // 2 if d % 2 == 0 else (d // 2 + (d // 2) % 2)      # half to even, in integers
                want = ramp[origin:origin + outsz]
            assert np.array_equal(got, want), (insz, outsz)


def test_mirror_then_crop_differs_from_crop_then_mirror():
    """A 4 x 4 image cropped to 4 x 3: the difference of 1 gives origin 0, so the crop keeps columns 0..2 -- of the
    mirrored image for the mirrored row, which are source columns 3, 2, 1, not the mirror 2, 1, 0 of the plain crop."""
    src = np.zeros((1, 4, 4, 3), np.uint8)
    src[0, :, :, 0] = np.array([10, 20, 30, 40], np.uint8)[None, :]
    # the kernel's width must be a multiple of 4, the restatement's need not
    rows, _, _ = S.reference_rows(src, None, 4, 3, gray=0, norm=0)
    plain = np.rint(rows[0, 0, 0] * 255).astype(int).tolist()
    mirrored = np.rint(rows[1, 0, 0] * 255).astype(int).tolist()
    assert plain == [10, 20, 30] and mirrored == [40, 30, 20] and mirrored != plain[::-1]


def test_gray_f_paste_rule_is_what_pil_stores():
    v = np.arange(-300, 600.25, 0.25)
    base = Image.fromarray(np.full((1, v.size), 7, np.uint8))
    blk = Image.fromarray(v.reshape(1, -1))
    assert blk.mode == "F" and base.mode == "L"
    base.paste(blk, (0, 0))
    assert np.array_equal(np.asarray(base)[0], S.f_paste_byte(v))
    # the value is rounded to f32 BEFORE the clip: 254.999995 is 255.0 in f32
    w = np.array([254.999995, 254.99999, 0.9999999999, 1e-9, -1e-9, 255.9])
    assert S.f_paste_byte(w).tolist() == [255, 254, 1, 0, 0, 255]
    b2 = Image.fromarray(np.zeros((1, w.size), np.uint8))
    b2.paste(Image.fromarray(w.reshape(1, -1)), (0, 0))
    assert np.asarray(b2)[0].tolist() == [255, 254, 1, 0, 0, 255]


def test_reference_rows_known_answers():
    """Gray + pad + white block + NB by hand on a constant image."""
    src = np.full((2, 4, 4, 3), 100, np.uint8)
    desc = np.zeros((4, 64), np.int32)
    desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3], desc[:, 4] = 3, 1, 2, 2, 2
    rows, near, drawn = S.reference_rows(src, desc, 6, 8, gray=1, norm=0, fill="white")
    assert rows.shape == (4, 1, 6, 8) and not near.any() and drawn == 0
    want = np.zeros((6, 8), np.float32)
    want[1:5, 2:6] = np.float32(100) / np.float32(255)               # L of (100, 100, 100) is 100; pad 1 / 1 and 2 / 2
    want[2:4, 1:3] = 1.0                                             # the block, in OUTPUT coordinates, over the padding too
    assert np.array_equal(rows[0, 0], want) and np.array_equal(rows[3, 0], want)
    nb, _, _ = S.reference_rows(src, desc, 4, 4, norm=1, fill="black", protocol="NB", index0=1)
    assert (nb[0:2] == np.float32((np.float32(100) / np.float32(255) - np.float32(0.5)) / np.float32(0.5))).all()
    assert (nb[2:4, :, 2:4, 1:3] == -1.0).all() and (nb[2:4, :, 0:2] != -1.0).all()        # image 1 + 1 is even


def test_gauss_normals_and_block_bytes():
    z = S.normals(3, 5, 106, 106, 3)
    assert z.shape == (106, 106, 3) and abs(z.mean()) < 0.02 and abs(z.var() - 1.0) < 0.03
    assert not np.array_equal(z, S.normals(3, 4, 106, 106, 3)) and not np.array_equal(z, S.normals(4, 5, 106, 106, 3))
    assert np.array_equal(z[:50, :60], S.normals(3, 5, 50, 60, 3))   # a function of the position, not of the block size
    rgb = np.asarray(S.block_image("gauss", "RGB", 106, 106, z))
    t = np.trunc(z * 255).astype(np.int64)
    assert np.array_equal(rgb, (t % 256).astype(np.uint8))
    img = Image.fromarray(np.zeros((106, 106), np.uint8))
    img.paste(S.block_image("gauss", "L", 106, 106, z[:, :, :1]), (0, 0))
    assert np.array_equal(np.asarray(img), S.f_paste_byte(z[:, :, 0] * 255))


def test_eval_pairs_refuses_bad_arguments_on_the_host():
    from msml_amd import verification as V
    ok = torch.zeros(2, 112, 112, 3, dtype=torch.uint8)
    bad = [
        (dict(src=ok, fill="grey"), "fill"),
        (dict(src=ok, protocol="XB"), "protocol"),
        (dict(src=ok, protocol="NB", gray=True), "NB"),
        (dict(src=ok, lo=10, hi=None), "lo and hi"),
        (dict(src=ok, lo=50, hi=40), "block range"),
        (dict(src=ok, index0=-1), "index0"),
        (dict(src=ok.float()), "uint8"),
        (dict(src=ok[:, :, :, :2]), "uint8"),
        (dict(src=ok.numpy()), "uint8"),
        (dict(src=ok[:, ::2]), "contiguous"),
        (dict(src=ok, out_size=(112, 110)), "multiple of 4"),
        (dict(src=ok, out_size=300), "sizes"),
        (dict(src=torch.zeros(2, 2, 112, 3, dtype=torch.uint8)), "sizes"),
        (dict(src=ok), "on the device"),                              # everything else is fine: a host tensor
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            V.eval_pairs(**kw)


def test_eval_pairs_entry_point_refuses_before_any_launch():
    """The C entry point validates before it launches, so its refusals run without a GPU."""
    import ctypes
    from msml_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(src=p, N=1, H=112, W=112, desc=None, out=p, oh=112, ow=112, gray=0, norm=1, fill=0, protocol=0, seed=1, index0=0)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.msml_eval_pairs(a["src"], a["N"], a["H"], a["W"], a["desc"], a["out"], a["oh"], a["ow"], a["gray"],
                                   a["norm"], a["fill"], a["protocol"], a["seed"], a["index0"], None)
    SHAPE, UNSUPPORTED = -1, -4
    assert rc(src=None) == SHAPE and rc(out=None) == SHAPE and rc(index0=-1) == SHAPE and rc(out=p + 4) == SHAPE
    for kw in (dict(N=0), dict(ow=110), dict(ow=260), dict(oh=2), dict(H=300), dict(W=3), dict(fill=3), dict(fill=-1),
               dict(protocol=2), dict(protocol=1, gray=1)):
        assert rc(**kw) == UNSUPPORTED, kw


def test_sweep_seed_is_a_function_of_seed_level_and_repeat():
    from msml_amd import verification as V
    assert V.sweep_seed(1, 0, 0) == (1 + 0x9E3779B97F4A7C15) % (1 << 63)
    assert V.sweep_seed(1, 2, 3) == (1 + 0x9E3779B97F4A7C15 * (2048 + 4)) % (1 << 63)
    seen = {V.sweep_seed(s, k, r) for s in (1, 2) for k in range(10) for r in range(10)}
    assert len(seen) == 200 and all(0 <= v < (1 << 63) for v in seen)
    assert V.LEVELS == tuple((lo, lo + 1) for lo in range(0, 100, 10))
