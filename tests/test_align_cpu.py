"""CPU tests of the host side of the face alignment (msml_amd/ijb.py: align_matrices, pack_images, the meta check of
align_faces) and a self-check of the oracle's fixed-point warp (tests/align_cases.py) against exact bilinear
interpolation.  Neither OpenCV nor skimage is needed; parity with them is not what these tests show."""
import numpy as np
import pytest
import torch

from tests import align_cases as A


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_align_matrices_equal_the_closed_form_fit():
    """48 random float32 landmark sets: Umeyama with scale (SVD) and the closed-form similarity fit are the same
    least-squares solution; bound 1e-12 relative (a prototype measured 2e-15).  Also: the 68-point reduction, the batch
    against a loop over single sets, the independent restatement of skimage's routine, and the refusals."""
    from msml_amd import ijb
    rng = np.random.default_rng(3)
    lm, exact = A.random_landmarks(rng, 48)
    assert lm.dtype == np.float32
    m = ijb.align_matrices(lm)
    assert m.shape == (48, 2, 3) and m.dtype == np.float64
    worst = 0.0
    for i in range(48):
        worst = max(worst, _rel(m[i], A.closed_form(lm[i], A.DST112)))
        assert _rel(m[i], A.umeyama(lm[i], A.DST112)[:2]) <= 1e-12
        assert np.array_equal(ijb.align_matrices(lm[i])[0], m[i])               # batch == loop, bit for bit
        mapped = lm[i].astype(np.float64) @ m[i][:, :2].T + m[i][:, 2]
        assert np.abs(mapped - A.DST112).max() < 8.0      # it lands the landmarks: the noise is 1.5 px sigma there
    print("umeyama vs closed form: max relative difference %.3e (bound 1e-12)" % worst)
    assert worst <= 1e-12
    # 68 points: only 36, 39, 42, 45, 30, 48, 54 count
    lm68 = rng.uniform(0, 250, (6, 68, 2)).astype(np.float32)
    five = np.stack([A.reduce68(v) for v in lm68])
    assert five.dtype == np.float32
    assert np.array_equal(ijb.align_matrices(lm68), ijb.align_matrices(five))
    other = lm68.copy()
    keep = [36, 39, 42, 45, 30, 48, 54]
    mask = np.ones(68, bool)
    mask[keep] = False
    other[:, mask] += 17.0
    assert np.array_equal(ijb.align_matrices(other), ijb.align_matrices(lm68))
    # refusals name the row
    bad = lm.copy()
    bad[7, 2, 1] = np.nan
    with pytest.raises(ValueError, match="row 7"):
        ijb.align_matrices(bad)
    bad = lm.copy()
    bad[11] = bad[11, 0]
    with pytest.raises(ValueError, match="row 11"):
        ijb.align_matrices(bad)
    with pytest.raises(ValueError):
        ijb.align_matrices(np.zeros((3, 4, 2)))


def test_align_matrices_rank_one_and_reflection():
    """Collinear landmarks (rank 1) and a mirrored set (det < 0) take skimage's branches: equal to the restatement."""
    from msml_amd import ijb
    line = np.stack([np.linspace(10, 90, 5), np.linspace(20, 60, 5)], 1)
    mirrored = A.DST112.astype(np.float64) * np.array([-1.0, 1.0]) + np.array([200.0, 3.0])
    sets = np.stack([line, mirrored, line[::-1]])
    m = ijb.align_matrices(sets)
    for i in range(3):
        want = A.umeyama(sets[i], A.DST112)[:2]
        assert np.abs(m[i] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.linalg.det(m[1][:, :2]) > 0                # Umeyama never returns a reflection


def test_pack_images_layout_and_refusals():
    from msml_amd import ijb
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((37, 53), (1, 1), (9, 300))]
    imgs.append(big[::2, 3:14])                          # a strided view, as a crop of a decoded image is
    buf, meta = ijb.pack_images(imgs)
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and meta.dtype == np.int64 and meta.shape == (4, 4)
    flat = buf.numpy()
    end = 0
    for i, im in enumerate(imgs):
        off, h, w, pitch = (int(v) for v in meta[i])
        assert off % 4 == 0 and off >= end and (h, w) == im.shape[:2] and pitch == 3 * w
        assert np.array_equal(flat[off:off + h * pitch].reshape(h, w, 3), im)
        end = off + h * pitch
    assert buf.numel() >= end and buf.numel() % 4 == 0
    ok = imgs[0]
    for bad in ([], [ok.astype(np.float32)], [ok[:, :, :2]], [ok[:, :, 0]], [np.zeros((0, 5, 3), np.uint8)],
                [np.zeros((1, 32768, 3), np.uint8)], [ok, ok.tolist()]):
        with pytest.raises(ValueError):
            ijb.pack_images(bad)
    ijb.pack_images([np.zeros((1, 32767, 3), np.uint8)])


def test_invert_matrices_follows_the_stated_order():
    from msml_amd import ijb
    rng = np.random.default_rng(6)
    _, mats = A.random_landmarks(rng, 16)
    mats = np.concatenate([mats, np.array([[[2.0, 4.0, 1.0], [1.0, 2.0, 5.0]]])])      # D == 0
    got = ijb.invert_matrices(mats)
    for i in range(len(mats)):
        assert np.array_equal(got[i], A.invert(mats[i]))
    assert np.array_equal(got[-1][[0, 1, 3, 4]], np.zeros(4))
    with pytest.raises(ValueError):
        ijb.invert_matrices(np.full((1, 2, 3), np.inf))


def test_align_faces_checks_meta_before_the_launch(monkeypatch):
    """Every meta row must describe an image inside the buffer; nothing is uploaded or launched otherwise."""
    from msml_amd import ijb
    calls = []
    monkeypatch.setattr(ijb, "call", lambda *a: calls.append(a))
    buf = torch.zeros(4000, dtype=torch.uint8)
    eye = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    good = [0, 30, 40, 120]
    for row in ([-4, 30, 40, 120], [2, 30, 40, 120], [0, 30, 40, 119], [0, 0, 40, 120], [0, 30, 0, 120],
                [0, 30, 32768, 3 * 32768], [0, 34, 40, 120], [404, 30, 40, 120], [0, 30, 40, 134],
                [4000, 1, 1, 3], [0, 30, 40, 2 ** 31]):
        with pytest.raises(ValueError, match="meta row 1"):
            ijb.align_faces(buf, np.array([good, row]), np.repeat(eye, 2, 0))
    with pytest.raises(ValueError):
        ijb.align_faces(buf, np.array([good]), np.repeat(eye, 2, 0))            # two matrices, one image
    with pytest.raises(ValueError):
        ijb.align_faces(buf, np.array([good], np.float64), eye)
    with pytest.raises(ValueError):
        ijb.align_faces(buf.float(), np.array([good]), eye)
    assert calls == []


def test_oracle_fixed_point_warp_is_within_one_level_of_exact_bilinear():
    """tests/align_cases.warp (5 fraction bits, weights summing to 32768, rounded result) against exact f64 bilinear
    interpolation of the same uint8 samples, on the smooth image 127.5 + 60 sin(x (0.05 + 0.01 c) + c) + 60 cos(y (0.04 +
    0.01 c) - c): where the exact source position lies in [1, W - 3] x [1, H - 3] the two differ by at most 1 grey
    level (0.5 from the final rounding + the 1/64-pixel position error times the gradient; a prototype measured 0.62).
    At least 25 % of all pixels must be interior, so that the bound is not vacuous."""
    rng = np.random.default_rng(9)
    worst, interior, total = 0.0, 0, 0
    for h, w in A.SIZES:
        img = A.smooth_image(h, w)
        lm, _ = A.random_landmarks(rng, 8, (h, w))
        for i in range(8):
            minv = A.invert(A.umeyama(lm[i], A.DST112)[:2])
            got = A.warp(img, minv, 112, 112, swap_rb=False).astype(np.float64)
            want = A.warp_exact(img, minv, 112, 112)
            xs, ys = A.source_positions(minv, 112, 112)
            inner = (xs >= 1) & (xs <= w - 3) & (ys >= 1) & (ys <= h - 3)
            interior += int(inner.sum())
            total += inner.size
            if inner.any():
                worst = max(worst, float(np.abs(got - want)[inner].max()))
    share = interior / total
    print("fixed-point vs exact bilinear: max |diff| %.3f grey levels over %d interior pixels (%.1f %% of all)"
          % (worst, interior, 100 * share))
    assert share >= 0.25
    assert worst <= 1.0


def test_oracle_pairs_layout():
    """Row 2i is the normalised face in CHW, row 2i + 1 its mirror; the block is black = -1."""
    rng = np.random.default_rng(2)
    faces = rng.integers(0, 256, (2, 8, 12, 3), dtype=np.uint8)
    desc = np.zeros((2, 64), np.int32)
    desc[1, :5] = (3, 4, 2, 5, 3)
    out = A.pairs(faces, desc)
    assert out.shape == (4, 3, 8, 12) and out.dtype == np.float32
    assert out[0, 1, 3, 7] == np.float32((np.float32(faces[0, 3, 7, 1]) / np.float32(255) - np.float32(0.5)) / np.float32(0.5))
    assert np.array_equal(out[1], out[0][..., ::-1]) and np.array_equal(out[3], out[2][..., ::-1])
    assert (out[2][:, 2:5, 4:9] == -1).all()
    clean = A.pairs(faces)
    outside = np.ones((8, 12), bool)
    outside[2:5, 4:9] = False
    assert np.array_equal(out[2][:, outside], clean[2][:, outside]) and np.array_equal(out[0], clean[0])
