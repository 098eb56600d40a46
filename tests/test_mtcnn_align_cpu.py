"""CPU tests of the MTCNN alignment (msml_amd/mtcnn_align.py): the numpy restatement tests/mtcnn_align_cases.py and the
host side of the module against tests/golden/g14_mtcnn_align.npz, which holds what the reference's own code and Pillow
give (tools/make_golden_mtcnn_align.py); the point maps, verification.read_pairs_txt, and the refusals that need no GPU."""
import os

import numpy as np
import pytest

from msml_amd import _lib, mtcnn_align as MA, verification
from tests import mtcnn_align_cases as C
from tests import mtcnn_cases as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}
SIZES = ((112, 112), (96, 112), (256, 256), (128, 96))


def golden():
    if "g" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "g14_mtcnn_align.npz")) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
        with np.load(os.path.join(GOLDEN, "g13_mtcnn.npz")) as z:
            _CACHE["g"].update(composite=z["composite"], face=z["face"])
    return _CACHE["g"]


def ulp_bound(m):
    """4 float32 ulps of the largest entry of the matrix (the bound the fit is held to)."""
    return 4 * float(np.spacing(np.float32(np.abs(m).max())))


def test_template_bit_equal():
    g = golden()
    for w, h in SIZES:
        want = g["template_%d_%d" % (w, h)]
        assert want.dtype == np.float32
        for got in (C.reference_points((w, h)), MA.reference_points((w, h))):
            assert got.dtype == np.float32 and np.array_equal(got, want), (w, h)
    for got in (C.reference_points((112, 112), False), MA.reference_points((112, 112), False)):
        assert np.array_equal(got, g["template_112_112_notsquare"])
    # a non-square crop other than 96 x 112 scales BOTH axes by w / 112
    assert np.array_equal(MA.reference_points((128, 96)),
                          MA.reference_points((112, 112)) * np.float32(128 / 112.))


def test_resize_restatement_equals_pillow():
    g = golden()
    for name, img, ow, oh in C.resize_cases(g["composite"], g["face"]):
        for filt in (C.BILINEAR, C.BICUBIC):
            assert np.array_equal(C.resize(img, ow, oh, filt), g["resize_%s_%d" % (name, filt)]), (name, filt)
    # the checkerboard meets both clips under the bicubic filter: an unclipped accumulator leaves 0..255 there
    name, img, ow, oh = [c for c in C.resize_cases(g["composite"], g["face"]) if c[0] == "checker"][0]
    lo = hi = 0
    a = img.astype(np.int64)
    for xx, (xmin, k) in enumerate(C.axis_coeffs(img.shape[1], ow, C.BICUBIC)):
        acc = (1 << 21) + sum(a[:, xmin + j] * c for j, c in enumerate(k))
        lo, hi = min(lo, int((acc >> 22).min())), max(hi, int((acc >> 22).max()))
    assert lo < 0 and hi > 255


def test_resample_rows_equal_restatement():
    """The tables the kernel reads against the restatement's coefficients, for the lengths of the image cases."""
    for filt in (C.BILINEAR, C.BICUBIC):
        for insz, outsz in ((300, 320), (170, 181), (300, 40), (170, 23), (112, 320), (300, 1), (53, 31), (37, 50),
                            (61, 97), (45, 30), (7, 9), (32767, 3)):
            tab = MA.resample_rows(insz, outsz, filt)
            want = C.axis_coeffs(insz, outsz, filt)
            assert tab.shape[0] == outsz and tab.shape[1] == 2 + max(len(k) for _, k in want)
            for row, (xmin, k) in zip(tab, want):
                assert row[0] == xmin and row[1] == len(k) and list(row[2:2 + len(k)]) == k and not row[2 + len(k):].any()
    ident = MA.resample_rows(5, 5, C.BICUBIC)
    assert np.array_equal(ident, np.stack([np.arange(5), np.ones(5), np.full(5, 1 << 22)], 1))


def test_transpose_restatement_equals_pillow():
    g = golden()
    for name, img in C.orient_cases(g["composite"], g["face"]):
        for method in range(5):
            assert np.array_equal(C.transpose(img, method), g["orient_%s_%d" % (name, method)]), (name, method)


def test_fit_within_four_float32_ulps():
    g = golden()
    ref = g["template_112_112"]
    ok = ~g["fit_degenerate"]
    assert ok.sum() >= 64 and g["fit_mirrored"].sum() >= 1 and g["fit_degenerate"].sum() == 1
    tfm, inv = MA.similarity_matrices(g["fit_points"][ok], ref)
    assert tfm.dtype == np.float64 and tfm.shape == (ok.sum(), 2, 3) == inv.shape
    worst = 0.0
    for n, k in enumerate(np.flatnonzero(ok)):
        t, ti = C.similarity(g["fit_points"][k], ref)
        for got, want in ((t, g["fit_tfm"][k]), (tfm[n], g["fit_tfm"][k]), (ti, g["fit_inv"][k]), (inv[n], g["fit_inv"][k])):
            err = np.abs(got - want).max()
            worst = max(worst, err / ulp_bound(want))
            assert err <= ulp_bound(want), (k, err, ulp_bound(want))
    print("largest error / bound: %.3g" % worst)
    # the mirrored sets took the second branch: a reflection has a negative determinant
    det = tfm[:, 0, 0] * tfm[:, 1, 1] - tfm[:, 0, 1] * tfm[:, 1, 0]
    assert np.array_equal(det < 0, g["fit_mirrored"][ok])
    # reflective=False keeps the plain fit for them
    t_plain, _ = MA.similarity_matrices(g["fit_points"][ok], ref, reflective=False)
    assert (t_plain[:, 0, 0] * t_plain[:, 1, 1] - t_plain[:, 0, 1] * t_plain[:, 1, 0] > 0).all()
    k = int(np.flatnonzero(g["fit_mirrored"][ok])[0])
    assert np.abs(t_plain[k] - C.similarity(g["fit_points"][ok][k], ref, reflective=False)[0]).max() <= ulp_bound(t_plain[k])


def test_fit_refusals():
    g = golden()
    ref = g["template_112_112"]
    pts = g["fit_points"][:3].copy()
    # the reference's rank test is on the template
    with pytest.raises(ValueError, match="twoUniquePointsReq"):
        MA.similarity_matrices(pts, np.full((5, 2), 3.0, np.float32))
    with pytest.raises(ValueError, match="twoUniquePointsReq"):
        C.similarity(pts[0], np.full((5, 2), 3.0, np.float32))
    # coinciding landmarks: the reference returns the inverse of a singular matrix (recorded: entries of 1e9 and more)
    k = int(np.flatnonzero(g["fit_degenerate"])[0])
    assert np.abs(g["fit_tfm"][k]).max() > 1e9
    bad = pts.copy()
    bad[1] = g["fit_points"][k]
    with pytest.raises(ValueError, match="row 1"):
        MA.similarity_matrices(bad, ref)
    bad = pts.copy()
    bad[2, 3, 1] = np.nan
    with pytest.raises(ValueError, match="row 2"):
        MA.similarity_matrices(bad, ref)
    bad[2, 3, 1] = np.inf
    with pytest.raises(ValueError, match="row 2"):
        MA.similarity_matrices(bad, ref)
    with pytest.raises(ValueError):
        MA.similarity_matrices(pts[:, :4], ref)
    with pytest.raises(ValueError):
        MA.similarity_matrices(np.zeros((0, 5, 2), np.float32), ref)


def test_point_and_box_maps():
    g = golden()
    lm, box = g["map_landmarks"], g["map_boxes"]
    for i in range(4):                                          # a 300 x 170 photo: not square
        want = g["map_points_%d" % i]
        assert np.array_equal(C.map_points(lm[0], i, 300, 170), want)
        got = MA.map_points(lm, i, 300, 170)
        assert got.dtype == np.float32 and got.shape == (2, 5, 2) and np.array_equal(got[0], want)
        assert np.array_equal(C.map_boxes(box, i, 300, 170), g["map_boxes_%d" % i])
        assert np.array_equal(MA.map_boxes(box, i, 300, 170), g["map_boxes_%d" % i])
    assert np.array_equal(MA.map_points(lm[0:1] / np.float32(320. / 300), 3, 300, 170)[0], g["map_points_fast_3"])
    # the maps undo the transposes: a marked pixel of the turned copy lands on the pixel it came from
    img = np.zeros((17, 30, 3), np.uint8)
    img[4, 21] = 255
    for i in (1, 2, 3):
        y, x = np.argwhere(C.transpose(img, i + 1)[:, :, 0])[0]
        back = MA.map_points(np.array([[x] * 5 + [y] * 5], np.float32), i, 30, 17)[0, 0]
        assert tuple(back) == (21.0, 4.0), (i, back)
    with pytest.raises(ValueError):
        MA.map_points(lm, 4, 300, 170)


def _cases():
    g = golden()
    return [g["face"], C.transpose(g["face"], C.ROTATE_180), np.zeros((64, 64, 3), np.uint8), g["composite"]]


@pytest.mark.parametrize("fast", (True, False))
def test_align_fully_branches(fast):
    """Which orientation finds the face in the inputs of the GPU test, by the numpy detector, against the reference's own
    detector (recorded): the plain face at ori[0], the face turned by 180 degrees at ori[1] and NOT at ori[0], nothing in
    the black image, the composite at ori[0]."""
    g = golden()
    detect = C.numpy_detector(M.load_golden_weights(GOLDEN))
    tag = "fast" if fast else "slow"
    want = g["fully_%s_orientation" % tag]
    assert list(want) == [0, 1, -1, 0]
    scores = list(g["fully_%s_score" % tag])
    for k, img in enumerate(_cases()):
        if k == 3 and not fast:
            continue                                            # the composite at full size: covered by fast mode
        r = C.align_fully(detect, img, fast_mode=fast)
        assert (r["orientation"] if r else -1) == want[k], k
        if r:
            # the f64 numpy nets against the reference's f32 ones: the detector's recorded floor, times the shrink
            assert np.abs(r["points"] - g["fully_%s_points" % tag][k]).max() < 0.05 * max(img.shape[1] / 320., 1.0)
            assert r["crop"].shape == (112, 112, 3) and r["crop"].any()
            assert abs(r["score"] - scores[[0, 1, None, 2][k]]) < 1e-3


def test_get_landmarks_branches():
    g = golden()
    detect = C.numpy_detector(M.load_golden_weights(GOLDEN))
    faces, boxes = C.get_landmarks(detect, g["face"])
    assert list(g["landmarks_slow_found"]) == [True, True, True] and len(faces) == 3 and boxes.shape == (3, 5)
    for crop, pts in faces:
        assert crop.shape == (256, 256, 3) and pts.shape == (5, 2)
    # (the detector is not made for turned faces: the points of the three orientations need not agree)


def test_read_pairs_txt():
    files = {"bob": ["bob_0002.png", "bob_0001.png"], "al": ["al_0003.png", "al_0001.png", "al_0002.png"],
             "cy": ["cy_0001.png"]}
    order = verification.pairs_file_order(files)
    assert order == [("al", "al_0001.png"), ("al", "al_0002.png"), ("al", "al_0003.png"), ("bob", "bob_0001.png"),
                     ("bob", "bob_0002.png"), ("cy", "cy_0001.png")]
    pairs, issame = verification.read_pairs_txt(["al 1 3\n", "bob 2 al 2\n", "cy 1 cy 1\n", "bob 1 2"], files)
    assert pairs.dtype == np.int64 and pairs.tolist() == [[0, 2], [4, 1], [5, 5], [3, 4]]
    assert issame.dtype == bool and issame.tolist() == [True, False, False, True]
    with pytest.raises(ValueError, match="line 0"):
        verification.read_pairs_txt(["al 1\n"], files)
    with pytest.raises(ValueError, match="line 1"):
        verification.read_pairs_txt(["al 1 2\n", "al 1 4\n"], files)
    with pytest.raises(ValueError, match="line 0"):
        verification.read_pairs_txt(["al 0 1\n"], files)
    with pytest.raises(ValueError, match="line 0"):
        verification.read_pairs_txt(["dan 1 2\n"], files)


def test_new_prototypes_are_exported_and_bound():
    names = _lib.exported_symbols()
    for n in ("msml_img_orient", "msml_img_resize", "msml_img_resize_workspace"):
        assert n in names
    sizes = np.array([[170, 300, 181, 320], [112, 112, 1, 1]], np.int64)
    assert _lib.value("msml_img_resize_workspace", sizes.ctypes.data, 2) == 170 * 960 + 112 * 4
    sizes[1, 3] = 32768
    assert _lib.value("msml_img_resize_workspace", sizes.ctypes.data, 2) == 0
    assert _lib.value("msml_img_resize_workspace", None, 2) == 0


def test_library_refusals_without_a_launch():
    """Every refusal of the two entry points comes before a launch, so it needs no GPU: the pointers are never followed."""
    from msml_amd._lib import call_status
    lib = _lib.load()
    SHAPE, UNSUPPORTED, WORKSPACE = -1, -4, -5
    plan = np.array([[2, 300, 170]], np.int64)
    p8, p4, odd = 4096, 4100, 4101

    def orient(src=p8, nbytes=1000, meta=p8, method=p4, dst=p8, meta_out=p8, pl=None, n=1):
        return call_status("msml_img_orient", src, nbytes, meta, method, dst, meta_out,
                           (plan if pl is None else pl).ctypes.data, n, None)

    assert orient(n=0) == UNSUPPORTED and orient(n=65536) == UNSUPPORTED
    assert orient(src=None) == SHAPE and orient(dst=None) == SHAPE and orient(method=None) == SHAPE
    assert orient(src=odd) == SHAPE and orient(dst=odd) == SHAPE and orient(meta=p4) == SHAPE
    assert orient(meta_out=p4) == SHAPE and orient(method=odd) == SHAPE
    for bad in ([[5, 300, 170]], [[-1, 300, 170]], [[0, 0, 170]], [[0, 300, 32768]]):
        assert orient(pl=np.array(bad, np.int64)) == UNSUPPORTED, bad
    assert orient(pl=np.array([[5, 3, 3]], np.int64)) == UNSUPPORTED and b"method 5" in lib.msml_last_error()

    sizes = np.array([[170, 300, 181, 320]], np.int64)

    def resize(src=p8, meta=p8, dst=p8, meta_out=p8, tables=p4, jobs=p8, sz=None, n=1, filt=3, ws=p8, ws_bytes=1 << 20):
        return call_status("msml_img_resize", src, meta, dst, meta_out, tables, jobs,
                           (sizes if sz is None else sz).ctypes.data, n, filt, ws, ws_bytes, None)

    assert resize(n=0) == UNSUPPORTED
    for filt in (0, 1, 4, 5, -1):
        assert resize(filt=filt) == UNSUPPORTED
    assert resize(src=None) == SHAPE and resize(ws=None) == SHAPE and resize(tables=None) == SHAPE
    assert resize(dst=odd) == SHAPE and resize(ws=odd) == SHAPE and resize(jobs=p4) == SHAPE and resize(meta=p4) == SHAPE
    for bad in ([[0, 300, 181, 320]], [[170, 32768, 181, 320]], [[170, 300, 0, 320]], [[170, 300, 181, 40000]]):
        assert resize(sz=np.array(bad, np.int64)) == UNSUPPORTED, bad
    assert resize(ws_bytes=170 * 960 - 1) == WORKSPACE


def test_host_wrapper_refusals():
    """What the wrappers refuse before they touch the device: meta against the buffer length, methods, sizes, filters."""
    import torch
    buf = torch.zeros(5 * 24, dtype=torch.uint8)
    meta = np.array([[0, 5, 7, 24]], np.int64)
    for bad in ([[0, 6, 7, 24]], [[4, 5, 7, 24]], [[0, 5, 9, 24]], [[2, 4, 7, 24]], [[0, 5, 7, 20]], [[0, 0, 7, 24]],
                [[0, 5, 32768, 24]]):
        with pytest.raises(ValueError, match="meta row 0"):
            MA._packed((buf, np.array(bad, np.int64)))
    assert MA._packed((buf, meta))[1].tolist() == meta.tolist()
    with pytest.raises(ValueError, match="method"):
        MA.img_orient((buf, meta), [5])
    with pytest.raises(ValueError, match="methods"):
        MA.img_orient((buf, meta), [1, 2])
    with pytest.raises(ValueError, match="filter"):
        MA.img_resize((buf, meta), (4, 4), filter=1)
    with pytest.raises(ValueError, match="1..32767"):
        MA.img_resize((buf, meta), (0, 4))
    with pytest.raises(ValueError, match="sizes for"):
        MA.img_resize((buf, meta), [(4, 4), (5, 5)])
    for bad in ((112, 300), (110, 112), (2, 2)):
        with pytest.raises(ValueError, match="crop_size"):
            MA._crop_hw(bad)
    assert MA._crop_hw((96, 112)) == (112, 96)
