"""CPU tests of the MTCNN detector's oracle and host side: the numpy restatement tests/mtcnn_cases.py against the record
of the reference in tests/golden/g13_mtcnn.npz (tools/make_golden_mtcnn.py), its resampling against Pillow itself, the
reference's peculiarities one by one, and the host side of msml_amd/detect.py (weights, packing, scale lists)."""
import os

import numpy as np
import pytest

from msml_amd import detect
from tests import mtcnn_cases as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = ("c24", "c32", "f24", "f32")
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "g13_mtcnn.npz")) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
        _CACHE["w"] = M.load_golden_weights(GOLDEN)
    return _CACHE["g"], _CACHE["w"]


def restated(tag):
    """tests/mtcnn_cases.detect_faces (f64 nets) on the golden input of run `tag`, once per process."""
    if tag not in _CACHE:
        g, w = golden()
        img = g["composite"] if tag[0] == "c" else g["face"]
        mfs = float(g["mfs_small"] if tag.endswith("24") else g["mfs_large"])
        rec, trace = {}, {}
        boxes, marks, dropped = M.detect_faces(img, w, mfs, trace=trace, record=rec)
        _CACHE[tag] = (rec, trace, dropped)
    return _CACHE[tag]


def test_the_record_meets_its_own_conditions():
    g, _ = golden()
    assert g["margin_prob"] >= 1e-3 and g["margin_overlap"] >= 1e-3 and g["margin_round"] >= 1e-2
    assert g["margin_ties"] <= 16
    assert 20 <= g["mfs_small"] <= 32 and g["mfs_large"] == 32
    assert g["composite"].shape == (170, 300, 3) and g["face"].shape == (112, 112, 3)
    for k in ("pnet", "rnet", "onet", "final"):
        assert 0 < g["floor_" + k] < 1e-4


@pytest.mark.parametrize("tag", RUNS)
def test_restatement_equals_the_record(tag):
    g, _ = golden()
    rec, trace, dropped = restated(tag)
    assert dropped == 0
    assert np.array_equal(rec["scales"], g[tag + "_scales"])
    for li in range(len(rec["scales"])):
        assert np.array_equal(rec["level%d" % li], g["%s_level%d" % (tag, li)]), "level %d" % li
    for k in ("crops24", "crops48"):
        assert np.array_equal(rec[k], g["%s_%s" % (tag, k)]), k
    # box lists: the same boxes kept in the same order; integer coordinates exactly, scores and calibrated boxes closely
    for k in ("boxes1", "boxes1r", "boxes2", "boxes2r"):
        want = g["%s_%s" % (tag, k)]
        assert rec[k].shape == want.shape, k
        assert np.array_equal(rec[k][:, :4], want[:, :4]), k
        assert np.abs(rec[k][:, 4:] - want[:, 4:]).max() <= 4 * float(g["floor_final"]), k
    floors = {"pnet": float(g["floor_pnet"]), "rnet": float(g["floor_rnet"]), "onet": float(g["floor_onet"])}
    worst = {k: 0.0 for k in floors}
    for li in range(len(rec["scales"])):
        for k in ("pnet_a%d" % li, "pnet_b%d" % li):
            worst["pnet"] = max(worst["pnet"], float(np.abs(rec[k] - g["%s_%s" % (tag, k)]).max()))
    for k in ("rnet_cls", "rnet_off"):
        worst["rnet"] = max(worst["rnet"], float(np.abs(rec[k] - g["%s_%s" % (tag, k)]).max()))
    for k in ("onet_cls", "onet_off", "onet_lm"):
        worst["onet"] = max(worst["onet"], float(np.abs(rec[k] - g["%s_%s" % (tag, k)]).max()))
    print(tag, "worst", worst, "floors", floors)
    for k in floors:
        assert worst[k] <= 4 * floors[k], k
    for k in ("boxes3", "landmarks"):
        want = g["%s_%s" % (tag, k)]
        assert rec[k].shape == want.shape, k
        assert np.abs(rec[k] - want).max() <= 4 * float(g["floor_final"]), k
    assert np.abs(rec["boxes3"] - g[tag + "_boxes3_f64"]).max() <= 4 * float(g["floor_final"])


@pytest.mark.parametrize("tag", ["c20", "c64"])
def test_pyramid_levels_equal_pillow_bit_for_bit(tag):
    g, _ = golden()
    img = g["composite"]
    mfs = float(tag[1:])
    sc = M.scales(img.shape[0], img.shape[1], mfs)
    assert np.array_equal(np.array(sc), g[tag + "_scales"]) and len(sc) >= 2
    assert sc == detect.pyramid_scales(img.shape[0], img.shape[1], mfs)
    for li, s in enumerate(sc):
        sh, sw = M.level_size(img.shape[0], img.shape[1], s)
        assert np.array_equal(M.resize(img, sw, sh), g["%s_level%d" % (tag, li)]), li
    if tag == "c64":      # the shrink by 5.3 takes 11 taps: more than data.resample_table's 8
        assert max(len(k) for _, k in M.axis_coeffs(300, g["c64_level0"].shape[1])) == 11


@pytest.mark.parametrize("src,dst", [((12, 13), (12, 12)), ((20, 17), (34, 29)), ((64, 85), (13, 16)), ((15, 9), (15, 9))])
def test_resize_equals_pillow(src, dst):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(src[0] * 100 + dst[0])
    a = rng.integers(0, 256, (src[0], src[1], 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), Image.BILINEAR))
    assert np.array_equal(M.resize(a, dst[1], dst[0]), want)


def test_softmax_runs_along_the_width():
    a = np.array([[[[0.0, 1.0, 3.0], [2.0, 2.0, 2.0]], [[1.0, 1.0, 1.0], [0.0, 0.0, np.log(2.0)]]]])
    p = M.width_softmax(a)
    assert np.allclose(p.sum(-1), 1.0)
    assert np.allclose(p[0, 1, 0], [1 / 3, 1 / 3, 1 / 3]) and np.allclose(p[0, 1, 1], [0.25, 0.25, 0.5])
    # not the class softmax: a one-column map is all ones whatever the logits
    assert np.array_equal(M.width_softmax(np.array([[[[5.0]], [[-5.0]]]])), np.ones((1, 2, 1, 1)))


def test_flatten_order_and_the_folded_weight():
    x = np.arange(2 * 3 * 2 * 2, dtype=np.float64).reshape(2, 3, 2, 2)
    f = M.flatten(x)
    assert f[0, :4].tolist() == [0.0, 2.0, 1.0, 3.0]                   # (c, x, y): the column first
    rng = np.random.default_rng(0)
    w = rng.standard_normal((5, 12)).astype(np.float32)
    d = {"features.conv4.weight": w, "features.conv4.bias": np.zeros(5, np.float32),
         "features.prelu4.weight": np.zeros(5, np.float32)}
    wt = detect._fc_block(d, 4, 3, 2)[0].reshape(12, 5)                 # [In][Out] over the (c, y, x) order of the device
    assert np.allclose(x.reshape(2, -1) @ wt, f @ w.T.astype(np.float64))


def test_refine_leaves_the_boxes_clipped():
    boxes = np.array([[-6.0, 4.0, 20.0, 30.0, 0.9], [30.0, 25.0, 55.0, 50.0, 0.8], [5.0, 5.0, 14.0, 14.0, 0.7]])
    off = np.zeros((3, 4))
    b, win, valid = M.refine(boxes, off, 40, 50)
    assert valid.all() and np.all(b[:, 4] == 0)                        # convert_to_square drops the score
    assert b[0].tolist()[:4] == [0.0, 4.0, 20.0, 30.0] and win[0].tolist() == [-6, 4, 27, 27]
    assert b[1].tolist()[:4] == [30.0, 25.0, 49.0, 39.0] and win[1].tolist() == [30, 25, 26, 26]
    assert b[2].tolist()[:4] == [5.0, 5.0, 14.0, 14.0]
    # the next calibration sees the CLIPPED width: 21, not 27
    assert M.calibrate(b[:1], np.array([[0.0, 0.0, 1.0, 0.0]]))[0, 2] == 20.0 + 21.0


def test_nms_tie_goes_to_the_higher_index():
    b = np.array([[0, 0, 9, 9, 0.5], [1, 1, 10, 10, 0.5], [30, 30, 39, 39, 0.5], [0, 0, 9, 9, 0.4]], np.float64)
    assert M.nms(b, 0.5) == [2, 1]
    assert M.nms(b[[1, 0, 2, 3]], 0.5) == [2, 1]
    assert M.nms(b[:2], 0.9) == [1, 0] and M.nms(b[:0]) == []
    small = np.array([[0, 0, 19, 19, 0.9], [5, 5, 9, 9, 0.8]], np.float64)
    assert M.nms(small, 0.7, "union") == [0, 1] and M.nms(small, 0.7, "min") == [0]


def test_box_outside_the_image_is_dropped():
    boxes = np.array([[60.0, 5.0, 80.0, 25.0, 0.9], [-30.0, 5.0, -10.0, 25.0, 0.9], [5.0, 45.0, 20.0, 60.0, 0.9],
                      [10.0, 10.0, 20.0, 20.0, 0.9], [49.0, 39.0, 60.0, 50.0, 0.9]])
    b, win, valid = M.refine(boxes, np.zeros((5, 4)), 40, 50)
    assert valid.tolist() == [False, False, False, True, True]
    img = np.full((40, 50, 3), 200, np.uint8)
    c = M.crops(img, win, valid, 24)
    assert not c[0].any() and not c[1].any() and not c[2].any() and (c[3] == 200).all()
    assert c[4][0, 0, 0] == 200 and c[4][-1, -1, 0] == 0               # one pixel inside, black beyond the corner


def test_weights_load_from_both_forms(tmp_path):
    g, w = golden()
    got = detect.load_weights(GOLDEN)
    for a, b in zip(got, w):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert got[2]["features.conv5.weight"].shape == (256, 1152)
    for name, d in zip(("pnet", "rnet", "onet"), w):
        np.save(os.path.join(tmp_path, name + ".npy"), d, allow_pickle=True)
    again = detect.load_weights(str(tmp_path))
    for a, b in zip(again, w):
        assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in b)
    assert detect.pack_pnet(w[0]).size == 6632
    assert detect.pack_rnet(w[1]).size == 28 * 27 + 56 + 48 * 252 + 96 + 64 * 192 + 128 + 576 * 128 + 256 + 128 * 16 + 16
    with pytest.raises(FileNotFoundError):
        detect.load_weights(os.path.join(str(tmp_path), "nothing"))


def test_first_landmarks():
    lm = [np.zeros((0, 10), np.float32), np.arange(20, dtype=np.float32).reshape(2, 10)]
    pts, found = detect.first_landmarks(lm)
    assert found.tolist() == [False, True] and pts.shape == (2, 5, 2)
    assert pts[1, :, 0].tolist() == [0, 1, 2, 3, 4] and pts[1, :, 1].tolist() == [5, 6, 7, 8, 9]
