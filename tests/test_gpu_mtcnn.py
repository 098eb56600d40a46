"""GPU tests of the MTCNN detector (msml_amd/detect.py, csrc/detect.hip) against the numpy restatement
tests/mtcnn_cases.py: resampling and crops bit for bit, the three nets within 4 x the recorded f32-vs-f64 floor of the
reference (tests/golden/g13_mtcnn.npz), NMS keep lists equal, and detect_faces end to end on the recorded inputs.
Inputs of the net tests are cuts of the recorded composite, so that the activations have the size the floors were
measured at."""
import os

import numpy as np
import pytest
import torch

from msml_amd import detect
from tests import mtcnn_cases as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def fixtures():
    """(golden arrays, weights, Detector), once per process."""
    if "s" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "g13_mtcnn.npz")) as z:
            g = {k: z[k] for k in z.files}
        w = M.load_golden_weights(GOLDEN)
        _CACHE["s"] = (g, w, detect.Detector(detect.load_weights(GOLDEN)))
    return _CACHE["s"]


def restated(name, img, mfs):
    key = (name, mfs)
    if key not in _CACHE:
        _CACHE[key] = M.detect_faces(img, fixtures()[1], mfs)
    return _CACHE[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def resample(det, images, jobs):
    """jobs: (image, x0, y0, w, h, out_w, out_h) -> list of uint8 [out_h][out_w][3] read back from the f32 output."""
    from msml_amd import ijb
    buf, meta = ijb.pack_images(images)
    table, off = [], 0
    for j in jobs:
        table.append(tuple(j) + (off,))
        off += 3 * j[5] * j[6]
    out = torch.full((off,), 7.0, dtype=torch.float32, device="cuda")
    det.resample(buf.cuda(), dev(meta), dev(np.array(table, np.int64)), out, max(j[5] * j[6] for j in jobs))
    out = out.cpu().numpy()
    res = []
    for j in table:
        f = out[j[7]:j[7] + 3 * j[5] * j[6]].reshape(3, j[6], j[5]).transpose(1, 2, 0)
        u = f / np.float32(0.0078125) + np.float32(127.5)
        assert np.array_equal(u, np.round(u)) and u.min() >= 0 and u.max() <= 255
        res.append(u.astype(np.uint8))
    return res


def test_resample_and_crops_bit_exact():
    g, _, det = fixtures()
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((12, 12), (13, 14), (40, 29), (64, 85))]
    jobs = []
    for i, im in enumerate(images):                       # whole images: identity, down, up (one axis kept at times)
        h, w = im.shape[:2]
        for oh, ow in ((h, w), (12, 12), (h, 12), (2 * h + 1, 2 * w - 3), (max(1, h // 4), max(1, w // 4))):
            jobs.append((i, 0, 0, w, h, ow, oh))
    jobs.append((3, 0, 0, 85, 64, 16, 12))                # / 5.3, a first pyramid level: 11 taps
    for size in (24, 48):
        jobs += [(2, 5, 6, 17, 17, size, size),           # inside
                 (2, -7, 4, 20, 20, size, size), (2, 15, 3, 22, 22, size, size),         # over the left / right side
                 (2, 3, -9, 19, 19, size, size), (2, 3, 30, 19, 19, size, size),         # over the top / bottom
                 (2, -5, -8, 30, 30, size, size), (2, 20, 31, 25, 25, size, size),       # two sides at once
                 (2, -40, -30, 160, 160, size, size),                                     # all four, 13+ taps
                 (2, 9, 9, 1, 7, size, size), (2, 9, 9, 7, 1, size, size), (2, 28, 39, 1, 1, size, size),   # 1 px wide
                 (1, 0, 0, 0, 0, size, size)]                                             # a dropped box: black
    taps = set()
    for j in jobs:
        if j[3] > 0:
            taps |= {len(k) for _, k in M.axis_coeffs(j[3], j[5])}
    assert {1, 2, 9} <= taps and max(taps) >= 12
    got = resample(det, images, jobs)
    bad = 0
    for j, r in zip(jobs, got):
        want = (np.zeros((j[6], j[5], 3), np.uint8) if j[3] == 0 else
                M.resize(M.window(images[j[0]], j[1], j[2], j[3], j[4]), j[5], j[6]))
        d = int((r != want).sum())
        if d:
            print("job", j, "differs in", d, "bytes")
        bad += d
    assert bad == 0


def test_pyramid_equals_the_recorded_levels():
    g, _, det = fixtures()
    img = g["composite"]
    jobs = []
    for tag in ("c20", "c64"):
        for li in range(len(g[tag + "_scales"])):
            lv = g["%s_level%d" % (tag, li)]
            jobs.append((0, 0, 0, img.shape[1], img.shape[0], lv.shape[1], lv.shape[0]))
    got = resample(det, [img], jobs)
    k = 0
    for tag in ("c20", "c64"):
        for li in range(len(g[tag + "_scales"])):
            assert np.array_equal(got[k], g["%s_level%d" % (tag, li)]), (tag, li)
            k += 1


def test_pnet_at_edge_sizes():
    g, w, det = fixtures()
    img = g["composite"]
    t = det.tile
    # one cell; odd / even pool edges; ending exactly on a tile edge and one cell past it, per axis; several tiles
    sizes = [(12, 12), (13, 14), (14, 13), (2 * t + 9, 2 * t + 11), (2 * t + 11, 2 * t + 10), (45, 62)]
    assert detect.pnet_out(2 * t + 9) == t and detect.pnet_out(2 * t + 10) == t and detect.pnet_out(2 * t + 11) == t + 1
    cuts, levels, in_off, out_off = [], [], 0, 0
    for i, (h, wd) in enumerate(sizes):
        y0, x0 = 20 + 3 * i, 10 + 17 * i
        cuts.append(M.normalise(img[y0:y0 + h, x0:x0 + wd], np.float32))
        oh, ow = detect.pnet_out(h), detect.pnet_out(wd)
        levels.append((in_off, h, wd, out_off, oh, ow))
        in_off += 3 * h * wd
        out_off += 6 * oh * ow
    levels = np.array(levels, np.int64)
    maps = det.run_pnet(dev(np.concatenate([c.ravel() for c in cuts])), levels).cpu().numpy()
    assert maps.size == out_off
    tol = 4 * float(g["floor_pnet"])
    worst = 0.0
    for c, lv in zip(cuts, levels):
        a, b = M.pnet_logits(c[None].astype(np.float64), w[0])
        want = np.concatenate([a[0], b[0]], 0)
        assert want.shape == (6, lv[4], lv[5])
        got = maps[lv[3]:lv[3] + want.size].reshape(want.shape)
        err = float(np.abs(got - want).max())
        print("pnet %dx%d -> %dx%d: max err %.3e (bound %.3e)" % (lv[1], lv[2], lv[4], lv[5], err, tol))
        worst = max(worst, err)
    assert worst <= tol


def _cuts(img, n, size):
    rng = np.random.default_rng(n + size)
    out = np.empty((n, size, size, 3), np.uint8)
    for i in range(n):
        s = int(rng.integers(20, 90))
        x0, y0 = int(rng.integers(-10, 300 - s + 10)), int(rng.integers(-10, 170 - s + 10))
        out[i] = M.resize(M.window(img, x0, y0, s, s), size, size)
    return out


@pytest.mark.parametrize("net", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_rnet_onet(net, n):
    g, w, det = fixtures()
    size = 24 if net == 0 else 48
    u8 = _cuts(g["composite"], n, size)
    got = det.run_net(net, dev(M.normalise_batch(u8, np.float32)), n).cpu().numpy()
    want = np.concatenate((M.rnet_raw if net == 0 else M.onet_raw)(M.normalise_batch(u8, np.float64), w[1 + net]), 1)
    tol = 4 * float(g["floor_rnet" if net == 0 else "floor_onet"])
    err = float(np.abs(got[:, :want.shape[1]] - want).max())
    print("net %d n %d: max err %.3e (bound %.3e)" % (net, n, err, tol))
    assert err <= tol
    assert not got[:, want.shape[1]:].any()


def _boxes(rng, n, ties=False):
    b = np.zeros((n, detect.COLS))
    x, y = rng.integers(0, 60, n), rng.integers(0, 60, n)
    s = rng.integers(8, 40, n)
    b[:, 0], b[:, 1], b[:, 2], b[:, 3] = x, y, x + s, y + s
    b[:, 4] = rng.permutation(n) / max(n, 1) * 0.5 + 0.4
    if ties and n >= 2:
        b[rng.integers(0, n, n // 2), 4] = 0.75
        b[1, :4] = b[0, :4] + 1
        b[0, 4] = b[1, 4] = 0.99                   # two overlapping boxes with the best score: index 1 must win
    return b


@pytest.mark.parametrize("mode", ["union", "min"])
def test_nms_keep_lists(mode):
    g, w, det = fixtures()
    rng = np.random.default_rng(11)
    lengths = [0, 1, 2, 64, 65, 0, 300, 16]
    segs = [_boxes(rng, n, ties=(i % 2 == 1 or n == 16)) for i, n in enumerate(lengths)]
    rows = np.concatenate(segs)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    valid = np.ones(len(rows), np.uint8)
    valid[off[6] + 5:off[6] + 300:7] = 0
    for use_valid in (False, True):
        keep, cnt = det.nms(dev(rows), dev(off), dev(valid) if use_valid else None, len(lengths), max(lengths), 0.5, mode)
        keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
        for s, n in enumerate(lengths):
            b = segs[s][:, :5]
            idx = np.flatnonzero(valid[off[s]:off[s + 1]]) if use_valid else np.arange(n)
            want = [int(idx[k]) for k in M.nms(b[idx], 0.5, mode)]
            got = keep[off[s]:off[s] + cnt[s]] - off[s]
            assert got.tolist() == want, (s, n, use_valid)
            assert (keep[off[s] + cnt[s]:off[s + 1]] == -1).all()
    assert segs[3][0, 4] == segs[3][1, 4] == 0.99


def test_refine_clips_drops_and_crops():
    """k_det_refine directly: boxes inside, over one and two sides, pushed wholly outside by their offsets (each side),
    with one pixel inside, of no width, with an absurd coordinate, with a side of 39 611 (refused) and of 605 pixels (a
    crop of 26 and 51 taps per axis, nearly all outside the image); two image sizes in one call."""
    from msml_amd import ijb
    g, _, det = fixtures()
    rng = np.random.default_rng(3)
    images = [g["composite"], rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)]
    cases = [  # image, box, offsets
        (1, (10, 10, 20, 20), (0, 0, 0, 0)), (1, (10, 10, 20, 20), (0.13, -0.21, 0.08, 0.17)),
        (1, (-6, 4, 20, 30), (0, 0, 0, 0)), (1, (30, 25, 55, 50), (0, 0, 0, 0)), (1, (-8, -9, 12, 14), (-0.1, 0, 0, 0.2)),
        (1, (10, 10, 20, 20), (5, 0, 5, 0)), (1, (10, 10, 20, 20), (-5, 0, -5, 0)), (1, (10, 10, 20, 20), (0, 4, 0, 4)),
        (1, (10, 10, 20, 20), (0, -4, 0, -4)), (1, (49, 39, 60, 50), (0, 0, 0, 0)), (1, (50, 39, 61, 50), (0, 0, 0, 0)),
        (1, (10, 10, 20, 20), (0.6, 0.6, -0.6, -0.6)), (1, (10, 10, 20, 20), (-1e12, 0, 1e12, 0)),
        (0, (250, 120, 320, 190), (0.02, -0.03, 0.01, 0.04)), (0, (100, 50, 140, 99), (-0.07, 0.1, 0.05, -0.02)),
        (1, (10, 10, 20, 20), (-1800, -1800, 1800, 1800)), (1, (10, 10, 20, 20), (-27, -27, 27, 27))]
    rows = np.zeros((len(cases), detect.COLS))
    for i, (im, box, off) in enumerate(cases):
        rows[i, :4], rows[i, 4], rows[i, 5], rows[i, 6:10] = box, 0.9, im, off
    buf, meta = ijb.pack_images(images)
    for size in (24, 48):
        dev_rows = dev(rows)
        crops, valid = det.crops(buf.cuda(), dev(meta), dev_rows, len(cases), size)
        got, valid, crops = dev_rows.cpu().numpy(), valid.cpu().numpy().astype(bool), crops.cpu().numpy()
        for im in (0, 1):
            sel = np.flatnonzero(rows[:, 5] == im)
            h, w = images[im].shape[:2]
            with np.errstate(all="ignore"):
                b, win, ok = M.refine(rows[sel, :5], rows[sel, 6:10], h, w)
            assert valid[sel].tolist() == ok.tolist(), (size, im)
            fin = np.abs(b[:, :4]).max(1) < 1e9
            assert np.array_equal(got[sel][fin, :5], b[fin]), (size, im)
            want = M.normalise_batch(M.crops(images[im], win, ok, size))
            assert np.array_equal(crops[sel], want), (size, im)
        assert valid.tolist() == [True] * 5 + [False] * 4 + [True, False, False, False, True, True, False, True]


def _check(det_boxes, det_marks, want, tol):
    boxes, marks, _ = want
    assert det_boxes.shape == boxes.shape and det_marks.shape == marks.shape and det_boxes.dtype == np.float64
    assert det_marks.dtype == np.float32
    if len(boxes):
        eb, el = float(np.abs(det_boxes - boxes).max()), float(np.abs(det_marks - marks).max())
        print("boxes max err %.3e, landmarks max err %.3e (bound %.3e)" % (eb, el, tol))
        assert eb <= tol and el <= tol


@pytest.mark.parametrize("which", ["small", "large"])
def test_detect_faces_end_to_end(which, monkeypatch):
    g, w, det = fixtures()
    mfs = float(g["mfs_" + which])
    gray = np.full((40, 40, 3), 128, np.uint8)
    imgs = [g["composite"], g["face"], gray]
    res = det.detect_faces(imgs, min_face_size=mfs)
    tol = 4 * float(g["floor_final"])
    assert res.dropped == 0
    _check(res.boxes[0], res.landmarks[0], restated("composite", imgs[0], mfs), tol)
    _check(res.boxes[1], res.landmarks[1], restated("face", imgs[1], mfs), tol)
    assert len(res.boxes[0]) == 3 and len(res.boxes[1]) == 1
    assert res.boxes[2].shape == (0, 5) and res.landmarks[2].shape == (0, 10)
    # the record of the reference itself
    tag = "24" if which == "small" else "32"
    assert np.abs(res.boxes[0] - g["c%s_boxes3" % tag]).max() <= 2 * tol
    assert np.abs(res.landmarks[1] - g["f%s_landmarks" % tag]).max() <= 2 * tol
    # a batch equals its images run singly, bit for bit
    for i, im in enumerate(imgs):
        one = det.detect_faces([im], min_face_size=mfs)
        assert np.array_equal(one.boxes[0], res.boxes[i]) and np.array_equal(one.landmarks[0], res.landmarks[i]), i
    pts, found = detect.first_landmarks(res.landmarks)
    assert found.tolist() == [True, True, False] and pts[0, 0, 0] == res.landmarks[0][0, 0]
    # a caller's (buf, meta) with a row past the buffer is refused on the host, before anything is uploaded or launched
    from msml_amd import ijb

    def no_call(*a, **k):
        raise AssertionError("a launch for a meta row that is not an image inside the buffer")

    buf, meta = ijb.pack_images([g["face"]])
    assert len(det.detect_faces((buf.cuda(), meta), min_face_size=mfs).boxes[0]) == 1
    meta[0, 1] += 1
    monkeypatch.setattr(detect, "call", no_call)
    with pytest.raises(ValueError, match="detect_faces: meta row 0"):
        det.detect_faces((buf.cuda(), meta), min_face_size=mfs)


def test_candidate_capacity_overflow_is_an_error():
    from msml_amd import _lib
    g, w, det = fixtures()
    with pytest.raises(detect.CapacityError) as e:
        det.detect_faces([g["composite"]], min_face_size=float(g["mfs_small"]), max_candidates=2)
    assert e.value.code == detect.ERR_CAPACITY == -6 and "capacity" in str(e.value)
    rows, off = dev(np.zeros((4, detect.COLS))), dev(np.array([0, 4], np.int64))
    scratch = torch.zeros(4, dtype=torch.int32, device="cuda")
    cap = det.nms_capacity
    assert _lib.call_status("msml_det_nms", rows, off, None, 1, cap + 1, cap, 0.5, 0, scratch, scratch, scratch) == -6
    assert _lib.call_status("msml_det_nms", rows, off, None, 1, 4, cap + 1, 0.5, 0, scratch, scratch, scratch) == -1
    # enough room: the same call goes through
    assert len(det.detect_faces([g["composite"]], min_face_size=float(g["mfs_small"]), max_candidates=cap).boxes[0]) == 3


@pytest.mark.parametrize("stage", [2, 3])
def test_no_survivor_gives_empty_results(stage):
    """P-Net fires, then R-Net (stage 2) or O-Net (stage 3) rejects every box of the call -- a threshold of 1.0 stands for
    a photo without a face: empty arrays and a dropped count of 0, alone and beside the gray image."""
    g, w, det = fixtures()
    thr = (0.6, 1.0, 0.8) if stage == 2 else (0.6, 0.7, 1.0)
    for imgs in ([g["composite"]], [np.full((40, 40, 3), 128, np.uint8), g["composite"], g["face"]]):
        res = det.detect_faces(imgs, min_face_size=float(g["mfs_small"]), thresholds=thr)
        assert res.dropped == 0 and len(res.boxes) == len(res.landmarks) == len(imgs)
        for b, m in zip(res.boxes, res.landmarks):
            assert b.shape == (0, 5) and b.dtype == np.float64 and m.shape == (0, 10) and m.dtype == np.float32
    assert not detect.first_landmarks(res.landmarks)[1].any()


def test_capacity_is_per_image_not_per_batch():
    """A batch whose images TOGETHER keep more boxes after stage 1 than the capacity, while no image holds more candidates
    than it: the same result as one image alone, and one candidate less of room is the error."""
    g, w, det = fixtures()
    img, mfs = g["composite"], float(g["mfs_small"])
    most = 0                                               # P-Net candidates of the image, by the restatement
    for s in M.scales(img.shape[0], img.shape[1], mfs):
        sh, sw = M.level_size(img.shape[0], img.shape[1], s)
        a, b = M.pnet_logits(M.normalise(M.resize(img, sw, sh), np.float64)[None], w[0])
        most += len(M.generate_boxes(M.width_softmax(a)[0, 1], b[0], s, 0.6))
    kept = len(g["c24_boxes1"])
    copies = most // kept + 1
    print("candidates %d, %d kept after stage 1, %d copies" % (most, kept, copies))
    assert copies * kept > most and copies <= 512
    one = det.detect_faces([img], min_face_size=mfs)
    res = det.detect_faces([img] * copies, min_face_size=mfs, max_candidates=most)
    for i in range(copies):
        assert np.array_equal(res.boxes[i], one.boxes[0]) and np.array_equal(res.landmarks[i], one.landmarks[0])
    with pytest.raises(detect.CapacityError):
        det.detect_faces([img] * 2, min_face_size=mfs, max_candidates=most - 1)


def test_detect_and_embed_equals_align_and_embed():
    from msml_amd import ijb
    from msml_amd.backbones import MSML
    from oracle.fill import fill_module
    g, w, det = fixtures()
    peer = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
    torch.manual_seed(0)
    model = fill_module(MSML("iresnet18", "unet", (1, 1, 1, 1), 8, fp16=False, fm_params=(3, 2, "sigmoid", "mul"),
                             header_type="AMArcFace", peer_params=peer)).cuda().eval()
    mfs = float(g["mfs_large"])
    bgr = [np.ascontiguousarray(im[:, :, ::-1]) for im in (g["composite"], np.full((40, 40, 3), 128, np.uint8), g["face"])]
    feats, found, res = detect.detect_and_embed(model, bgr, det, min_face_size=mfs, batch=4, lo=40, hi=41, seed=3)
    assert found.tolist() == [True, False, True] and feats.shape[0] == 2 and feats.is_cuda
    pts, _ = detect.first_landmarks(res.landmarks)
    want = ijb.align_and_embed(model, [bgr[0], bgr[2]], pts[[0, 2]], batch=4, lo=40, hi=41, seed=3)
    assert torch.equal(feats, want) and bool(torch.isfinite(feats).all())
