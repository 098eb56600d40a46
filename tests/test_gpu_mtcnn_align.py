"""GPU tests of the MTCNN alignment (msml_amd/mtcnn_align.py, csrc/imgops.hip): the two image kernels bit for bit
against Pillow's recorded bytes (tests/golden/g14_mtcnn_align.npz) and the numpy restatement tests/mtcnn_align_cases.py,
and the four methods against the restatement fed THE DEVICE'S OWN detections, which isolates the new code from the
detector's f32 floor (tests/test_gpu_mtcnn.py bounds that).  The shapes are the smallest at which each kernel can go
wrong, not photo sizes."""
import os

import numpy as np
import pytest
import torch

from msml_amd import _lib, detect, ijb, mtcnn_align as MA, packed
from tests import align_cases as A
from tests import mtcnn_align_cases as C
from tests import packed_cases as P

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}
GUARD = 256


def fixtures():
    """(golden arrays, Detector), once per process."""
    if "s" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "g14_mtcnn_align.npz")) as z:
            g = {k: z[k] for k in z.files}
        with np.load(os.path.join(GOLDEN, "g13_mtcnn.npz")) as z:
            g.update(composite=z["composite"], face=z["face"])
        _CACHE["s"] = (g, detect.Detector(detect.load_weights(GOLDEN)))
    return _CACHE["s"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_detect(img, min_face_size, thresholds):
    """The device's detections of ONE image, for the restatement."""
    d = fixtures()[1].detect_faces([np.ascontiguousarray(img)], float(min_face_size), tuple(thresholds))
    return d.boxes[0], d.landmarks[0]


def ulp_bound(m):
    return 4 * float(np.spacing(np.float32(np.abs(m).max())))


def guarded(total):
    return P.guarded(total, guard=GUARD)


def bands_untouched(whole):
    return P.bands_untouched(whole, guard=GUARD)


def unpack_checked(buf, meta):
    """The images of a packed output with rows of whole dwords; the bytes between 3 W and the pitch must be 0."""
    for o, h, w, p in meta:
        assert p % 4 == 0 and o % 4 == 0 and 0 <= p - 3 * w < 4
    return P.unpack(buf, meta)


def test_orient_every_method_bit_exact_with_guard_bands():
    g, _ = fixtures()
    cases = C.orient_cases(g["composite"], g["face"])
    images = [im for _, im in cases]
    assert [im.shape[:2] for im in images] == [(5, 7), (112, 112), (170, 300)]
    flat, meta = A.pack(images, pitch_extra=3)                  # pitches 24, 339, 903: rows start at any alignment
    assert meta[0, 3] == 24
    src = dev(flat)
    for shift in range(5):                                      # every (image, method) pair; methods differ inside a launch
        methods = np.array([(shift + k) % 5 for k in range(3)], np.int64)
        turn = (methods == 2) | (methods == 4)
        meta_out, total = packed.layout(np.where(turn, meta[:, 2], meta[:, 1]), np.where(turn, meta[:, 1], meta[:, 2]))
        plan = np.ascontiguousarray(np.stack([methods, meta_out[:, 1], meta_out[:, 2]], 1))
        whole, out = guarded(total)
        _lib.call("msml_img_orient", src, src.numel(), dev(meta), dev(methods.astype(np.int32)), out, dev(meta_out),
                  plan.ctypes.data, 3)
        torch.cuda.synchronize()
        assert bands_untouched(whole)
        for (name, im), m, got in zip(cases, methods, unpack_checked(out, meta_out)):
            assert np.array_equal(got, g["orient_%s_%d" % (name, m)]), (name, m)
            assert np.array_equal(got, C.transpose(im, m))
    # the wrapper, on a list of arrays, gives the same images
    buf, mo = MA.img_orient(images, [2, 4, 3])
    for (name, _), m, got in zip(cases, (2, 4, 3), MA.unpack(buf, mo)):
        assert np.array_equal(got, g["orient_%s_%d" % (name, m)])


@pytest.mark.parametrize("filt", (C.BILINEAR, C.BICUBIC))
def test_resize_bit_exact_in_one_launch(filt):
    g, _ = fixtures()
    cases = C.resize_cases(g["composite"], g["face"])
    names = [c[0] for c in cases]
    assert names[:5] == ["fast", "down", "up", "equal", "one"] and cases[5][2] % 4 != 0 and cases[6][0] == "checker"
    assert (cases[0][1].shape[:2], cases[0][2:]) == ((170, 300), (320, 181))
    taps = max(len(k) for _, k in C.axis_coeffs(300, 40, filt))
    assert taps >= (15 if filt == C.BILINEAR else 30)           # the support is many taps
    images = [c[1] for c in cases]
    buf, meta_out = MA.img_resize(images, np.array([(c[2], c[3]) for c in cases], np.int64), filt)
    bad = []
    for (name, im, ow, oh), got in zip(cases, unpack_checked(buf, meta_out)):
        want = g["resize_%s_%d" % (name, filt)]
        assert got.shape == want.shape == (oh, ow, 3)
        if not np.array_equal(got, want):
            bad.append((name, int((got != want).sum())))
    assert not bad, bad
    if filt == C.BICUBIC:                                       # the overshoot met both clips
        want = g["resize_checker_%d" % filt]
        assert want.min() == 0 and want.max() == 255
    # a source with a row pitch and a guarded destination, straight through the library
    flat, meta = A.pack(images[5:8], pitch_extra=5)
    sizes = np.array([(c[2], c[3]) for c in cases[5:8]], np.int64)
    whole_src = dev(flat)
    got_buf, got_meta = MA.img_resize((whole_src, meta), sizes, filt)
    for (name, im, ow, oh), got in zip(cases[5:8], unpack_checked(got_buf, got_meta)):
        assert np.array_equal(got, g["resize_%s_%d" % (name, filt)]), name


def test_resize_guard_bands_and_workspace():
    g, _ = fixtures()
    images = [g["face"], A.smooth_image(37, 53)]
    sizes = np.array([(31, 50), (97, 30)], np.int64)
    buf, meta = ijb.pack_images(images)
    meta_out, total = packed.layout(sizes[:, 1], sizes[:, 0])
    hostsz = np.ascontiguousarray(np.stack([meta[:, 1], meta[:, 2], sizes[:, 1], sizes[:, 0]], 1))
    ws_bytes = _lib.value("msml_img_resize_workspace", hostsz.ctypes.data, 2)
    assert ws_bytes == 112 * 96 + 37 * 292
    jobs = np.zeros((2, 5), np.int64)
    parts, used = [], 0
    for i in range(2):
        for col, (a, b) in ((0, (meta[i, 2], sizes[i, 0])), (2, (meta[i, 1], sizes[i, 1]))):
            tab = MA.resample_rows(int(a), int(b), C.BICUBIC)
            jobs[i, col], jobs[i, col + 1] = used, tab.shape[1] - 2
            parts.append(tab.reshape(-1))
            used += tab.size
    jobs[1, 4] = 112 * 96
    whole, out = guarded(total)
    whole_ws, ws = guarded(ws_bytes)
    args = (buf.cuda(), dev(meta), out, dev(meta_out), dev(np.concatenate(parts)), dev(jobs), hostsz.ctypes.data, 2,
            C.BICUBIC, ws)
    _lib.call("msml_img_resize", *args, ws_bytes)
    torch.cuda.synchronize()
    assert bands_untouched(whole) and bands_untouched(whole_ws)
    for im, (ow, oh), got in zip(images, sizes, unpack_checked(out, meta_out)):
        assert np.array_equal(got, C.resize(im, int(ow), int(oh), C.BICUBIC))
    # the refusals come before any launch: the destination stays as it was
    before = whole.clone()
    assert _lib.call_status("msml_img_resize", *args, ws_bytes - 1) == -5
    assert _lib.call_status("msml_img_resize", *args[:8], 1, ws, ws_bytes) == -4
    assert _lib.call_status("msml_img_resize", *args[:7], 0, C.BICUBIC, ws, ws_bytes) == -4
    assert _lib.call_status("msml_img_resize", args[0], args[1], out[1:], *args[3:], ws_bytes) == -1
    plan = np.array([[5, 112, 112], [0, 37, 53]], np.int64)
    oargs = (buf.cuda(), buf.numel(), dev(meta), dev(np.array([5, 0], np.int32)), out, dev(meta_out))
    assert _lib.call_status("msml_img_orient", *oargs, plan.ctypes.data, 2) == -4
    plan[0, 0] = 0
    assert _lib.call_status("msml_img_orient", *oargs, plan.ctypes.data, 0) == -4
    assert _lib.call_status("msml_img_orient", *oargs[:4], None, oargs[5], plan.ctypes.data, 2) == -1
    torch.cuda.synchronize()
    assert torch.equal(whole, before)


def test_align_multi_crops_from_the_devices_own_landmarks():
    g, det = fixtures()
    images = [g["composite"], g["face"]]
    crops, inv, boxes = MA.align_multi(det, images, min_face_size=24.0)
    assert [c.shape[0] for c in crops] == [3, 1] and [len(b) for b in boxes] == [3, 1]
    assert all(c.is_cuda and c.dtype == torch.uint8 and tuple(c.shape[1:]) == (112, 112, 3) for c in crops)
    for img, c, ti, b in zip(images, crops, inv, boxes):
        assert (np.diff(b[:, 4]) <= 0).all()                    # the detector's order: descending score
        want_c, want_inv, want_b = C.align_multi(device_detect, img, min_face_size=24.0)
        assert np.array_equal(want_b, b)
        assert np.array_equal(c.cpu().numpy(), want_c)
        assert want_c.any(axis=(1, 2, 3)).all()
        for got, want in zip(ti, want_inv):
            assert np.abs(got - want).max() <= ulp_bound(want)
    one, inv1, boxes1 = MA.align_multi(det, images, limit=1, min_face_size=24.0)
    assert [c.shape[0] for c in one] == [1, 1] and [len(b) for b in boxes1] == [1, 1] and inv1[0].shape == (1, 2, 3)
    assert torch.equal(one[0][0], crops[0][0]) and torch.equal(one[1], crops[1])
    # another crop size, and an image without a face
    c96, _, _ = MA.align_multi(det, [g["face"], np.zeros((64, 64, 3), np.uint8)], min_face_size=24.0, crop_size=(96, 112))
    want, _, _ = C.align_multi(device_detect, g["face"], min_face_size=24.0, crop_size=(96, 112))
    assert tuple(c96[0].shape) == (1, 112, 96, 3) and np.array_equal(c96[0].cpu().numpy(), want)
    assert tuple(c96[1].shape) == (0, 112, 96, 3)
    # align: the first face of each
    first, found, inv_first = MA.align(det, [g["composite"], np.zeros((64, 64, 3), np.uint8), g["face"]])
    assert found.tolist() == [True, False, True] and not first[1].any() and not inv_first[1].any()
    w0 = C.align_multi(device_detect, g["composite"])
    assert np.array_equal(first[0].cpu().numpy(), w0[0][0]) and np.abs(inv_first[0] - w0[1][0]).max() <= ulp_bound(w0[1][0])


def _fully_cases(g):
    return [g["face"], C.transpose(g["face"], C.ROTATE_180), np.zeros((64, 64, 3), np.uint8), g["composite"]]


@pytest.mark.parametrize("fast", (True, False))
def test_align_fully_by_rounds(fast):
    g, det = fixtures()
    images = _fully_cases(g)
    calls = []
    real = det.detect_faces
    det.detect_faces = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        crops, found, orientation, inv, score = MA.align_fully(det, images, fast_mode=fast)
    finally:
        del det.detect_faces
    assert len(calls) == 3                                      # ONE detector call per round, whatever the widths
    assert found.tolist() == [True, True, False, True]
    assert orientation.tolist() == [0, 1, -1, 0] == list(g["fully_%s_orientation" % ("fast" if fast else "slow")])
    assert tuple(crops.shape) == (4, 112, 112, 3) and not crops[2].any() and score[2] == 0 and not inv[2].any()
    for k, img in enumerate(images):
        want = C.align_fully(device_detect, img, fast_mode=fast)
        if want is None:
            assert not found[k]
            continue
        assert want["orientation"] == orientation[k] and want["score"] == score[k]
        assert np.array_equal(crops[k].cpu().numpy(), want["crop"]), k
        assert np.abs(inv[k] - want["tfm_inv"]).max() <= ulp_bound(want["tfm_inv"])
    again = MA.align_fully(det, images, fast_mode=fast)
    assert torch.equal(again[0], crops) and np.array_equal(again[3], inv) and np.array_equal(again[4], score)


def test_get_landmarks_every_orientation():
    g, det = fixtures()
    faces, boxes = MA.get_landmarks(det, [g["face"], np.zeros((64, 64, 3), np.uint8)])
    want, want_boxes = C.get_landmarks(device_detect, g["face"])
    assert len(faces[0]) == len(want) == int(g["landmarks_slow_found"].sum()) and faces[1] == [] and len(boxes[1]) == 0
    assert np.array_equal(boxes[0], want_boxes)
    for (crop, pts), (wcrop, wpts) in zip(faces[0], want):
        assert tuple(crop.shape) == (256, 256, 3) and np.array_equal(pts, wpts)
        assert np.array_equal(crop.cpu().numpy(), wcrop)
    fast, _ = MA.get_landmarks(det, [g["face"]], fast_mode=True)
    want, _ = C.get_landmarks(device_detect, g["face"], fast_mode=True)
    assert len(fast[0]) == len(want) == int(g["landmarks_fast_found"].sum())
    for (crop, pts), (wcrop, wpts) in zip(fast[0], want):
        assert np.array_equal(pts, wpts) and np.array_equal(crop.cpu().numpy(), wcrop)


def test_two_runs_give_the_same_bits():
    g, det = fixtures()
    images = [g["composite"], g["face"], A.smooth_image(37, 53)]
    a = MA.img_resize(images, (97, 61), C.BICUBIC)
    b = MA.img_resize(images, (97, 61), C.BICUBIC)
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a = MA.img_orient(images, [4, 2, 0])
    b = MA.img_orient(images, [4, 2, 0])
    assert torch.equal(a[0], b[0])
    c1 = MA.align_multi(det, images[:2], min_face_size=24.0)
    c2 = MA.align_multi(det, images[:2], min_face_size=24.0)
    assert all(torch.equal(x, y) for x, y in zip(c1[0], c2[0])) and all(np.array_equal(x, y) for x, y in zip(c1[1], c2[1]))


def test_align_and_embed_equals_the_model_on_the_pairs():
    from msml_amd.backbones import MSML
    from oracle.fill import fill_module
    from tests import ijb_cases
    g, det = fixtures()
    peer = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
    torch.manual_seed(0)
    model = fill_module(MSML("iresnet18", "unet", (1, 1, 1, 1), 8, fp16=False, fm_params=(3, 2, "sigmoid", "mul"),
                             header_type="AMArcFace", peer_params=peer)).cuda().eval()
    images = [g["composite"], np.zeros((64, 64, 3), np.uint8), g["face"]]
    feats, owner, found = MA.align_and_embed(model, det, images, which="multi", min_face_size=24.0)
    crops, _, _ = MA.align_multi(det, images, min_face_size=24.0)
    with torch.no_grad():
        want = model(ijb.pair_inputs(torch.cat(crops), None))[0].float().reshape(4, -1)
    assert owner.tolist() == [0, 0, 0, 2] and found.tolist() == [True, False, True]
    assert feats.dtype == torch.float32 and feats.is_cuda and torch.equal(feats, want)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 1e-3
    by3, _, _ = MA.align_and_embed(model, det, images, which="multi", batch=3, min_face_size=24.0)
    assert float((by3 - want).abs().max()) <= ijb_cases.tolerance(1, want.shape[1] // 2)
    f1, o1, _ = MA.align_and_embed(model, det, images, which="first")
    assert [len(device_detect(im, 64.0, (0.6, 0.7, 0.8))[1]) > 0 for im in images] == [True, False, True]
    f2, o2, fd2 = MA.align_and_embed(model, det, images, which="fully")
    assert o1.tolist() == [0, 2] == o2.tolist() and fd2.tolist() == [True, False, True]
    assert tuple(f1.shape) == (2, want.shape[1]) == tuple(f2.shape)
    none, o0, f0 = MA.align_and_embed(model, det, [images[1]], which="multi")
    assert none is None and o0.size == 0 and f0.tolist() == [False]
