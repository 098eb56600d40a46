"""Writes tests/golden/g14_mtcnn_align.npz, the fixture of the alignment tests (tests/test_mtcnn_align_cpu.py,
tests/test_gpu_mtcnn_align.py): what the reference's own code and Pillow give for the cases of tests/mtcnn_align_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_mtcnn_align.py [REFERENCE_ROOT]

From the reference, none of whose text goes into the file:
  * mtcnn_pytorch/src/matlab_cp2tform.py is imported as it is (it needs only numpy);
  * align_trans.py imports cv2, which does not exist here: get_reference_facial_points, its constants and
    warp_and_crop_face are cut out of its syntax tree, and warp_and_crop_face runs with a stand-in `cv2` whose warpAffine
    hands back the matrix it was given -- that yields the template after the shrink of :277-284 (logged from the call of
    get_similarity_transform_for_cv2), tfm and tfm_inv;
  * MTCNN.align_fully and MTCNN.get_landmarks are cut out of eval/preprocess/mtcnn.py and run with `self.detect_faces`
    either a stand-in that returns prepared boxes and landmarks (the point and box maps for i = 0..3 on a non-square
    photo; get_landmarks' `boxes`, which it builds and drops, are logged from its np.concatenate) or the reference's own
    detector as tools/make_golden_mtcnn.py drives it (which orientation finds the face in the cases of the GPU test).
From Pillow: Image.resize with BILINEAR and BICUBIC and Image.transpose for the image cases; img.resize(size) without a
filter is asserted equal to BICUBIC.  The numpy and Pillow versions are recorded."""
import ast
import os
import sys
import types
import warnings

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
GOLD = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(REF, "eval", "preprocess", "mtcnn_pytorch", "src")
LIMIT = 1 << 20


def cut(path, names):
    """The top-level assignments, classes and functions `names` of a file, as a module body."""
    tree = ast.parse(open(path).read())
    body = []
    for n in tree.body:
        if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names:
            body.append(n)
        elif isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id in names for t in n.targets):
            body.append(n)
    return ast.Module(body=body, type_ignores=[])


def cut_methods(path, cls_name, names):
    tree = ast.parse(open(path).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name][0]
    return ast.Module(body=[n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names], type_ignores=[])


def load_align_trans():
    sys.path.insert(0, SRC)
    import matlab_cp2tform as cp
    log = []

    def fit(src_pts, dst_pts, reflective=True):
        log.append((np.array(src_pts), np.array(dst_pts)))
        return cp.get_similarity_transform_for_cv2(src_pts, dst_pts, reflective)

    ns = {"np": np, "cv2": types.SimpleNamespace(warpAffine=lambda img, tfm, size: tfm),
          "get_similarity_transform_for_cv2": fit}
    names = ("REFERENCE_FACIAL_POINTS", "DEFAULT_CROP_SIZE", "FaceWarpException", "get_reference_facial_points",
             "warp_and_crop_face")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # `is` with a literal
        exec(compile(cut(os.path.join(SRC, "align_trans.py"), names), "align_trans", "exec"), ns)
    return cp, ns, log


class LoggingNumpy:
    """numpy with a concatenate that keeps what it returned."""

    def __init__(self):
        self.joined = []

    def __getattr__(self, name):
        return getattr(np, name)

    def concatenate(self, *a, **k):
        out = np.concatenate(*a, **k)
        self.joined.append(out.copy())
        return out


def load_methods(ns_align):
    npx = LoggingNumpy()
    ns = {"np": npx, "Image": Image, "warp_and_crop_face": ns_align["warp_and_crop_face"]}
    exec(compile(cut_methods(os.path.join(REF, "eval", "preprocess", "mtcnn.py"), "MTCNN",
                             ("align_fully", "get_landmarks")), "mtcnn", "exec"), ns)
    return ns, npx


def main():
    sys.path.insert(0, ROOT)
    from tests import mtcnn_align_cases as mac
    warnings.simplefilter("ignore", FutureWarning)
    cp, ns, fit_log = load_align_trans()
    warp_and_crop_face = ns["warp_and_crop_face"]
    out = {"numpy_version": np.array(np.__version__), "pillow_version": np.array(PIL.__version__)}
    with np.load(os.path.join(GOLD, "g13_mtcnn.npz")) as z:
        composite, face = z["composite"], z["face"]
        real = np.concatenate([z["c24_landmarks"], z["f24_landmarks"]]).astype(np.float32)
    assert real.shape == (4, 10)

    # the template: MTCNN() holds get_reference_facial_points(default_square=True); the shrink happens in every warp
    reference = ns["get_reference_facial_points"](default_square=True)
    some = [[real[0][j], real[0][j + 5]] for j in range(5)]
    for w, h in ((112, 112), (96, 112), (256, 256), (128, 96)):
        del fit_log[:]
        warp_and_crop_face(None, some, reference, crop_size=(w, h), return_trans_inv=True)
        out["template_%d_%d" % (w, h)] = fit_log[0][1]
        assert fit_log[0][1].dtype == np.float32
        assert np.array_equal(mac.reference_points((w, h)), fit_log[0][1]), (w, h)
    del fit_log[:]
    warp_and_crop_face(None, some, ns["get_reference_facial_points"](default_square=False), crop_size=(112, 112))
    out["template_112_112_notsquare"] = fit_log[0][1]

    # the fit: jittered real landmark sets, mirrored ones, and one whose points all coincide
    rng = np.random.default_rng(14)
    sets = []
    for k in range(66):
        p = np.stack([real[k % 4][0:5], real[k % 4][5:10]], 1).astype(np.float64)
        c = p.mean(0)
        th, sc = rng.uniform(-0.6, 0.6), rng.uniform(0.5, 3.0)
        rot = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        p = (p - c) @ rot.T + c + rng.uniform(-20, 200, 2) + rng.standard_normal((5, 2)) * 0.8 * sc
        if k % 11 == 10:                                        # a mirrored photo: the second fit wins
            p[:, 0] = 300.0 - p[:, 0]
        sets.append(p.astype(np.float32))
    sets.append(np.full((5, 2), 57.25, np.float32))             # all points equal
    sets = np.stack(sets)
    tfm, inv, mirrored = [], [], []
    for p in sets:
        for size, store in (((112, 112), True), ((256, 256), False)):
            del fit_log[:]
            t, ti = warp_and_crop_face(None, p.tolist(), reference, crop_size=size, return_trans_inv=True)
            assert np.array_equal(fit_log[0][0], p) and t.dtype == np.float64
            if store:
                t1 = cp.findNonreflectiveSimilarity(p.copy(), fit_log[0][1].copy())[0]
                tfm.append(t), inv.append(ti), mirrored.append(not np.allclose(t, t1[:, 0:2].T))
    out["fit_points"], out["fit_tfm"], out["fit_inv"] = sets, np.stack(tfm), np.stack(inv)
    out["fit_mirrored"] = np.array(mirrored)
    out["fit_degenerate"] = np.array([bool((p == p[0]).all()) for p in sets])
    assert out["fit_mirrored"][:-1].sum() == 6 and out["fit_degenerate"].sum() == 1
    for k in np.flatnonzero(~out["fit_degenerate"]):
        t, ti = mac.similarity(sets[k], mac.reference_points((112, 112)))
        assert np.abs(t - tfm[k]).max() <= 1e-9 * np.abs(tfm[k]).max(), k
        assert np.abs(ti - inv[k]).max() <= 1e-9 * np.abs(inv[k]).max(), k
    try:
        cp.get_similarity_transform_for_cv2(sets[0].copy(), np.full((5, 2), 3.0, np.float32))
        raise AssertionError("the rank test did not fire")
    except Exception as e:
        assert "twoUniquePointsReq" in str(e)

    # Pillow: resize with both filters, transpose with the five methods
    for name, img, ow, oh in mac.resize_cases(composite, face):
        pil = Image.fromarray(img)
        for filt, const in ((mac.BILINEAR, Image.BILINEAR), (mac.BICUBIC, Image.BICUBIC)):
            got = np.asarray(pil.resize((ow, oh), const), np.uint8)
            assert np.array_equal(mac.resize(img, ow, oh, filt), got), (name, filt)
            out["resize_%s_%d" % (name, filt)] = got
        assert np.array_equal(np.asarray(pil.resize((ow, oh))), out["resize_%s_%d" % (name, mac.BICUBIC)]), name
    for name, img in mac.orient_cases(composite, face):
        for method in range(5):
            got = np.asarray(Image.fromarray(img).transpose(method), np.uint8)
            assert np.array_equal(mac.transpose(img, method), got), (name, method)
            out["orient_%s_%d" % (name, method)] = got

    # the point and box maps of align_fully / get_landmarks on a non-square photo, from prepared detections
    meth, npx = load_methods(ns)
    photo = Image.fromarray(composite)                          # 300 x 170
    prepared_lm = np.stack([real[1] * np.float32(0.5) + np.float32(3.25), real[2]]).astype(np.float32)
    prepared_box = np.array([[20.5, 30.25, 90.0, 110.75, 0.99], [120.0, 15.5, 160.25, 70.0, 0.9]])
    got_pts = []
    ns_warp = meth["warp_and_crop_face"]
    meth["warp_and_crop_face"] = lambda img, pts, ref, **k: (got_pts.append(np.float32(pts)), None)[:0] + (np.zeros((2, 2, 3), np.uint8), None)
    me = types.SimpleNamespace(reference=reference,
                               detect_faces=lambda img, **k: (prepared_box.copy(), prepared_lm.copy()))
    out["map_landmarks"], out["map_boxes"] = prepared_lm, prepared_box
    for i in range(4):
        del got_pts[:], npx.joined[:]
        meth["align_fully"](me, photo, return_trans_inv=True, ori=[i], fast_mode=False)
        out["map_points_%d" % i] = got_pts[0]
        meth["get_landmarks"](me, photo, ori=[i])
        out["map_boxes_%d" % i] = npx.joined[-1]
        assert np.array_equal(got_pts[1], got_pts[0])
        assert np.array_equal(mac.map_points(prepared_lm[0], i, 300, 170), got_pts[0]), i
        assert np.array_equal(mac.map_boxes(prepared_box, i, 300, 170), npx.joined[-1]), i
    # fast mode: the landmarks are divided by the scale in float32
    del got_pts[:]
    meth["align_fully"](me, photo, return_trans_inv=True, ori=[3], fast_mode=True)
    out["map_points_fast_3"] = got_pts[0]
    assert np.array_equal(mac.map_points(prepared_lm[0] / np.float32(320. / 300), 3, 300, 170), got_pts[0])
    meth["warp_and_crop_face"] = ns_warp

    # which orientation finds the face: the reference's own detector on the cases of the GPU test
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_mtcnn as g13
    nets, (detect_cut, _) = g13.reference()
    n3 = types.SimpleNamespace(pnet=nets.PNet().eval(), rnet=nets.RNet().eval(), onet=nets.ONet().eval())
    os.chdir(ROOT)

    def real_detect(img, min_face_size=64.0, thresholds=(0.6, 0.7, 0.8)):
        return detect_cut(n3, img, min_face_size, list(thresholds), [0.7, 0.7, 0.7], 0.707)

    me = types.SimpleNamespace(reference=reference, detect_faces=real_detect)
    cases = [face, mac.transpose(face, mac.ROTATE_180), np.zeros((64, 64, 3), np.uint8), composite]
    for fast in (True, False):
        orientation, points, score = [], [], []
        for img in cases:
            found = []
            saved = me.detect_faces

            def logging_detect(im, **k):
                b, l = real_detect(im, **k)
                found.append(len(l))
                if len(l):
                    score.append(float(b[0][4]))
                return b, l

            me.detect_faces = logging_detect
            del fit_log[:]
            res = meth["align_fully"](me, Image.fromarray(img), return_trans_inv=True, fast_mode=fast)
            me.detect_faces = saved
            if res[0] is None:
                orientation.append(-1), points.append(np.zeros((5, 2), np.float32))
            else:
                orientation.append((0, 1, 3)[len(found) - 1]), points.append(fit_log[0][0])
        tag = "fast" if fast else "slow"
        out["fully_%s_orientation" % tag], out["fully_%s_points" % tag] = np.array(orientation), np.stack(points)
        out["fully_%s_score" % tag] = np.array(score)
        print("align_fully", tag, orientation)
    for fast in (True, False):
        counts = []
        me.detect_faces = lambda im, **k: (lambda r: (counts.append(len(r[1])), r)[1])(real_detect(im, **k))
        faces = meth["get_landmarks"](me, Image.fromarray(face), fast_mode=fast)
        out["landmarks_%s_found" % ("fast" if fast else "slow")] = np.array(counts) > 0
        assert len(faces) == int((np.array(counts) > 0).sum())
        print("get_landmarks", "fast" if fast else "slow", counts)

    path = os.path.join(GOLD, "g14_mtcnn_align.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= LIMIT


if __name__ == "__main__":
    main()
