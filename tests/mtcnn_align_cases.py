"""numpy restatement of the four alignment methods of the reference's MTCNN class (eval/preprocess/mtcnn.py:25-158) and of
what they call, for tests/test_mtcnn_align_cpu.py, tests/test_gpu_mtcnn_align.py and tools/make_golden_mtcnn_align.py.
Independent of msml_amd.mtcnn_align; builds on tests/mtcnn_cases.py (the detector, Pillow's triangle filter) and
tests/align_cases.py (cv2.warpAffine).  No torch, no PIL, no GPU.

* `resize(a, out_w, out_h, filter)`   Image.resize with BILINEAR (2) or BICUBIC (3): Resample.c's two passes
* `transpose(a, method)`              Image.transpose for methods 0..4
* `reference_points(crop_size, sq)`   get_reference_facial_points + the shrink of warp_and_crop_face (align_trans.py:277-284)
* `similarity(points, ref)`           get_similarity_transform_for_cv2 (matlab_cp2tform.py) for one point set
* `map_points(lm10, i, w, h)`         the landmark maps of mtcnn.py:60-67 / :125-142
* `map_boxes(box, i, w, h)`           the box maps of mtcnn.py:129-147
* `warp_face(img, tfm, crop_size)`    cv2.warpAffine(img, tfm, crop_size) as tests/align_cases.py restates it
* `align_multi / align_fully / get_landmarks`  the methods themselves, on a `detect(img, min_face_size, thresholds)`
                                      callable: the numpy detector on the CPU, the device's own results in the GPU tests
"""
import numpy as np

from tests import align_cases as ac
from tests import mtcnn_cases as mc

BILINEAR, BICUBIC = 2, 3
FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, ROTATE_90, ROTATE_180, ROTATE_270 = range(5)


# ---------------------------------------------------------------------------------------------------------------------
# Pillow: Resample.c

def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTERS = {BILINEAR: (mc._triangle, 1.0), BICUBIC: (_bicubic, 2.0)}


def axis_coeffs(insz, outsz, filter):
    """precompute_coeffs + normalize_coeffs_8bpc: [(first tap, [22-bit integer coefficients])] per output position."""
    kernel, support = _FILTERS[filter]
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = support * fs
    ss = 1.0 / fs
    out = []
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insz)
        k = [kernel((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        out.append((xmin, [int(-0.5 + v * (1 << mc.PRECISION)) if v < 0 else int(0.5 + v * (1 << mc.PRECISION))
                           for v in k]))
    return out


def _pass(a, axis, outsz, filter):
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    res = np.empty((outsz,) + a.shape[1:], np.int64)
    for xx, (xmin, k) in enumerate(axis_coeffs(a.shape[0], outsz, filter)):
        acc = np.full(a.shape[1:], 1 << (mc.PRECISION - 1), np.int64)
        for j, c in enumerate(k):
            acc += a[xmin + j] * c
        res[xx] = np.clip(acc >> mc.PRECISION, 0, 255)
    return np.moveaxis(res.astype(np.uint8), 0, axis)


def resize(a, out_w, out_h, filter=BICUBIC):
    """Image.fromarray(a).resize((out_w, out_h), filter): horizontal pass, then vertical, each skipped at equal size."""
    if a.shape[1] != out_w:
        a = _pass(a, 1, out_w, filter)
    if a.shape[0] != out_h:
        a = _pass(a, 0, out_h, filter)
    return np.ascontiguousarray(a)


def transpose(a, method):
    """Image.fromarray(a).transpose(method)"""
    if method == FLIP_LEFT_RIGHT:
        out = a[:, ::-1]
    elif method == FLIP_TOP_BOTTOM:
        out = a[::-1]
    elif method == ROTATE_90:                     # counter-clockwise: out[y][x] = in[x][W - 1 - y]
        out = a[:, ::-1].transpose(1, 0, 2)
    elif method == ROTATE_180:
        out = a[::-1, ::-1]
    elif method == ROTATE_270:                    # clockwise: out[y][x] = in[H - 1 - x][y]
        out = a[::-1].transpose(1, 0, 2)
    else:
        raise ValueError(method)
    return np.ascontiguousarray(out)


# ---------------------------------------------------------------------------------------------------------------------
# the template and the fit

FIVE_POINTS = [[30.29459953, 51.69630051], [65.53179932, 51.50139999], [48.02519989, 71.73660278],
               [33.54930115, 92.3655014], [62.72990036, 92.20410156]]


def reference_points(crop_size=(112, 112), square=True):
    """The float32 [5][2] points warp_and_crop_face fits to, for crop_size = (w, h)."""
    pts = np.array(FIVE_POINTS)
    size = np.array((96, 112))
    if square:
        pts += (max(size) - size) / 2
    ref = np.float32(pts)
    if crop_size[0] == 96 and crop_size[1] == 112:
        ref[:, 0] = (ref[:, 0] - crop_size[0] / 2) * 0.85 + crop_size[0] / 2
        ref[:, 1] = (ref[:, 1] - crop_size[1] / 2) * 0.85 + crop_size[1] / 2
    else:
        ref = (ref - 112 / 2) * 0.85 + 112 / 2
        ref *= crop_size[0] / 112.
    assert ref.dtype == np.float32
    return ref


def _nonreflective(uv, xy):
    m = xy.shape[0]
    x, y = xy[:, 0:1], xy[:, 1:2]
    X = np.vstack((np.hstack((x, y, np.ones((m, 1)), np.zeros((m, 1)))),
                   np.hstack((y, -x, np.zeros((m, 1)), np.ones((m, 1))))))
    U = np.vstack((uv[:, 0:1], uv[:, 1:2]))
    if np.linalg.matrix_rank(X) < 4:
        raise ValueError("cp2tform:twoUniquePointsReq")
    r = np.squeeze(np.linalg.lstsq(X, U, rcond=None)[0])
    sc, ss, tx, ty = r
    tinv = np.array([[sc, -ss, 0], [ss, sc, 0], [tx, ty, 1]])
    t = np.linalg.inv(tinv)
    t[:, 2] = np.array([0, 0, 1])
    return t, tinv


def _forward(trans, uv):
    return np.dot(np.hstack((uv, np.ones((uv.shape[0], 1)))), trans)[:, 0:-1]


def similarity(points, ref, reflective=True):
    """(tfm [2][3], tfm_inv [2][3]) of get_similarity_transform_for_cv2(points, ref) for float32 [5][2] inputs.  As in
    the reference, the mirrored copy of `ref` REPLACES it before the two residuals are taken (findSimilarity's xyR is
    xy itself), so both norms are distances to the mirrored template."""
    uv, xy = np.float32(points), np.float32(ref).copy()
    if not reflective:
        t, tinv = _nonreflective(uv, xy)
    else:
        t1, t1inv = _nonreflective(uv, xy)
        xy[:, 0] = -1 * xy[:, 0]
        t2r, _ = _nonreflective(uv, xy)
        t2 = np.dot(t2r, np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]))
        norm1 = np.linalg.norm(_forward(t1, uv) - xy)
        norm2 = np.linalg.norm(_forward(t2, uv) - xy)
        if norm1 <= norm2:
            t, tinv = t1, t1inv
        else:
            t, tinv = t2, np.linalg.inv(t2)
    return t[:, 0:2].T.copy(), tinv[:, 0:2].T.copy()


def warp_face(img, tfm, crop_size):
    """cv2.warpAffine(img, tfm, (w, h)): uint8 [h][w][3]."""
    return ac.warp(img, ac.invert(tfm), crop_size[1], crop_size[0], swap_rb=False)


# ---------------------------------------------------------------------------------------------------------------------
# the orientation maps

def five(lm10):
    """[[x_j, y_j]] of one landmark row x0..x4 y0..y4 (float32)."""
    lm10 = np.asarray(lm10, np.float32)
    return np.stack([lm10[0:5], lm10[5:10]], 1)


def map_points(lm10, i, w, h):
    """mtcnn.py:60-67: the five points found in the copy transposed by method i + 1, in the original w x h photo."""
    lm10 = np.asarray(lm10, np.float32)
    x, y = lm10[0:5], lm10[5:10]
    if i == 0:
        out = [x, y]
    elif i == 1:
        out = [np.float32(w - 1) - y, x]
    elif i == 2:
        out = [np.float32(w - 1) - x, np.float32(h - 1) - y]
    elif i == 3:
        out = [y, np.float32(h - 1) - x]
    else:
        raise ValueError(i)
    return np.stack(out, 1).astype(np.float32)


def map_boxes(box, i, w, h):
    """mtcnn.py:129-147 on a copy of box [n][5]."""
    box = np.array(box, np.float64)
    if i == 1:
        x1, y1, x2, y2 = w - 1 - box[:, 1], box[:, 0], w - 1 - box[:, 3], box[:, 2]
        box[:, :4] = np.stack((x2, y1, x1, y2), axis=1)
    elif i == 2:
        x1, y1, x2, y2 = w - 1 - box[:, 0], h - 1 - box[:, 1], w - 1 - box[:, 2], h - 1 - box[:, 3]
        box[:, :4] = np.stack((x2, y2, x1, y1), axis=1)
    elif i == 3:
        x1, y1, x2, y2 = box[:, 1], h - 1 - box[:, 0], box[:, 3], h - 1 - box[:, 2]
        box[:, :4] = np.stack((x1, y2, x2, y1), axis=1)
    return box


# ---------------------------------------------------------------------------------------------------------------------
# the methods; detect(img, min_face_size, thresholds) -> (boxes f64 [n][5], landmarks f32 [n][10])

def numpy_detector(weights, factor=0.707):
    def detect(img, min_face_size, thresholds):
        b, l, _ = mc.detect_faces(img, weights, min_face_size, tuple(thresholds), (0.7, 0.7, 0.7), factor)
        return b, l
    return detect


def align_multi(detect, img, limit=None, min_face_size=64.0, crop_size=(112, 112), thresholds=(0.6, 0.7, 0.8),
                square=True):
    """(crops [n][h][w][3], tfm_inv [n][2][3], boxes [n][5]); n = 0 where the reference returns None."""
    boxes, landmarks = detect(img, min_face_size, thresholds)
    if limit:
        boxes, landmarks = boxes[:limit], landmarks[:limit]
    ref = reference_points(crop_size, square)
    crops = np.zeros((len(landmarks), crop_size[1], crop_size[0], 3), np.uint8)
    inv = np.zeros((len(landmarks), 2, 3))
    for k, lm in enumerate(landmarks):
        tfm, inv[k] = similarity(five(lm), ref)
        crops[k] = warp_face(img, tfm, crop_size)
    return crops, inv, boxes


def shrunken(img, sw):
    """The copy align_fully / get_landmarks detect on and its scale: img.resize((int(w * scale), int(h * scale)))."""
    h, w = img.shape[:2]
    scale = sw / w
    return resize(img, int(w * scale), int(h * scale), BICUBIC), scale


def align_fully(detect, img, crop_size=(112, 112), ori=(0, 1, 3), fast_mode=True, thresholds=(0.6, 0.7, 0.7),
                square=True):
    """None, or dict(crop, orientation, points, tfm_inv, score)."""
    h, w = img.shape[:2]
    sw = 320. if fast_mode else w
    small, scale = shrunken(img, sw)
    for i in ori:
        rimg = transpose(small, i + 1) if i > 0 else small
        box, landmarks = detect(rimg, sw / 10, thresholds)
        if len(landmarks) == 0:
            continue
        landmarks = landmarks / np.float32(scale)
        pts = map_points(landmarks[0], i, w, h)
        tfm, inv = similarity(pts, reference_points(crop_size, square))
        return dict(crop=warp_face(img, tfm, crop_size), orientation=i, points=pts, tfm_inv=inv, score=box[0][4])
    return None


def get_landmarks(detect, img, min_face_size=32, crop_size=(256, 256), fast_mode=False, ori=(0, 1, 3), square=True):
    """([(crop, points)] per orientation that found a face, boxes [m][5] mapped back and concatenated)."""
    h, w = img.shape[:2]
    sw = 640. if fast_mode else w
    small, scale = shrunken(img, sw)
    if fast_mode:
        min_face_size = sw / 20
    faces, boxes = [], np.zeros([0, 5])
    for i in ori:
        rimg = transpose(small, i + 1) if i > 0 else small
        box, landmarks = detect(rimg, min_face_size, (0.6, 0.7, 0.7))
        if len(landmarks) == 0:
            continue
        landmarks = landmarks / np.float32(scale)
        pts = map_points(landmarks[0], i, w, h)
        boxes = np.concatenate((boxes, map_boxes(box, i, w, h)), axis=0)      # the box is NOT divided by scale (:122)
        tfm, _ = similarity(pts, reference_points(crop_size, square))
        faces.append((warp_face(img, tfm, crop_size), pts))
    return faces, boxes


# ---------------------------------------------------------------------------------------------------------------------
# the image cases of the kernel tests: name -> (image, out_w, out_h)

def checkerboard(h, w, cell=3):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    v = (((y // cell) + (x // cell)) % 2 * 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([v, 255 - v, v], -1))


def resize_cases(composite, face):
    """The resize cases of the kernel test, in a fixed order: [(name, image, out_w, out_h)]."""
    return [("fast", composite, 320, 181), ("down", composite, 40, 23), ("up", face, 320, 320),
            ("equal", face, 112, 112), ("one", composite, 1, 1), ("odd", ac.smooth_image(37, 53), 31, 50),
            ("checker", checkerboard(45, 61), 97, 30), ("width_only", ac.smooth_image(5, 7), 9, 5)]


def orient_cases(composite, face):
    return [("tiny", ac.smooth_image(5, 7)), ("face", face), ("composite", composite)]
