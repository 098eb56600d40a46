"""numpy restatement of MTCNN.detect_faces for the detector tests: integer resampling as Pillow does it, f64 box
arithmetic in the reference's order of operations, the three nets in any float dtype.  No torch, no PIL, no GPU.

A `trace` dict, when given, collects the smallest margins the comparison with another implementation depends on:
  prob     |probability - threshold| of every thresholded probability
  overlap  |overlap - threshold| of every overlap NMS compares
  round    distance of every rounded value from a half-integer
  ties     the largest number of boxes in an NMS call that holds two equal scores (0: never)
"""
import numpy as np

PRECISION = 22


def _note(trace, key, values, ref=None):
    if trace is None:
        return
    v = np.asarray(values, np.float64).ravel()
    if v.size == 0:
        return
    if key == "round":
        d = np.abs(v - np.floor(v) - 0.5)
    else:
        d = np.abs(v - ref)
    trace[key] = min(trace.get(key, np.inf), float(d.min()))


# ---------------------------------------------------------------------------------------------------------------------
# Pillow: Resample.c precompute_coeffs + normalize_coeffs_8bpc for the triangle filter

def _triangle(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def axis_coeffs(insz, outsz):
    """[(first tap, [22-bit integer coefficients])] for every output position of one axis."""
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insz)
        k = [_triangle((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        out.append((xmin, [int(0.5 + v * (1 << PRECISION)) for v in k]))
    return out


def _pass(a, axis, outsz):
    """One resampling pass over `axis` of a uint8 array [h][w][c]."""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    res = np.empty((outsz,) + a.shape[1:], np.int64)
    for xx, (xmin, k) in enumerate(axis_coeffs(a.shape[0], outsz)):
        acc = np.full(a.shape[1:], 1 << (PRECISION - 1), np.int64)
        for j, c in enumerate(k):
            acc += a[xmin + j] * c
        res[xx] = np.clip(acc >> PRECISION, 0, 255)
    return np.moveaxis(res.astype(np.uint8), 0, axis)


def resize(a, out_w, out_h):
    """Image.fromarray(a).resize((out_w, out_h), BILINEAR): horizontal pass, then vertical, each skipped at equal size."""
    if a.shape[1] != out_w:
        a = _pass(a, 1, out_w)
    if a.shape[0] != out_h:
        a = _pass(a, 0, out_h)
    return a


def window(img, x0, y0, w, h):
    """The w x h cut at (x0, y0), black outside the image (get_image_boxes' img_box)."""
    H, W = img.shape[:2]
    box = np.zeros((h, w, 3), np.uint8)
    sx0, sy0, sx1, sy1 = max(x0, 0), max(y0, 0), min(x0 + w, W), min(y0 + h, H)
    if sx1 > sx0 and sy1 > sy0:
        box[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = img[sy0:sy1, sx0:sx1]
    return box


def normalise(u8, dtype=np.float32):
    """_preprocess: HWC uint8 -> CHW (x - 127.5) * 0.0078125 (exact in f32 and f64)."""
    return ((u8.astype(dtype) - dtype(127.5)) * dtype(0.0078125)).transpose(2, 0, 1)


def scales(height, width, min_face_size=64.0, factor=0.707):
    out = []
    m = 12 / min_face_size
    length = min(height, width) * m
    count = 0
    while length > 12:
        out.append(m * factor ** count)
        length *= factor
        count += 1
    return out


def level_size(height, width, s):
    import math
    return math.ceil(height * s), math.ceil(width * s)


# ---------------------------------------------------------------------------------------------------------------------
# the nets; x is [n][c][h][w], weights a dict under the reference's parameter names

def _conv(x, w, b):
    k = w.shape[2]
    win = np.lib.stride_tricks.sliding_window_view(x, (k, k), axis=(2, 3))      # n c ho wo k k
    return np.einsum("nchwij,ocij->nohw", win, w.astype(x.dtype), optimize=True) + b.astype(x.dtype)[None, :, None, None]


def _prelu(x, a):
    a = a.astype(x.dtype).reshape((1, -1) + (1,) * (x.ndim - 2))
    return np.where(x > 0, x, a * x)


def _pool(x, k):
    """MaxPool2d(k, 2, ceil_mode=True)"""
    n, c, h, w = x.shape
    ho, wo = -(-(h - k) // 2) + 1, -(-(w - k) // 2) + 1
    pad = np.full((n, c, (ho - 1) * 2 + k, (wo - 1) * 2 + k), -np.inf, x.dtype)
    pad[:, :, :h, :w] = x
    out = np.full((n, c, ho, wo), -np.inf, x.dtype)
    for i in range(k):
        for j in range(k):
            out = np.maximum(out, pad[:, :, i:i + 2 * ho:2, j:j + 2 * wo:2])
    return out


def flatten(x):
    """Flatten of get_nets.py: transpose(3, 2) first, so the feature order is c, x, y."""
    return x.transpose(0, 1, 3, 2).reshape(x.shape[0], -1)


def _fc(x, w, b):
    return x @ w.astype(x.dtype).T + b.astype(x.dtype)


def _softmax(a, axis):
    e = np.exp(a - a.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def pnet_logits(x, P):
    """[n][3][h][w] -> (class logits [n][2][oh][ow], offsets [n][4][oh][ow])"""
    f = "features."
    x = _pool(_prelu(_conv(x, P[f + "conv1.weight"], P[f + "conv1.bias"]), P[f + "prelu1.weight"]), 2)
    x = _prelu(_conv(x, P[f + "conv2.weight"], P[f + "conv2.bias"]), P[f + "prelu2.weight"])
    x = _prelu(_conv(x, P[f + "conv3.weight"], P[f + "conv3.bias"]), P[f + "prelu3.weight"])
    return _conv(x, P["conv4_1.weight"], P["conv4_1.bias"]), _conv(x, P["conv4_2.weight"], P["conv4_2.bias"])


def width_softmax(a):
    """F.softmax(a, dim=-1) of the reference's P-Net: over the WIDTH of the [n][2][h][w] class map."""
    return _softmax(a, -1)


def rnet_raw(x, P):
    """[n][3][24][24] -> (class logits [n][2], offsets [n][4])"""
    f = "features."
    x = _pool(_prelu(_conv(x, P[f + "conv1.weight"], P[f + "conv1.bias"]), P[f + "prelu1.weight"]), 3)
    x = _pool(_prelu(_conv(x, P[f + "conv2.weight"], P[f + "conv2.bias"]), P[f + "prelu2.weight"]), 3)
    x = _prelu(_conv(x, P[f + "conv3.weight"], P[f + "conv3.bias"]), P[f + "prelu3.weight"])
    x = _prelu(_fc(flatten(x), P[f + "conv4.weight"], P[f + "conv4.bias"]), P[f + "prelu4.weight"])
    return _fc(x, P["conv5_1.weight"], P["conv5_1.bias"]), _fc(x, P["conv5_2.weight"], P["conv5_2.bias"])


def onet_raw(x, P):
    """[n][3][48][48] -> (class logits [n][2], offsets [n][4], landmarks [n][10])"""
    f = "features."
    x = _pool(_prelu(_conv(x, P[f + "conv1.weight"], P[f + "conv1.bias"]), P[f + "prelu1.weight"]), 3)
    x = _pool(_prelu(_conv(x, P[f + "conv2.weight"], P[f + "conv2.bias"]), P[f + "prelu2.weight"]), 3)
    x = _pool(_prelu(_conv(x, P[f + "conv3.weight"], P[f + "conv3.bias"]), P[f + "prelu3.weight"]), 2)
    x = _prelu(_conv(x, P[f + "conv4.weight"], P[f + "conv4.bias"]), P[f + "prelu4.weight"])
    x = _prelu(_fc(flatten(x), P[f + "conv5.weight"], P[f + "conv5.bias"]), P[f + "prelu5.weight"])
    return (_fc(x, P["conv6_1.weight"], P["conv6_1.bias"]), _fc(x, P["conv6_2.weight"], P["conv6_2.bias"]),
            _fc(x, P["conv6_3.weight"], P["conv6_3.bias"]))


# ---------------------------------------------------------------------------------------------------------------------
# boxes

def generate_boxes(prob, offsets, scale, threshold, trace=None):
    """prob [oh][ow], offsets [4][oh][ow] -> [n][9] f64 in np.where's order."""
    thr = float(np.float32(threshold))
    _note(trace, "prob", prob, thr)
    ys, xs = np.nonzero(prob > thr)
    if ys.size == 0:
        return np.zeros((0, 9))
    args = [(2.0 * xs + 1.0) / scale, (2.0 * ys + 1.0) / scale, (2.0 * xs + 1.0 + 12.0) / scale,
            (2.0 * ys + 1.0 + 12.0) / scale]
    for a in args:
        _note(trace, "round", a)
    cols = [np.round(a) for a in args] + [prob[ys, xs].astype(np.float64)]
    cols += [offsets[k, ys, xs].astype(np.float64) for k in range(4)]
    return np.stack(cols, 1)


def nms(boxes, threshold=0.5, mode="union", trace=None):
    """Greedy NMS in the reference's order: descending score, the HIGHER index first among equal scores."""
    n = len(boxes)
    if n == 0:
        return []
    b = np.asarray(boxes, np.float64)
    score = b[:, 4]
    if trace is not None and np.unique(score).size < n:
        trace["ties"] = max(trace.get("ties", 0), n)
    order = sorted(range(n), key=lambda i: (score[i], i), reverse=True)
    area = (b[:, 2] - b[:, 0] + 1.0) * (b[:, 3] - b[:, 1] + 1.0)
    alive = [True] * n
    pick = []
    for pos, i in enumerate(order):
        if not alive[pos]:
            continue
        pick.append(i)
        rest = [p for p in range(pos + 1, n) if alive[p]]
        if not rest:
            continue
        j = np.array([order[p] for p in rest])
        w = np.maximum(0.0, np.minimum(b[i, 2], b[j, 2]) - np.maximum(b[i, 0], b[j, 0]) + 1.0)
        h = np.maximum(0.0, np.minimum(b[i, 3], b[j, 3]) - np.maximum(b[i, 1], b[j, 1]) + 1.0)
        inter = w * h
        ov = inter / np.minimum(area[i], area[j]) if mode == "min" else inter / (area[i] + area[j] - inter)
        _note(trace, "overlap", ov, threshold)
        for p, o in zip(rest, ov):
            if o > threshold:
                alive[p] = False
    return pick


def calibrate(boxes, offsets):
    b = np.array(boxes, np.float64)
    o = np.asarray(offsets, np.float64)
    w = b[:, 2] - b[:, 0] + 1.0
    h = b[:, 3] - b[:, 1] + 1.0
    b[:, 0] = b[:, 0] + w * o[:, 0]
    b[:, 1] = b[:, 1] + h * o[:, 1]
    b[:, 2] = b[:, 2] + w * o[:, 2]
    b[:, 3] = b[:, 3] + h * o[:, 3]
    return b


def to_square(boxes):
    """convert_to_square: the score column comes out as 0, as zeros_like leaves it."""
    b = np.asarray(boxes, np.float64)
    out = np.zeros_like(b)
    h = b[:, 3] - b[:, 1] + 1.0
    w = b[:, 2] - b[:, 0] + 1.0
    side = np.maximum(h, w)
    out[:, 0] = b[:, 0] + w * 0.5 - side * 0.5
    out[:, 1] = b[:, 1] + h * 0.5 - side * 0.5
    out[:, 2] = out[:, 0] + side - 1.0
    out[:, 3] = out[:, 1] + side - 1.0
    return out


def refine(boxes, offsets, height, width, trace=None):
    """calibrate, square, round, then correct_bboxes.  Returns (boxes clipped to the image -- the state the reference's
    in-place views leave --, windows int [n][4] = x0 y0 w h of the unclipped rounded boxes, valid [n]): valid is False
    for a box with no pixel inside the image, where the reference raises and the device drops; so is a box with a
    side of 32768 pixels or more, or a coordinate that is not finite."""
    b = to_square(calibrate(boxes, offsets))
    _note(trace, "round", b[:, :4])
    b[:, :4] = np.round(b[:, :4])
    w = b[:, 2] - b[:, 0] + 1.0
    h = b[:, 3] - b[:, 1] + 1.0
    valid = (w >= 1) & (h >= 1) & (b[:, 2] >= 0) & (b[:, 3] >= 0) & (b[:, 0] <= width - 1.0) & (b[:, 1] <= height - 1.0)
    with np.errstate(invalid="ignore"):                      # the device refuses a side of 32768 or more, and NaN / inf
        valid &= (np.abs(b[:, :2]) < 1e9).all(1) & (w < 32768) & (h < 32768)
    win = np.stack([b[:, 0], b[:, 1], w, h], 1)
    win = np.where(valid[:, None], win, 0).astype(np.int64)
    b[:, 2] = np.minimum(b[:, 2], width - 1.0)
    b[:, 3] = np.minimum(b[:, 3], height - 1.0)
    b[:, 0] = np.maximum(b[:, 0], 0.0)
    b[:, 1] = np.maximum(b[:, 1], 0.0)
    return b, win, valid


def crops(img, windows, valid, size):
    """uint8 [n][size][size][3]: the resized cuts (black for a dropped box)."""
    out = np.zeros((len(windows), size, size, 3), np.uint8)
    for i, (x0, y0, w, h) in enumerate(windows):
        if valid[i]:
            out[i] = resize(window(img, int(x0), int(y0), int(w), int(h)), size, size)
    return out


def class_prob(logits):
    return _softmax(logits, -1)[:, 1]


# ---------------------------------------------------------------------------------------------------------------------

def detect_faces(img, weights, min_face_size=64.0, thresholds=(0.6, 0.7, 0.8), nms_thresholds=(0.7, 0.7, 0.7),
                 factor=0.707, dtype=np.float64, trace=None, record=None):
    """The whole of MTCNN.detect_faces on one HWC uint8 image.  Returns (boxes f64 [n][5], landmarks f32 [n][10], dropped).
    `record`, a dict, receives every intermediate the golden file holds."""
    pw, rw, ow_ = weights
    H, W = img.shape[:2]
    rec = record if record is not None else {}
    empty = (np.zeros((0, 5)), np.zeros((0, 10), np.float32), 0)
    sc = scales(H, W, min_face_size, factor)
    rec["scales"] = np.array(sc, np.float64)
    per_scale = []
    for li, s in enumerate(sc):
        sh, sw = level_size(H, W, s)
        lvl = resize(img, sw, sh)
        a, b = pnet_logits(normalise(lvl, dtype)[None], pw)
        rec["level%d" % li], rec["pnet_a%d" % li], rec["pnet_b%d" % li] = lvl, a[0], b[0]
        boxes = generate_boxes(width_softmax(a)[0, 1], b[0], s, thresholds[0], trace)
        if len(boxes):
            per_scale.append(boxes[nms(boxes[:, :5], 0.5, "union", trace)])
    if not per_scale:
        return empty
    boxes = np.vstack(per_scale)
    boxes = boxes[nms(boxes[:, :5], nms_thresholds[0], "union", trace)]
    rec["boxes1"] = boxes.copy()
    boxes, win, valid = refine(boxes[:, :5], boxes[:, 5:], H, W, trace)
    dropped = int((~valid).sum())
    rec["boxes1r"] = boxes.copy()

    c24 = crops(img, win, valid, 24)
    rec["crops24"] = c24
    cls, off = rnet_raw(normalise_batch(c24, dtype), rw)
    rec["rnet_cls"], rec["rnet_off"] = cls, off
    prob = class_prob(cls)
    thr = float(np.float32(thresholds[1]))
    _note(trace, "prob", prob[valid], thr)
    keep = np.nonzero((prob > thr) & valid)[0]
    boxes, off = boxes[keep], off[keep]
    boxes[:, 4] = prob[keep].astype(np.float32)
    keep = nms(boxes, nms_thresholds[1], "union", trace)
    boxes, off = boxes[keep], off[keep]
    rec["boxes2"] = boxes.copy()
    boxes, win, valid = refine(boxes, off.astype(np.float32), H, W, trace)
    dropped += int((~valid).sum())
    rec["boxes2r"] = boxes.copy()
    if len(boxes) == 0:
        return empty[0], empty[1], dropped

    c48 = crops(img, win, valid, 48)
    rec["crops48"] = c48
    cls, off, lm = onet_raw(normalise_batch(c48, dtype), ow_)
    rec["onet_cls"], rec["onet_off"], rec["onet_lm"] = cls, off, lm
    prob = class_prob(cls)
    thr = float(np.float32(thresholds[2]))
    _note(trace, "prob", prob[valid], thr)
    keep = np.nonzero((prob > thr) & valid)[0]
    boxes, off, lm = boxes[keep], off[keep].astype(np.float32), lm[keep].astype(np.float32)
    boxes[:, 4] = prob[keep].astype(np.float32)
    w = boxes[:, 2] - boxes[:, 0] + 1.0
    h = boxes[:, 3] - boxes[:, 1] + 1.0
    marks = np.empty((len(boxes), 10), np.float32)
    marks[:, 0:5] = boxes[:, 0:1] + w[:, None] * lm[:, 0:5].astype(np.float64)
    marks[:, 5:10] = boxes[:, 1:2] + h[:, None] * lm[:, 5:10].astype(np.float64)
    boxes = calibrate(boxes, off)
    keep = nms(boxes, nms_thresholds[2], "min", trace)
    rec["boxes3"], rec["landmarks"] = boxes[keep], marks[keep]
    return boxes[keep], marks[keep], dropped


def normalise_batch(u8, dtype=np.float32):
    """[n][s][s][3] uint8 -> [n][3][s][s]"""
    return ((u8.astype(dtype) - dtype(127.5)) * dtype(0.0078125)).transpose(0, 3, 1, 2)


def load_golden_weights(folder):
    """The three parameter dicts from tests/golden/mtcnn_{pnet,rnet,onet}*.npz (O-Net's conv5 weight may be split)."""
    import glob
    import os
    out = []
    for name in ("pnet", "rnet", "onet"):
        d = {}
        for path in sorted(glob.glob(os.path.join(folder, "mtcnn_%s*.npz" % name))):
            with np.load(path) as z:
                for k in z.files:
                    d[k] = z[k]
        parts = sorted(k for k in d if ".part" in k)
        for base in sorted({k.split(".part")[0] for k in parts}):
            d[base] = np.concatenate([d.pop(k) for k in parts if k.startswith(base + ".part")], 0)
        out.append(d)
    return out
