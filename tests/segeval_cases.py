"""The numpy restatement of csrc/segeval.hip and msml_amd/segeval.py, and the cases its tests share.

Masks here are 2-D or 3-D boolean arrays `occ` (True = occluded) unless a function says otherwise; `index_mask` turns
one into the project's uint8 convention (0 = occluded, 1 = clean).  The labelling is a plain two-pass union-find of its
own: scipy.ndimage.label is the independent second opinion of tests/test_segeval_cpu.py, not a part of it.
"""
import functools

import numpy as np

SIZES = ((1, 1), (1, 9), (9, 1), (5, 7), (112, 112), (128, 128))
COUNT_SHAPES = ((1, 1, 1), (1, 5, 7), (3, 3, 113), (2, 112, 112), (2, 128, 128), (1, 256, 256))
DENSITIES = (0.3, 0.5, 0.593)
KINDS = {"f32": 0, "bf16": 1, "u8": 2, "i64": 3}


# ---------------------------------------------------------------------------------------------- the class rule
def logits_occluded(logits):
    """[N][2][H][W] f32 (bf16 widened exactly) -> bool [N][H][W]: clean iff b > a; ties and NaN are occluded."""
    logits = np.asarray(logits, np.float32)
    with np.errstate(invalid="ignore"):
        return ~(logits[:, 1] > logits[:, 0])


def index_occluded(mask):
    return np.asarray(mask) == 0


def index_mask(occ, dtype=np.uint8):
    return (~np.asarray(occ, bool)).astype(dtype)


# ---------------------------------------------------------------------------------------------- pixel counts
def counts(pred_occ, gt_occ):
    """int64 [N][4] = (tp, fp, fn, tn) per image, positive = occluded."""
    p, g = np.asarray(pred_occ, bool), np.asarray(gt_occ, bool)
    assert p.shape == g.shape and p.ndim == 3
    ax = (1, 2)
    return np.stack([(p & g).sum(ax), (p & ~g).sum(ax), (~p & g).sum(ax), (~p & ~g).sum(ax)], 1).astype(np.int64)


def _div(a, b):
    return float(a) / float(b) if b > 0 else float("nan")


def metrics(c):
    c = np.asarray(c, np.int64)
    tp, fp, fn, tn = (int(v) for v in (c.sum(0) if c.ndim == 2 else c))
    out = {"pixel_acc": _div(tp + tn, tp + fp + fn + tn), "iou_occ": _div(tp, tp + fp + fn),
           "iou_clean": _div(tn, tn + fp + fn), "dice_occ": _div(2 * tp, 2 * tp + fp + fn),
           "precision": _div(tp, tp + fp), "recall": _div(tp, tp + fn), "false_alarm": _div(fp, fp + tn)}
    d = [v for v in (out["iou_occ"], out["iou_clean"]) if not np.isnan(v)]
    out["miou"] = sum(d) / len(d) if d else float("nan")
    if c.ndim == 2:
        ious = [_div(r[0], r[0] + r[1] + r[2]) for r in c if r[0] + r[1] + r[2] > 0]
        out["images_defined"] = len(ious)
        out["image_iou_occ"] = float(np.mean(ious)) if ious else float("nan")
    return out


def same_metrics(a, b, keys=None):
    """Equal as floats, NaN equal to NaN."""
    keys = list(b) if keys is None else keys
    return all((np.isnan(a[k]) and np.isnan(b[k])) or a[k] == b[k] for k in keys)


# ---------------------------------------------------------------------------------------------- labelling
def _find(parent, a):
    while parent[a] != a:
        a = parent[a]
    return a


def _label_one(occ, connectivity):
    h, w = occ.shape
    prov = np.zeros((h, w), np.int64)
    parent = [0]
    back = ((-1, 0), (0, -1)) if connectivity == 4 else ((-1, -1), (-1, 0), (-1, 1), (0, -1))
    for y in range(h):
        for x in range(w):
            if not occ[y, x]:
                continue
            roots = set()
            for dy, dx in back:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < w and occ[yy, xx]:
                    roots.add(_find(parent, prov[yy, xx]))
            if not roots:
                parent.append(len(parent))
                prov[y, x] = len(parent) - 1
            else:
                m = min(roots)
                prov[y, x] = m
                for r in roots:
                    parent[r] = m
    labels = np.zeros((h, w), np.int32)
    number = {}
    for y in range(h):                               # second pass: number the roots in raster order of first appearance
        for x in range(w):
            if occ[y, x]:
                r = _find(parent, prov[y, x])
                if r not in number:
                    number[r] = len(number) + 1
                labels[y, x] = number[r]
    return labels, len(number)


@functools.lru_cache(maxsize=None)
def _label_cached(data, h, w, connectivity):
    occ = np.frombuffer(data, np.uint8).reshape(h, w).astype(bool)
    labels, k = _label_one(occ, connectivity)
    labels.setflags(write=False)
    return labels, k


def label(occ, connectivity):
    """occ bool [H][W] or [N][H][W] -> (labels int32 of the same shape, count int or int32 [N])."""
    assert connectivity in (4, 8)
    occ = np.asarray(occ, bool)
    if occ.ndim == 2:
        return _label_cached(occ.astype(np.uint8).tobytes(), occ.shape[0], occ.shape[1], connectivity)
    out = [label(o, connectivity) for o in occ]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def kernel_merge_label(occ, connectivity):
    """The labelling with the SEEDS and the MERGES csrc/segeval.hip issues, in any order (here: raster): every pixel
    points at the first pixel of its row run; pixel (y, x) merges with the pixel above unless its left neighbour and the
    pixel above left are both occluded, and (8) with an occluded diagonal only where the pixel above is clean -- above
    left only when the left neighbour is clean too.  The root of a component is its smallest index.  Shows that the rule
    leaves no adjacency out."""
    occ = np.asarray(occ, bool)
    h, w = occ.shape
    parent = np.arange(h * w)
    for y in range(h):
        for x in range(w):
            if occ[y, x] and x > 0 and occ[y, x - 1]:
                parent[y * w + x] = parent[y * w + x - 1]

    def unite(a, b):
        a, b = _find(parent, a), _find(parent, b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for y in range(1, h):
        for x in range(w):
            if not occ[y, x]:
                continue
            i = y * w + x
            u = occ[y - 1, x]
            l = x > 0 and occ[y, x - 1]
            ul = x > 0 and occ[y - 1, x - 1]
            ur = x < w - 1 and occ[y - 1, x + 1]
            if u and not (l and ul):
                unite(i, i - w)
            if connectivity == 8 and not u:
                if ul and not l:
                    unite(i, i - w - 1)
                if ur:
                    unite(i, i - w + 1)
    labels = np.zeros(h * w, np.int32)
    roots = [i for i in range(h * w) if occ.flat[i] and _find(parent, i) == i]
    rank = {r: k + 1 for k, r in enumerate(roots)}
    for i in range(h * w):
        if occ.flat[i]:
            labels[i] = rank[_find(parent, i)]
    return labels.reshape(h, w), len(roots)


def blob_table(labels, count, b_occ, cap):
    """labels int32 [N][H][W], count [N], b_occ bool [N][H][W] -> int32 [N][cap][6] rows (area, hit, x0, y0, x1, y1)."""
    labels, b_occ = np.asarray(labels), np.asarray(b_occ, bool)
    n = labels.shape[0]
    table = np.zeros((n, cap, 6), np.int32)
    for i in range(n):
        rows = min(int(count[i]), cap)
        if rows == 0:
            continue
        lab = labels[i]
        sel = (lab >= 1) & (lab <= rows)
        ys, xs = np.nonzero(sel)
        k = lab[sel] - 1
        table[i, :rows, 0] = np.bincount(k, minlength=rows)
        table[i, :rows, 1] = np.bincount(k, weights=b_occ[i][sel], minlength=rows).astype(np.int32)
        for col, v, fn in ((2, xs, np.minimum), (3, ys, np.minimum), (4, xs, np.maximum), (5, ys, np.maximum)):
            acc = np.full(rows, 1 << 30 if fn is np.minimum else -1, np.int64)
            fn.at(acc, k, v)
            table[i, :rows, col] = acc
    return table


def blob_detection(pred_occ, gt_occ, tau=0.5, min_area=1, connectivity=8, cap=64, skip_overflow=False):
    """The dict of segeval.blob_detection; skip_overflow: an image with more than `cap` components in either mask is left
    out and counted in "n_overflow" (the rule of verification.segmentation_sweep) instead of raising."""
    pred_occ, gt_occ = np.asarray(pred_occ, bool), np.asarray(gt_occ, bool)
    lg, cg = label(gt_occ, connectivity)
    lp, cp = label(pred_occ, connectivity)
    over = (cg > cap) | (cp > cap)
    if over.any() and not skip_overflow:
        raise RuntimeError("image %d overflows" % int(np.flatnonzero(over)[0]))
    out = {}
    for name, labels, count, b in (("gt", lg, cg, pred_occ), ("pred", lp, cp, gt_occ)):
        t = blob_table(labels, count, b, cap).astype(np.int64)[~over]
        area, hit = t[:, :, 0], t[:, :, 1]
        big = (area >= min_area) & (area > 0)
        found = hit.astype(np.float64) >= np.float64(tau) * area.astype(np.float64)
        out[name] = (int(big.sum()), int((big & found).sum()), int((big & ~found).sum()))
    n_gt, n_found, n_pred, n_false = out["gt"][0], out["gt"][1], out["pred"][0], out["pred"][2]
    d = {"n_gt": n_gt, "n_found": n_found, "n_pred": n_pred, "n_false": n_false,
         "detection_rate": _div(n_found, n_gt), "false_alarm_rate": _div(n_false, n_pred)}
    if skip_overflow:
        d["n_overflow"] = int(over.sum())
    return d


def pair_masks(desc, oh, ow, protocol="BB", index0=0):
    """desc int32 [2n][>= 5] (kind, x0, y0, w, h) or None -> uint8 [2n][oh][ow], 0 inside the block."""
    if desc is None:
        raise ValueError("no descriptors: the caller knows the number of rows")
    out = np.ones((len(desc), oh, ow), np.uint8)
    for row, d in enumerate(desc):
        g = index0 + row // 2
        if int(d[0]) != 3 or (protocol == "NB" and g % 2):
            continue
        x0, y0, bw, bh = (int(v) for v in d[1:5])
        out[row, max(y0, 0):max(y0 + bh, 0), max(x0, 0):max(x0 + bw, 0)] = 0
    return out


# ---------------------------------------------------------------------------------------------- patterns
def serpentine(h, w):
    """Every even row, joined to the next at alternating ends: one path through the whole plane."""
    occ = np.zeros((h, w), bool)
    occ[0::2] = True
    for k, y in enumerate(range(1, h, 2)):
        occ[y, w - 1 if k % 2 == 0 else 0] = True
    return occ


def rings(h, w):
    y, x = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(y, h - 1 - y), np.minimum(x, w - 1 - x))
    return d % 2 == 0


def patterns(h, w):
    """name -> occ bool [h][w]: the patterns of the issue that make sense at this size."""
    p = {"clean": np.zeros((h, w), bool), "occluded": np.ones((h, w), bool)}
    c = np.zeros((h, w), bool)
    c[0, 0] = c[0, w - 1] = c[h - 1, 0] = c[h - 1, w - 1] = True
    p["corners"] = c
    y, x = np.mgrid[0:h, 0:w]
    p["checker"] = (y + x) % 2 == 0
    p["serpentine"] = serpentine(h, w)
    if h >= 2 and w >= 2:
        t = np.zeros((h, w), bool)
        t[:h // 2, :w // 2] = True
        t[h // 2:, w // 2:] = True
        p["corner_touch"] = t
    if h >= 5 and w >= 5:
        p["rings"] = rings(h, w)
        u = np.zeros((h, w), bool)
        u[:, 0] = u[:, w - 1] = u[h - 1, :] = True
        p["u"] = u
        comb = np.zeros((h, w), bool)
        comb[:, 0::2] = True
        comb[h - 1, :] = True
        comb[h - 2, :] = False
        comb[h - 2, 0::4] = True                       # half of the teeth reach the spine, the others end above it
        p["comb"] = comb
    for d in DENSITIES:
        rng = np.random.default_rng(int(d * 1000) + 17 * h + w)
        p["random%.3f" % d] = rng.random((h, w)) < d
    return p


def pattern_batch(h, w):
    """(names, occ bool [N][h][w]) of patterns(h, w) in a fixed order."""
    p = patterns(h, w)
    names = sorted(p)
    return names, np.stack([p[k] for k in names])


def planted_logits(n, h, w, seed):
    """f32 logits [n][2][h][w] with ties, signed zeros, infinities and NaN planted in either channel."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 2, h, w)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0], np.float32)
    pick = rng.random((n, h, w)) < 0.5
    a = special[rng.integers(0, len(special), (n, h, w))]
    b = special[rng.integers(0, len(special), (n, h, w))]
    x[:, 0][pick] = a[pick]
    x[:, 1][pick] = b[pick]
    tie = rng.random((n, h, w)) < 0.1
    x[:, 1][tie] = x[:, 0][tie]
    return x
