"""MTCNN face alignment on the device: the reference's own crops, for a batch of photos of any sizes.

The reference never calls MTCNN.detect_faces on its own; it calls four methods of the class (eval/preprocess/mtcnn.py):
align (:25-39), align_multi (:84-104), align_fully (:41-82) and get_landmarks (:106-158).  All four end in
warp_and_crop_face (mtcnn_pytorch/src/align_trans.py:218-329): the five detected points are fitted to a template by
get_similarity_transform_for_cv2 (matlab_cp2tform.py) and the photo is warped by cv2.warpAffine.  Here:

  host, numpy f64   reference_points (the template), similarity_matrices (the fit), the orientation maps
  device            detect.Detector.detect_faces, img_resize / img_orient (csrc/imgops.hip: the shrunken and turned copies
                    align_fully and get_landmarks detect on), ijb.align_faces (msml_align_warp: one launch for all faces)

Deliberately as the reference:
  * warp_and_crop_face ignores its `mode` argument; so there is none here.
  * Its default align_type is the misspelt 'smilarity', which selects the similarity branch; the 'affine' and
    'cv2_affine' branches are not built.
  * findSimilarity mirrors the template IN PLACE (its xyR is xy itself), so both residuals it compares are distances to
    the MIRRORED template.  similarity_matrices does the same; for a plain face the plain fit still wins, for a mirrored
    one the mirrored fit.
  * A crop other than 96 x 112 scales both axes of the template by w / 112, also when it is not square.
  * align_fully's `while len(candi) > 1` never runs (the loop over `ori` stops at the first face): not built.
  * get_landmarks divides the landmarks by the scale of its shrunken copy but NOT the boxes: kept.
Deliberately not:
  * An image without a face gives zero-length entries / found = False where the reference returns None.
  * Landmarks that all coincide raise ValueError; the reference inverts a singular matrix there and returns numbers
    of the order of 1e15.
  * With the numpy this was written against (2.2) numpy.linalg.lstsq returns the four parameters in float64 (its
    matrix X is float64 because np.ones is), so nothing is rounded to float32 between the float32 points and the
    returned matrices; the fit here is the closed form of the same least-squares problem in float64.
Out of scope: paste_back, norm_crop and the other templates of eval/preprocess/alignment.py, PIPNet, FaceBoxes, RealOcc.
"""
import functools

import numpy as np
import torch

from . import _lib, detect, ijb, packed
from ._lib import call
from .resample import pillow_coeffs

BILINEAR, BICUBIC = 2, 3                                  # PIL.Image's filter numbers
FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, ROTATE_90, ROTATE_180, ROTATE_270 = range(5)

_FIVE_POINTS = ((30.29459953, 51.69630051), (65.53179932, 51.50139999), (48.02519989, 71.73660278),
                (33.54930115, 92.3655014), (62.72990036, 92.20410156))      # align_trans.py:15-21, for a 96 x 112 crop


# ---------------------------------------------------------------------------------------------------------------------
# host: the template and the fit

def reference_points(crop_size=(112, 112), square=True):
    """The float32 [5][2] points warp_and_crop_face ends up fitting to for crop_size = (w, h).
    get_reference_facial_points(default_square=square) (align_trans.py:86-103) in float64: the 96 x 112 points, moved by
    (8, 0) when square.  Then the shrink of :277-284 in float32: (96, 112) is shrunk by 0.85 about (48, 56); any other
    size by 0.85 about (56, 56) and then scaled by w / 112 on BOTH axes."""
    w, h = int(crop_size[0]), int(crop_size[1])
    pts = np.array(_FIVE_POINTS, np.float64)
    if square:
        pts = pts + np.array([8.0, 0.0])
    ref = pts.astype(np.float32)
    f = np.float32
    if w == 96 and h == 112:
        ref[:, 0] = (ref[:, 0] - f(48.0)) * f(0.85) + f(48.0)
        ref[:, 1] = (ref[:, 1] - f(56.0)) * f(0.85) + f(56.0)
    else:
        ref = (ref - f(56.0)) * f(0.85) + f(56.0)
        ref = ref * f(w / 112.)
    return ref


def _rank_ok(p):
    """matrix_rank(X) >= 4 for the [2K][4] matrix findNonreflectiveSimilarity builds from the points p [N][K][2].  X'X
    has the eigenvalues of [[sum x^2 + y^2, |sum (x, y)|], [|sum (x, y)|, K]], each twice, so the singular values come in
    closed form; the tolerance is numpy's: the largest times max(2K, 4) eps."""
    k = p.shape[1]
    s = (p * p).sum((1, 2))
    c = p - p.mean(1, keepdims=True)
    det = k * (c * c).sum((1, 2))                                  # S K - |sum|^2, without the cancellation
    big = 0.5 * (s + k + np.sqrt((s - k) ** 2 + 4.0 * (s * k - det)))
    small = det / big
    return np.sqrt(small) > np.sqrt(big) * (max(2 * k, 4) * np.finfo(np.float64).eps)


def _nonreflective(uv, xy):
    """findNonreflectiveSimilarity for uv [N][K][2] and xy [K][2] in f64: (T [N][3][3], Tinv [N][3][3]) with
    [u v 1] = [x y 1] Tinv.  The least-squares solution of its system X r = U in closed form: with centred points,
    sc = sum (x u + y v) / sum (x^2 + y^2), ss = sum (y u - x v) / the same, t = mean(u, v) - the rotated mean(x, y)."""
    n = uv.shape[0]
    mxy, muv = xy.mean(0), uv.mean(1)
    x, y = xy[:, 0] - mxy[0], xy[:, 1] - mxy[1]
    u, v = uv[:, :, 0] - muv[:, 0:1], uv[:, :, 1] - muv[:, 1:2]
    den = (x * x + y * y).sum()
    sc = (x * u + y * v).sum(1) / den
    ss = (y * u - x * v).sum(1) / den
    tx = muv[:, 0] - sc * mxy[0] - ss * mxy[1]
    ty = muv[:, 1] + ss * mxy[0] - sc * mxy[1]
    tinv = np.zeros((n, 3, 3))
    tinv[:, 0, 0], tinv[:, 0, 1], tinv[:, 1, 0], tinv[:, 1, 1] = sc, -ss, ss, sc
    tinv[:, 2, 0], tinv[:, 2, 1], tinv[:, 2, 2] = tx, ty, 1.0
    d = sc * sc + ss * ss
    t = np.zeros((n, 3, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = sc / d, ss / d
    t[:, 0, 0], t[:, 0, 1], t[:, 1, 0], t[:, 1, 1] = a, b, -b, a
    t[:, 2, 0], t[:, 2, 1], t[:, 2, 2] = -(tx * a - ty * b), -(tx * b + ty * a), 1.0
    return t, tinv


def _forward(t, uv):
    return np.matmul(uv, t[:, 0:2, 0:2]) + t[:, 2:3, 0:2]


def similarity_matrices(points, ref, reflective=True):
    """get_similarity_transform_for_cv2(points[i], ref, reflective) (matlab_cp2tform.py) for every row:
    (tfm [N][2][3], tfm_inv [N][2][3]) float64; tfm maps the photo onto the crop, which is what cv2.warpAffine takes.
    points [N][5][2] (or [5][2]) and ref [5][2] are rounded to float32 first, as warp_and_crop_face does; everything
    after that is float64.  reflective: findSimilarity -- the plain fit against the fit to the mirrored template
    composed with TreflectY, the plain one when norm1 <= norm2, both norms taken against the mirrored template as the
    reference takes them; tfm_inv is then the fit's own inverse map for the plain fit and inv(trans2) for the mirrored.
    ValueError naming the row: for a template with fewer than two distinct points (the reference's rank test, :89,
    'cp2tform:twoUniquePointsReq'), for landmarks that all coincide (module docstring) and for non-finite points."""
    uv = np.asarray(points, np.float32)
    if uv.ndim == 2:
        uv = uv[None]
    xy = np.asarray(ref, np.float32)
    if uv.ndim != 3 or uv.shape[0] == 0 or uv.shape[2] != 2 or xy.shape != uv.shape[1:]:
        raise ValueError("similarity_matrices: points %s and ref %s are not [N][K][2] and [K][2]"
                         % (tuple(uv.shape), tuple(xy.shape)))
    uv, xy = uv.astype(np.float64), xy.astype(np.float64)
    if not np.isfinite(xy).all():
        raise ValueError("similarity_matrices: the template is not finite")
    bad = np.flatnonzero(~np.isfinite(uv).all((1, 2)))
    if bad.size:
        raise ValueError("similarity_matrices: points of row %d are not finite" % bad[0])
    if not _rank_ok(xy[None])[0]:
        raise ValueError("similarity_matrices: row 0: the template has fewer than two distinct points "
                         "(cp2tform:twoUniquePointsReq)")
    bad = np.flatnonzero(~_rank_ok(uv))
    if bad.size:
        raise ValueError("similarity_matrices: points of row %d coincide: no similarity transform" % bad[0])
    t1, t1inv = _nonreflective(uv, xy)
    if reflective:
        xyr = xy * np.array([-1.0, 1.0])
        t2 = _nonreflective(uv, xyr)[0]
        t2[:, :, 0] = -t2[:, :, 0]                                 # trans2r . TreflectY
        norm1 = np.sqrt(((_forward(t1, uv) - xyr) ** 2).sum((1, 2)))
        norm2 = np.sqrt(((_forward(t2, uv) - xyr) ** 2).sum((1, 2)))
        second = ~(norm1 <= norm2)
        if second.any():
            t1[second], t1inv[second] = t2[second], np.linalg.inv(t2[second])
    tfm = np.ascontiguousarray(t1[:, :, 0:2].transpose(0, 2, 1))
    inv = np.ascontiguousarray(t1inv[:, :, 0:2].transpose(0, 2, 1))
    if not (np.isfinite(tfm).all() and np.isfinite(inv).all()):
        bad = np.flatnonzero(~(np.isfinite(tfm).all((1, 2)) & np.isfinite(inv).all((1, 2))))
        raise ValueError("similarity_matrices: the transform of row %d is not finite" % bad[0])
    return tfm, inv


def five_points(landmarks):
    """[n][10] landmark rows x0..x4 y0..y4 -> [n][5][2] (x, y) points, float32."""
    lm = np.asarray(landmarks, np.float32).reshape(-1, 10)
    return np.stack([lm[:, 0:5], lm[:, 5:10]], 2)


def map_points(landmarks, i, w, h):
    """mtcnn.py:60-67: landmark rows [n][10] found in the copy transposed by method i + 1 (i = 0: not transposed) ->
    [n][5][2] float32 points in the w x h photo, with the reference's float32 arithmetic: i = 1 (w - 1 - y, x),
    i = 2 (w - 1 - x, h - 1 - y), i = 3 (y, h - 1 - x)."""
    lm = np.asarray(landmarks, np.float32).reshape(-1, 10)
    x, y = lm[:, 0:5], lm[:, 5:10]
    wm, hm = np.float32(w - 1), np.float32(h - 1)
    if i == 0:
        out = (x, y)
    elif i == 1:
        out = (wm - y, x)
    elif i == 2:
        out = (wm - x, hm - y)
    elif i == 3:
        out = (y, hm - x)
    else:
        raise ValueError("map_points: orientation %r is not 0..3" % (i,))
    return np.stack(out, 2).astype(np.float32)


def map_boxes(boxes, i, w, h):
    """mtcnn.py:129-147: boxes [n][5] of the copy transposed by method i + 1 -> a mapped copy, float64.  As there, the
    corners are swapped so that x1 <= x2 and y1 <= y2 stay, and w, h are those of the ORIGINAL photo although the boxes
    are in the coordinates of the shrunken copy."""
    b = np.array(boxes, np.float64).reshape(-1, 5)
    if i == 1:
        b[:, :4] = np.stack((w - 1 - b[:, 3], b[:, 0], w - 1 - b[:, 1], b[:, 2]), 1)
    elif i == 2:
        b[:, :4] = np.stack((w - 1 - b[:, 2], h - 1 - b[:, 3], w - 1 - b[:, 0], h - 1 - b[:, 1]), 1)
    elif i == 3:
        b[:, :4] = np.stack((b[:, 1], h - 1 - b[:, 2], b[:, 3], h - 1 - b[:, 0]), 1)
    elif i != 0:
        raise ValueError("map_boxes: orientation %r is not 0..3" % (i,))
    return b


# ---------------------------------------------------------------------------------------------------------------------
# device: packed images, Image.transpose, Image.resize

_FILTERS = {BILINEAR: "bilinear", BICUBIC: "bicubic"}                      # resample.FILTERS' names


@functools.lru_cache(maxsize=256)
def resample_rows(insz, outsz, filter=BICUBIC):
    """Pillow's coefficients for one axis (resample.pillow_coeffs) as msml_img_resize reads them: int32
    [outsz][2 + ksize] = first tap, taps, coefficients in 22-bit fixed point (zero behind the taps).  Equal lengths
    give the identity (one tap of 2^22): Pillow skips that pass, which is a copy."""
    insz, outsz = int(insz), int(outsz)
    if insz == outsz:
        tab = np.zeros((outsz, 3), np.int32)
        tab[:, 0], tab[:, 1], tab[:, 2] = np.arange(outsz), 1, 1 << 22
        return tab
    xmin, cnt, fixed = pillow_coeffs(insz, outsz, _FILTERS[filter])
    tab = np.zeros((outsz, 2 + fixed.shape[1]), np.int32)
    tab[:, 0], tab[:, 1], tab[:, 2:] = xmin, cnt, fixed
    return tab


def _packed(images):
    return packed.sources(images, "mtcnn_align")


def _up(buf, device="cuda"):
    return buf if buf.is_cuda else buf.to(device, non_blocking=True)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@torch.no_grad()
def img_orient(images, methods):
    """Image.transpose(methods[n]) of every packed image in one launch (msml_img_orient): 0 FLIP_LEFT_RIGHT,
    1 FLIP_TOP_BOTTOM, 2 ROTATE_90, 3 ROTATE_180, 4 ROTATE_270.  images: a list of RGB uint8 arrays or (buf, meta).
    Returns (buf on the device, meta numpy [N][4]) packed the same way with rows of a multiple of 4 bytes: what
    Detector.detect_faces and the functions of this module take."""
    buf, mt = _packed(images)
    n = mt.shape[0]
    m = np.asarray(methods).reshape(-1)
    if m.shape[0] != n or not np.issubdtype(m.dtype, np.integer):
        raise ValueError("img_orient: %d integer methods for %d images" % (m.shape[0], n))
    if ((m < 0) | (m > 4)).any():
        raise ValueError("img_orient: method %d is not one of 0..4" % m[(m < 0) | (m > 4)][0])
    turn = (m == ROTATE_90) | (m == ROTATE_270)
    meta_out, total = packed.layout(np.where(turn, mt[:, 2], mt[:, 1]), np.where(turn, mt[:, 1], mt[:, 2]))
    plan = np.ascontiguousarray(np.stack([m.astype(np.int64), meta_out[:, 1], meta_out[:, 2]], 1))
    buf = _up(buf)
    out = torch.empty(total, dtype=torch.uint8, device=buf.device)
    call("msml_img_orient", buf, buf.numel(), _dev(mt, buf.device), _dev(m.astype(np.int32), buf.device), out,
         _dev(meta_out, buf.device), plan.ctypes.data, n)
    return out, meta_out


@torch.no_grad()
def img_resize(images, sizes, filter=BICUBIC):
    """Image.resize(sizes[n], filter) of every packed image in one call (msml_img_resize, two launches): sizes [N][2] =
    (out_w, out_h) as PIL takes them (or one pair for all), filter 2 = BILINEAR or 3 = BICUBIC -- what img.resize(size)
    means for an RGB image since Pillow 7.  Bit for bit Pillow's two passes.  The coefficient tables are built on the
    host once per distinct (in, out) length (resample_rows) and cached.  Returns (buf on the device, meta numpy [N][4])."""
    if filter not in _FILTERS:
        raise ValueError("img_resize: filter %r is neither 2 (bilinear) nor 3 (bicubic)" % (filter,))
    buf, mt = _packed(images)
    n = mt.shape[0]
    sz = np.asarray(sizes)
    if not np.issubdtype(sz.dtype, np.integer):
        raise ValueError("img_resize: sizes must be integers")
    sz = np.broadcast_to(sz.reshape(-1, 2), (n, 2)) if sz.size == 2 else sz.reshape(-1, 2)
    if sz.shape[0] != n:
        raise ValueError("img_resize: %d sizes for %d images" % (sz.shape[0], n))
    ow, oh = sz[:, 0].astype(np.int64), sz[:, 1].astype(np.int64)
    if ((ow < 1) | (ow > 32767) | (oh < 1) | (oh > 32767)).any():
        raise ValueError("img_resize: an output size is outside 1..32767")
    meta_out, total = packed.layout(oh, ow)
    hostsz = np.ascontiguousarray(np.stack([mt[:, 1], mt[:, 2], oh, ow], 1))
    ws_bytes = _lib.value("msml_img_resize_workspace", hostsz.ctypes.data, n)
    if ws_bytes <= 0:
        raise RuntimeError("img_resize: msml_img_resize_workspace refused the sizes")
    # one table per distinct (in, out) length, horizontal and vertical alike
    where, parts, used = {}, [], 0
    jobs = np.zeros((n, 5), np.int64)
    inter = mt[:, 1] * meta_out[:, 3]
    jobs[:, 4] = np.cumsum(inter) - inter
    for i in range(n):
        for col, key in ((0, (int(mt[i, 2]), int(ow[i]))), (2, (int(mt[i, 1]), int(oh[i])))):
            if key not in where:
                tab = resample_rows(key[0], key[1], filter)
                where[key] = (used, tab.shape[1] - 2)
                parts.append(tab.reshape(-1))
                used += tab.size
            jobs[i, col], jobs[i, col + 1] = where[key]
    buf = _up(buf)
    dev = buf.device
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    call("msml_img_resize", buf, _dev(mt, dev), out, _dev(meta_out, dev), _dev(np.concatenate(parts), dev),
         _dev(jobs, dev), hostsz.ctypes.data, n, int(filter), ws, ws_bytes)
    return out, meta_out


def unpack(buf, meta):
    """The packed images as a list of H x W x 3 uint8 numpy arrays (one device-to-host copy)."""
    flat = buf.cpu().numpy()
    return [np.lib.stride_tricks.as_strided(flat[o:], (h, w, 3), (p, 3, 1)).copy() for o, h, w, p in np.asarray(meta)]


# ---------------------------------------------------------------------------------------------------------------------
# the four methods, batched

def _crop_hw(crop_size):
    w, h = int(crop_size[0]), int(crop_size[1])
    if not (4 <= w <= 256 and 4 <= h <= 256 and w % 4 == 0):
        raise ValueError("mtcnn_align: crop_size (w, h) = (%d, %d) is outside msml_align_warp's 4..256 with w %% 4 == 0"
                         % (w, h))
    return h, w


def _warp(buf, mt, owner, points, crop_size, square):
    """warp_and_crop_face for points [F][5][2] of the photos owner [F]: (crops uint8 [F][h][w][3] on the device,
    tfm_inv [F][2][3]).  One msml_align_warp launch with one meta row per FACE; rows of the same photo repeat it."""
    h, w = _crop_hw(crop_size)
    tfm, inv = similarity_matrices(points, reference_points(crop_size, square))
    return ijb.align_faces(buf, mt[owner], tfm, (h, w), bgr=False), inv


@torch.no_grad()
def align_multi(detector, images, limit=None, min_face_size=64.0, crop_size=(112, 112), thresholds=(0.6, 0.7, 0.8),
                factor=0.707, square=True):
    """MTCNN.align_multi(img, limit, min_face_size, crop_size, thresholds, factor, reverse=True) for every image: one
    detect_faces call for the batch, the fit of every face on the host, one warp launch for all faces.  images: a list
    of RGB uint8 arrays of any sizes, or (buf, meta).  Returns (crops, tfm_inv, boxes), each a list with one entry per
    image: crops uint8 [n][h][w][3] on the device in the detector's order (descending score), tfm_inv f64 [n][2][3],
    boxes f64 [n][5].  An image without a face gives entries of length 0; the reference returns None there.  limit cuts
    the list after the detection (:88-90).  crop_size = (w, h)."""
    h, w = _crop_hw(crop_size)
    buf, mt = _packed(images)
    buf = _up(buf, detector.device)
    det = detector.detect_faces((buf, mt), min_face_size, thresholds, factor=factor)
    boxes, marks = det.boxes, det.landmarks
    if limit:
        boxes, marks = [b[:limit] for b in boxes], [m[:limit] for m in marks]
    counts = np.array([len(m) for m in marks], np.int64)
    total = int(counts.sum())
    if total == 0:
        empty = torch.zeros(0, h, w, 3, dtype=torch.uint8, device=buf.device)
        return [empty for _ in counts], [np.zeros((0, 2, 3)) for _ in counts], boxes
    owner = np.repeat(np.arange(len(counts)), counts)
    crops, inv = _warp(buf, mt, owner, five_points(np.concatenate(marks)), crop_size, square)
    cuts = np.cumsum(counts)[:-1]
    return list(torch.tensor_split(crops, [int(c) for c in cuts])), np.split(inv, cuts), boxes


@torch.no_grad()
def align(detector, images, crop_size=(112, 112), square=True):
    """MTCNN.align(img, crop_size, return_trans_inv=True) for every image: the first face (the highest score) of each.
    Returns (crops uint8 [B][h][w][3] on the device, zeros where nothing was found; found [B] bool; tfm_inv f64
    [B][2][3], zeros where nothing was found)."""
    h, w = _crop_hw(crop_size)
    buf, mt = _packed(images)
    buf = _up(buf, detector.device)
    det = detector.detect_faces((buf, mt))
    points, found = detect.first_landmarks(det.landmarks)
    crops, inv = _scatter(buf, mt, np.flatnonzero(found), points[found], crop_size, square)
    return crops, found, inv


def _scatter(buf, mt, idx, points, crop_size, square):
    """Crops and tfm_inv of the photos idx, scattered into [B] rows of zeros."""
    h, w = _crop_hw(crop_size)
    crops = torch.zeros(mt.shape[0], h, w, 3, dtype=torch.uint8, device=buf.device)
    inv = np.zeros((mt.shape[0], 2, 3))
    if idx.size:
        c, inv[idx] = _warp(buf, mt, idx, points, crop_size, square)
        crops[torch.from_numpy(idx).to(buf.device)] = c
    return crops, inv


def _shrunken(buf, mt, sw):
    """img.resize((int(w * scale), int(h * scale))) with scale = sw / w of every image (sw None: the image's own width,
    scale 1, a copy that is not made): ((buf, meta) of the copies, scale [B] as Python floats)."""
    if sw is None:
        return (buf, mt), [int(w) / int(w) for w in mt[:, 2]]
    scale = [sw / int(w) for w in mt[:, 2]]
    sizes = np.array([(int(int(w) * s), int(int(h) * s)) for (h, w), s in zip(mt[:, 1:3], scale)], np.int64)
    if (sizes < 1).any():
        raise ValueError("mtcnn_align: image %d shrinks to nothing at width %g" % (np.flatnonzero((sizes < 1).any(1))[0], sw))
    return img_resize((buf, mt), sizes, BICUBIC), scale


def _oriented(small, idx, i):
    """The copies of the images idx transposed by method i + 1 (i = 0: the copies themselves, no launch)."""
    sbuf, smt = small
    if i == 0:
        return sbuf, smt[idx]
    if i not in (1, 2, 3):
        raise ValueError("mtcnn_align: orientation %r is not 0..3" % (i,))
    return img_orient((sbuf, smt[idx]), np.full(idx.size, i + 1, np.int64))


def _detect(detector, copies, min_face_sizes, thresholds):
    """ONE detect_faces call on the copies, each with its own min_face_size (sw / 10 or sw / 20: the same for every
    image in fast mode, a function of the image's width otherwise)."""
    det = detector.detect_faces(copies, np.asarray(min_face_sizes, np.float64), thresholds)
    return det.boxes, det.landmarks


@torch.no_grad()
def align_fully(detector, images, crop_size=(112, 112), ori=(0, 1, 3), fast_mode=True, thresholds=(0.6, 0.7, 0.7),
                square=True):
    """MTCNN.align_fully(img, crop_size, return_trans_inv=True, ori, fast_mode) for every image, by rounds: all images
    are shrunk to width 320 (fast_mode; else kept) with the bicubic filter in one call; round k turns the copies of the
    images still without a face by ori[k] (transpose method ori[k] + 1, none for 0) in one launch and runs ONE detector
    call on them with min_face_size = sw / 10 per image (without fast_mode sw is each image's own width): at most
    len(ori) detector calls per batch.  The first face's landmarks are divided by the scale (float32, as there), mapped
    back to the original photo (map_points) and the ORIGINAL photo is warped.  Returns (crops uint8 [B][h][w][3] on the
    device, zeros where nothing was found; found [B]; orientation [B], the ori value that found the face, -1 where none
    did; tfm_inv f64 [B][2][3]; score f64 [B] = box[0][4], 0 where nothing was found)."""
    buf, mt = _packed(images)
    buf = _up(buf, detector.device)
    n = mt.shape[0]
    small, scale = _shrunken(buf, mt, 320. if fast_mode else None)
    mfs = np.array([(320. if fast_mode else int(w)) / 10 for w in mt[:, 2]])
    orientation = np.full(n, -1, np.int64)
    score = np.zeros(n)
    points = np.zeros((n, 5, 2), np.float32)
    for i in ori:
        idx = np.flatnonzero(orientation < 0)
        if idx.size == 0:
            break
        boxes, marks = _detect(detector, _oriented(small, idx, i), mfs[idx], thresholds)
        for k, j in enumerate(idx):
            if len(marks[k]):
                lm = marks[k][0:1] / np.float32(scale[j])
                points[j] = map_points(lm, i, int(mt[j, 2]), int(mt[j, 1]))[0]
                orientation[j], score[j] = i, boxes[k][0][4]
    found = orientation >= 0
    crops, inv = _scatter(buf, mt, np.flatnonzero(found), points[found], crop_size, square)
    return crops, found, orientation, inv, score


@torch.no_grad()
def get_landmarks(detector, images, min_face_size=32, crop_size=(256, 256), fast_mode=False, ori=(0, 1, 3),
                  square=True):
    """MTCNN.get_landmarks for every image: every orientation of `ori`, with no early stop, one round per orientation as
    align_fully makes them; thresholds 0.6 / 0.7 / 0.7; in fast mode the copies are 640 wide and min_face_size is 32
    (640 / 20).  Returns (faces, boxes): faces[b] = [(crop uint8 [h][w][3] on the device, five points f32 [5][2] in the
    original photo)], one per orientation that found a face, in ori order; boxes[b] f64 [m][5] = every box of those
    orientations mapped back as mtcnn.py:129-147 do and concatenated (which the reference builds and drops).  As
    there, the landmarks are divided by the scale of the shrunken copy and the boxes are NOT."""
    buf, mt = _packed(images)
    buf = _up(buf, detector.device)
    n = mt.shape[0]
    small, scale = _shrunken(buf, mt, 640. if fast_mode else None)
    mfs = np.full(n, 640. / 20 if fast_mode else min_face_size, np.float64)
    owner, points, boxes = [], [], [np.zeros((0, 5)) for _ in range(n)]
    idx = np.arange(n)
    for i in ori:
        bxs, marks = _detect(detector, _oriented(small, idx, i), mfs, (0.6, 0.7, 0.7))
        for j in idx:
            if len(marks[j]):
                w, h = int(mt[j, 2]), int(mt[j, 1])
                owner.append((j, len(owner)))
                points.append(map_points(marks[j][0:1] / np.float32(scale[j]), i, w, h)[0])
                boxes[j] = np.concatenate((boxes[j], map_boxes(bxs[j], i, w, h)), 0)
    faces = [[] for _ in range(n)]
    if owner:
        own = np.array([j for j, _ in owner], np.int64)
        pts = np.stack(points)
        crops, _ = _warp(buf, mt, own, pts, crop_size, square)
        for j, k in sorted(owner):                                  # per image, in ori order
            faces[j].append((crops[k], pts[k]))
    return faces, boxes


@torch.no_grad()
def align_and_embed(model, detector, images, which="multi", batch=64, **kw):
    """Photos in, embeddings out: the crops of align_multi ("multi": every face), align ("first") or align_fully
    ("fully"), then ijb.pair_inputs(crops, None) and the model, `batch` crops per forward.  Returns (feats [F][2E] f32 on
    the device, embedding | embedding of the mirrored crop, or None when F = 0; owner [F] int64, the image of every row;
    found [B] bool).  kw goes to the method chosen."""
    if which == "multi":
        crops, _, _ = align_multi(detector, images, **kw)
        counts = np.array([c.shape[0] for c in crops], np.int64)
        owner, found = np.repeat(np.arange(len(crops)), counts), counts > 0
        faces = torch.cat(crops) if counts.sum() else None
    elif which in ("first", "fully"):
        res = align(detector, images, **kw) if which == "first" else align_fully(detector, images, **kw)
        found = res[1]
        owner = np.flatnonzero(found)
        faces = res[0][torch.from_numpy(owner).to(res[0].device)].contiguous() if owner.size else None
    else:
        raise ValueError("align_and_embed: which=%r is not 'multi', 'first' or 'fully'" % (which,))
    if faces is None:
        return None, owner, found
    batch = max(1, int(batch))
    out = None
    for i0 in range(0, faces.shape[0], batch):
        part = faces[i0:i0 + batch]
        f = model(ijb.pair_inputs(part, None))
        if isinstance(f, (tuple, list)):
            f = f[0]
        f = f.float().reshape(part.shape[0], -1)
        if out is None:
            out = torch.empty(faces.shape[0], f.shape[1], dtype=torch.float32, device=f.device)
        out[i0:i0 + part.shape[0]] = f
    return out, owner, found
