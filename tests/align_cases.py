"""Shared by tests/test_align_cpu.py, tests/test_gpu_align.py and tools/bench_align.py: an independent numpy restatement
(integers and f64, no import of msml_amd.ijb) of the face alignment in front of the template evaluation --
Embedding.get / forward_db of eval/qeval_ijbc.py:145-192 -- and the seeded synthetic cases the tests run on.

* `umeyama(src, dst)`          skimage's _umeyama with scale for ONE point set (a loop over images is the caller's)
* `closed_form(src, dst)`      the closed-form 2-D similarity fit (complex least squares), a second opinion on it
* `invert(m)`                  cv2.warpAffine's inversion of the 2 x 3 matrix, in its order of operations
* `warp(img, minv, oh, ow)`    OpenCV's classic warpAffine + remap (INTER_LINEAR, BORDER_CONSTANT 0) in integers
* `warp_exact(img, minv, ...)`  exact f64 bilinear interpolation of the same samples at the real-valued position
* `pairs(faces, desc)`         block occlusion + mirror + the three f32 normalisation steps

No OpenCV / skimage build was available when this was written: `warp` restates the arithmetic from OpenCV's source
(imgwarp.cpp: AB_BITS 10, INTER_BITS 5, INTER_REMAP_COEF_BITS 15) and has not been compared with cv2's output.
"""
import numpy as np

DST112 = np.array([[30.2946, 51.6963], [65.5318, 51.5014], [48.0252, 71.7366], [33.5493, 92.3655],
                   [62.7299, 92.2041]], dtype=np.float32)
DST112[:, 0] += 8.0                                  # qeval_ijbc.py:96, in float32 as the script does it
SIZES = ((37, 53), (112, 112), (250, 250), (480, 640), (1, 1), (9, 300))      # (H, W) of the sources


def reduce68(lm):
    """qeval_ijbc.py:149-155 for one [68][2] set."""
    lm = np.asarray(lm)
    out = np.zeros((5, 2), lm.dtype)
    out[0] = (lm[36] + lm[39]) / 2
    out[1] = (lm[42] + lm[45]) / 2
    out[2], out[3], out[4] = lm[30], lm[48], lm[54]
    return out


def umeyama(src, dst):
    """skimage.transform._geometric._umeyama(src, dst, estimate_scale=True) in f64 -> the 3 x 3 matrix (NaN at rank 0)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    num, dim = src.shape
    src_mean, dst_mean = src.mean(axis=0), dst.mean(axis=0)
    src_demean, dst_demean = src - src_mean, dst - dst_mean
    A = dst_demean.T @ src_demean / num
    d = np.ones((dim,), dtype=np.float64)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    T = np.eye(dim + 1, dtype=np.float64)
    U, S, V = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        return np.nan * T
    elif rank == dim - 1:
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            T[:dim, :dim] = U @ V
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ V
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ V
    scale = 1.0 / src_demean.var(axis=0).sum() * (S @ d)
    T[:dim, dim] = dst_mean - scale * (T[:dim, :dim] @ src_mean.T)
    T[:dim, :dim] *= scale
    return T


def closed_form(src, dst):
    """Least-squares 2-D similarity src -> dst without reflection: with centred points as complex numbers s, d,
    a + ib = sum conj(s) d / sum |s|^2, i.e. a = sum s.d / sum |s|^2, b = sum s x d / sum |s|^2; t = mean_d - R mean_s."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    s, d = src - ms, dst - md
    den = (s * s).sum()
    a = (s * d).sum() / den
    b = (s[:, 0] * d[:, 1] - s[:, 1] * d[:, 0]).sum() / den
    R = np.array([[a, -b], [b, a]])
    return np.concatenate([R, (md - R @ ms)[:, None]], 1)


def random_landmarks(rng, n, size=(112, 112), noise=1.5):
    """n float32 landmark sets: the destination points under a random inverse similarity (scale 0.25-3, rotation
    +-0.7 rad, placed about the middle of an H x W source) plus noise.  Returns (landmarks [n][5][2] f32, and the exact
    forward matrices [n][2][3] that map the noise-free landmarks onto the destination)."""
    h, w = size
    lms, mats = [], []
    for _ in range(n):
        sc, th = rng.uniform(0.25, 3.0), rng.uniform(-0.7, 0.7)
        c, s = np.cos(th), np.sin(th)
        R = sc * np.array([[c, -s], [s, c]])                           # forward: src -> dst
        centre = np.array([w / 2.0, h / 2.0]) + rng.uniform(-0.15, 0.15, 2) * np.array([w, h])
        t = np.array([56.0, 72.0]) - R @ centre                        # the source centre lands mid-face
        src = (np.linalg.inv(R) @ (DST112.astype(np.float64) - t).T).T
        lms.append((src + noise / sc * rng.standard_normal((5, 2))).astype(np.float32))
        mats.append(np.concatenate([R, t[:, None]], 1))
    return np.stack(lms), np.stack(mats)


def invert(m):
    """cv2.warpAffine without WARP_INVERSE_MAP: the 2 x 3 forward matrix -> the 6 inverse coefficients."""
    M = [float(v) for v in np.asarray(m, np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return np.array(M, np.float64)


def _sat_int(v):
    """round half to even, clamp to int32 in f64, convert (NaN -> INT_MIN)."""
    v = np.rint(np.asarray(v, np.float64))
    lo, hi = -2147483648.0, 2147483647.0
    with np.errstate(invalid="ignore"):
        v = np.where(~(v >= lo), lo, np.where(v > hi, hi, v))
    return v.astype(np.int64)


def _wrap32(v):
    """int64 -> the value a 32-bit two's-complement register holds."""
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def warp(img, minv, out_h, out_w, swap_rb=True):
    """img: H x W x 3 uint8 (any strides), minv: 6 inverse coefficients -> out_h x out_w x 3 uint8."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    m = [np.float64(v) for v in np.asarray(minv, np.float64).reshape(6)]
    x = np.arange(out_w, dtype=np.float64)
    y = np.arange(out_h, dtype=np.float64)
    adelta = _sat_int(m[0] * x * 1024.0)
    bdelta = _sat_int(m[3] * x * 1024.0)
    X0 = _wrap32(_sat_int((m[1] * y + m[2]) * 1024.0) + 16)
    Y0 = _wrap32(_sat_int((m[4] * y + m[5]) * 1024.0) + 16)
    X = _wrap32(X0[:, None] + adelta[None, :]) >> 5
    Y = _wrap32(Y0[:, None] + bdelta[None, :]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    acc = np.zeros((out_h, out_w, 3), np.int64)
    for dy, dx, wgt in ((0, 0, (32 - fx) * (32 - fy) * 32), (0, 1, fx * (32 - fy) * 32),
                        (1, 0, (32 - fx) * fy * 32), (1, 1, fx * fy * 32)):
        tx, ty = sx + dx, sy + dy
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        px = img[np.where(inside, ty, 0), np.where(inside, tx, 0)].astype(np.int64)
        acc += np.where(inside[..., None], px, 0) * wgt[..., None]
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out[..., ::-1].copy() if swap_rb else out


def source_positions(minv, out_h, out_w):
    """The real-valued source position (xs, ys) of every output pixel."""
    m = np.asarray(minv, np.float64).reshape(6)
    x, y = np.meshgrid(np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64))
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


def warp_exact(img, minv, out_h, out_w):
    """Exact bilinear interpolation in f64 of the H x W x 3 uint8 image at the real-valued source position (taps outside
    the image count 0), not rounded."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    xs, ys = source_positions(minv, out_h, out_w)
    x0, y0 = np.floor(xs), np.floor(ys)
    ax, ay = (xs - x0)[..., None], (ys - y0)[..., None]
    out = np.zeros((out_h, out_w, 3))
    for dy, dx, wgt in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
        tx, ty = x0 + dx, y0 + dy
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        px = img[np.where(inside, ty, 0).astype(np.int64), np.where(inside, tx, 0).astype(np.int64)].astype(np.float64)
        out += np.where(inside[..., None], px, 0.0) * wgt
    return out


def smooth(x, y, c):
    return 127.5 + 60.0 * np.sin(x * (0.05 + 0.01 * c) + c) + 60.0 * np.cos(y * (0.04 + 0.01 * c) - c)


def smooth_image(H, W):
    """The smooth test image rounded to uint8, H x W x 3."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return np.stack([np.rint(smooth(x, y, c)) for c in range(3)], -1).astype(np.uint8)


def pack(images, pitch_extra=0):
    """Independent of msml_amd.ijb.pack_images: (flat uint8 array, meta [N][4] int64); rows padded by pitch_extra."""
    meta, chunks, off = [], [], 0
    for im in images:
        h, w = im.shape[:2]
        pitch = 3 * w + pitch_extra
        rows = np.full((h, pitch), 0xA5, np.uint8)               # the padding is never read: any value
        rows[:, :3 * w] = im.reshape(h, 3 * w)
        size = (h * pitch + 3) & ~3
        chunks.append(np.concatenate([rows.reshape(-1), np.full(size - h * pitch, 0x5A, np.uint8)]))
        meta.append((off, h, w, pitch))
        off += size
    return np.concatenate(chunks), np.asarray(meta, np.int64)


def pairs(faces, desc=None):
    """faces [N][H][W][3] uint8, desc [N][64] int32 or None (kind 0 / 3; words 1-4 = x0, y0, w, h painted black) ->
    [2N][3][H][W] f32: row 2i = forward_db's div_(255).sub_(0.5).div_(0.5) in float32, row 2i + 1 its mirror."""
    f = np.array(faces, np.uint8)
    n = f.shape[0]
    if desc is not None:
        for i in range(n):
            kind, x0, y0, w, h = (int(v) for v in desc[i, :5])
            assert kind in (0, 3)
            if kind == 3:
                f[i, max(y0, 0):max(y0 + h, 0), max(x0, 0):max(x0 + w, 0)] = 0
    v = f.astype(np.float32)
    v = v / np.float32(255.0)
    v = v - np.float32(0.5)
    v = v / np.float32(0.5)
    v = v.transpose(0, 3, 1, 2)
    out = np.empty((2 * n,) + v.shape[1:], np.float32)
    out[0::2] = v
    out[1::2] = v[..., ::-1]
    return out
