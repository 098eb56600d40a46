"""Pillow's resampling coefficients for one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc), built on the
host in double precision: the one restatement the product keeps.  `data.resample_table` (csrc/occ.hip) and
`mtcnn_align.resample_rows` (csrc/imgops.hip) lay the result out as their kernels read it."""
import numpy as np


def _bicubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * -0.5, 0.0))


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}       # Resample.c: filter, support


def pillow_coeffs(insz, outsz, filter):
    """(xmin [outsz], cnt [outsz], fixed [outsz][cnt.max()]) as int64: first tap, taps and the weights in 22-bit fixed
    point (zero behind the taps) of every output position.  Pillow's order of operations: support scaled by
    max(scale, 1), window int(center -+ support + 0.5) clamped to the axis, the filter's argument times ss = 1 / that
    factor, the weights summed tap after tap and divided by the sum, then int(+-0.5 + k 2^22).  No identity shortcut:
    equal lengths give what the formulas give.  An unknown filter name is a KeyError."""
    kernel, support = FILTERS[filter]
    scale = insz / outsz
    fscale = max(scale, 1.0)
    support = support * fscale
    ss = 1.0 / fscale
    center = (np.arange(outsz) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)        # C's (int): truncation
    cnt = np.minimum((center + support + 0.5).astype(np.int64), insz) - xmin
    j = np.arange(int(cnt.max()))
    live = j[None, :] < cnt[:, None]
    w = np.where(live, kernel((j[None, :] + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(outsz)
    for k in j:                                                            # ww += w, tap after tap as the C loop
        ww = ww + w[:, k]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    fixed = np.where(w < 0, -0.5 + w * (1 << 22), 0.5 + w * (1 << 22)).astype(np.int64)      # (int): truncation
    return xmin, cnt, np.where(live, fixed, 0)
