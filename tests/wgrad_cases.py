"""The weight-gradient kernels (msml_conv_wgrad, msml_conv_wgrad_group, msml_conv_wgrad_bnin): the case list, one float64
restatement for every family, the derived error budget and the mutants the checks must catch.  tests/test_wgrad_cpu.py
runs the restatement against torch, every case's plan against the table below and every mutant against its check;
tests/test_gpu_wgrad.py runs the kernels.

    dW[a][boff + b][r][s] = sum over n, p, q of u[n][p][q][a] * v[n][p*stride - pad_h + r][q*stride - pad_w + s][b]
                            a < A, b < Breal; v outside its map = 0

u is NHWC [N][P][Q][up], v NHWC [N][H][W][vp], dW f32 [A][Btot][R][S].  Conv2d: u = dY, v = X; ConvTranspose2d: u = X on
the small grid, v = dY on the large one.  The products of two bf16 values are exact in f32, so a correct kernel's only
error is f32 accumulation.

Exact data: integers, u in [-4, 4], v in [-3, 3] ({-1, 0, 1} for the one case beyond 1.39 M pixels): every partial sum of
every summation order is an integer below 2^24, so every correct kernel gives the f64 result bit for bit.  The pad
channels (a >= A, b >= Breal) hold 7, the dW columns outside [boff, boff + Breal) a sentinel.

Budget on random data (the rule of the BatchNorm and head tests): SAFETY * k * 2^-24 * (sum |u * v| + |dW before|),
SAFETY = 2, k = chain + splits + 2 (+ 1 with accumulate, + 1 for f32 operands, whose products are rounded): `chain` f32
additions inside a workgroup (one per pixel position it walks over, padding positions included, whatever the order inside
an MFMA), `splits` additions in the fixed-order reduce, the slab store and the second-order terms.  chain per family, from
the kernel sources:
  halo      ceil(strips / splits) * 112: wgrad_halo.hip walks a.chunk = cdiv(nstrips, splits) strips (msml_wgrad_halo_launch),
            7 k-steps of 16 pixels each (the `for j < 7` loops of k_wgrad_halo); strips = N * ceil(H / 7) * ceil(W / 14), or
            (N + 1) / 2 image pairs on 7 x 7 maps; a grouped launch has the per-layer splits of its plan.
  im2col    the plan's chunk: k_wgrad_fast walks ceil(chunk / 64) stages of 64 pixels over [k_begin, k_begin + chunk).
  generic   the plan's chunk: k_conv_wgrad, steps of 32 pixels over the same range.
  n32       ceil(strips / splits) * 64: k_wgrad_n32, strips of SR = 4 rows x 16 pixels, strips = N * ceil(P / 4) * ceil(Q / 16).
  line      ceil(tiles / splits) * 224: k_wgrad_line, UBLK = 14 k-steps of 16 pixels per tile, tiles = N * ceil(L / (224 / L)).
  fc        N rounded up to 16: k_fc_wgrad, nsteps = (N + 15) >> 4 k-steps of 16 images, no split-K."""
import collections
import ctypes

import torch

from msml_amd import _lib

U32 = 2.0 ** -24
SAFETY = 2.0
PAD = 7.0                   # what the pad channels of u and v hold
SENTINEL = 4099.0           # what the dW columns outside [boff, boff + Breal) hold (exact in f32)
BF16, F32 = _lib.BF16, _lib.F32
FC, N32, LINE, HALO, FAST, GENERIC = range(1, 7)
WORDS = ("family", "variant", "ba", "bb", "ntw", "splits", "chunk", "direct")

Case = collections.namedtuple(
    "Case", "name path entry dtype group switch up vp A Breal Btot boff N H W P Q R S stride ph pw alpha tri")


def _case(name, path, up, vp, A, Breal, N, H, W, P, Q, R=3, S=3, stride=1, ph=1, pw=1, entry="one", dtype=BF16, group=1,
          switch=None, Btot=None, boff=0, alpha=False, tri=False):
    return Case(name, path, entry, dtype, group, switch, up, vp, A, Breal, Breal if Btot is None else Btot, boff, N, H, W,
                P, Q, R, S, stride, ph, pw, alpha, tri)


def conv(name, path, n, cin, cout, h, w, r=3, s=3, stride=1, ph=1, pw=1, up=None, vp=None, **kw):
    """Conv2d cin -> cout on an h x w input: u = dY [n][P][Q][up], v = X [n][h][w][vp], dW [cout][cin][r][s]."""
    p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
    return _case(name, path, up or cout, vp or cin, cout, cin, n, h, w, p, q, r, s, stride, ph, pw, **kw)


def deconv(name, path, n, cin, cout, p, q, r, stride, pad, up, vp, **kw):
    """ConvTranspose2d cin -> cout from a p x q input: u = X on p x q, v = dY on the large grid, dW [cin][cout][r][r]."""
    h, w = (p - 1) * stride - 2 * pad + r, (q - 1) * stride - 2 * pad + r
    return _case(name, path, up, vp, cin, cout, n, h, w, p, q, r, r, stride, pad, pad, **kw)


def cases():
    """The smallest shapes at which each path can still go wrong (see docs/KERNELS.md, "Weight-gradient kernel tests")."""
    L = [
        # ---- strip / halo kernel, 128-row tiles
        conv("halo128_n17_256", "halo128", 17, 256, 256, 14, 14),      # 34 strips, 32 splits, re-numbered, reduce_rows (1024)
        conv("halo128_n5_128x256", "halo128", 5, 128, 256, 14, 14),    # 10 splits, exactly 512 row blocks
        conv("halo128_n9_128_13x27", "halo128", 9, 128, 128, 13, 27),  # 36 splits, partial strip rows and columns
        conv("halo128_n17_256_g3", "halo128", 17, 256, 256, 14, 14, entry="group", group=3),     # a short split, empty ones
        conv("halo128_n17_256_g8", "halo128", 17, 256, 256, 14, 14, entry="group", group=8),
        conv("halo128_n10_128_21x28_g4", "halo128", 10, 128, 128, 21, 28, entry="group", group=4),
        # ---- 64-row tiles
        conv("halo64_n2_64", "halo64", 2, 64, 64, 14, 14),
        conv("halo64_n3_64x192", "halo64", 3, 64, 192, 14, 14),
        conv("halo64_n12_64_13x27", "halo64", 12, 64, 64, 13, 27),
        conv("halo64_n130_64", "halo64", 130, 64, 64, 14, 14),         # 260 strips over 256 splits
        conv("halo64_n20_64_21x28", "halo64", 20, 64, 64, 21, 28),
        # ---- image-pair strips on 7 x 7 maps
        conv("pair7_n5_64", "pair7", 5, 64, 64, 7, 7),                 # odd N: the last pair has one image
        conv("pair7_n33_64x256", "pair7", 33, 64, 256, 7, 7),
        conv("pair7_n67_256x64", "pair7", 67, 256, 64, 7, 7),
        conv("pair7_n601_64", "pair7", 601, 64, 64, 7, 7),             # 301 strips over 256 splits
        conv("pair7_n1_64_im2col", "im2col", 1, 64, 64, 7, 7),         # the 70 % rule sends it to the im2col kernel
        # ---- BatchNorm(+PReLU) applied in LDS
        conv("bnin_n17_256", "bnin", 17, 256, 256, 14, 14, entry="bnin"),
        conv("bnin_n17_256_prelu", "bnin", 17, 256, 256, 14, 14, entry="bnin", alpha=True),
        conv("bnin_n12_64_13x27", "bnin", 12, 64, 64, 13, 27, entry="bnin"),
        conv("bnin_n12_64_13x27_prelu", "bnin", 12, 64, 64, 13, 27, entry="bnin", alpha=True),
        # ---- im2col kernel
        conv("im2col_direct_n8_64_4x4", "im2col", 8, 64, 64, 4, 4),
        conv("im2col_slabs_n64_64_4x4", "im2col", 64, 64, 64, 4, 4),
        conv("im2col_n64_64_4x4_g2", "im2col", 64, 64, 64, 4, 4, entry="group", group=2),
        conv("im2col_n64_64_4x4_g4", "im2col", 64, 64, 64, 4, 4, entry="group", group=4),       # direct, four dW
        conv("im2col_n64_128_4x4", "im2col", 64, 128, 128, 4, 4),
        conv("im2col_n40_512_4x4", "im2col", 40, 512, 512, 4, 4),
        conv("im2col_n4_64_15x15", "im2col", 4, 64, 64, 15, 15),
        conv("im2col_n4_64_20x30", "im2col", 4, 64, 64, 20, 30),
        conv("im2col_s2_n3_64x128_14", "im2col", 3, 64, 128, 14, 14, stride=2),
        conv("im2col_s2_n3_64x128_9", "im2col", 3, 64, 128, 9, 9, stride=2),                   # odd: P = 5
        conv("im2col_1x1s2_n4_64x128_14", "im2col", 4, 64, 128, 14, 14, 1, 1, 2, 0, 0),
        conv("im2col_stem_n3_3x64_28", "im2col", 3, 3, 64, 28, 28, vp=8),
        conv("im2col_window_n4_18of32_7x7", "im2col", 4, 18, 128, 7, 7, vp=32, Btot=146, boff=128),
        conv("im2col_window_n16_18of32_7x7", "im2col", 16, 18, 128, 7, 7, vp=32, Btot=146, boff=128),   # plain reducer
        conv("im2col_rows_window_n64_4x4", "im2col", 64, 50, 512, 4, 4, vp=64, Btot=96, boff=32),
        conv("im2col_rows_window_s2_n40_9", "im2col", 40, 50, 512, 9, 9, stride=2, vp=64, Btot=96, boff=32),
        conv("im2col_7x1_n2_14x14", "im2col", 2, 64, 18, 14, 14, 7, 1, 1, 3, 0, up=32),
        deconv("im2col_deconv1_n4", "im2col", 4, 8, 18, 4, 4, 3, 2, 1, 8, 32),
        conv("im2col_decode_n3064_8_37x37", "im2col_decode", 3064, 8, 8, 37, 37, tri=True),
        # ---- generic kernel
        conv("generic_f32_n3_64", "generic", 3, 64, 64, 14, 14, dtype=F32),
        conv("generic_f32_s2_n3_128_9", "generic", 3, 128, 128, 9, 9, stride=2, dtype=F32),
        conv("generic_bf16_n64_64_4x4", "generic", 64, 64, 64, 4, 4, switch="MSML_NO_FAST_WGRAD"),
        # ---- narrow-operand kernel
        conv("n32_3x3_n1_14x14", "n32", 1, 18, 18, 14, 14, up=32, vp=32),
        conv("n32_3x3_n2_19x33", "n32", 2, 18, 18, 19, 33, up=32, vp=32),
        conv("n32_3x3_n40_56x56", "n32", 40, 18, 18, 56, 56, up=32, vp=32),                   # 512 splits, the cap
        deconv("n32_deconv4_n3_14x14", "n32", 3, 18, 18, 14, 14, 4, 2, 1, 32, 32),
        deconv("n32_deconv4_n2_15x17", "n32", 2, 18, 18, 15, 17, 4, 2, 1, 32, 32),
        # ---- line kernel
        conv("line_7x1_n1_28_v32", "line", 1, 18, 18, 28, 28, 7, 1, 1, 3, 0, up=32, vp=32),
        conv("line_1x7_n1_28_v64", "line", 1, 64, 18, 28, 28, 1, 7, 1, 0, 3, up=32, vp=64),
        conv("line_7x1_n3_56", "line", 3, 18, 18, 56, 56, 7, 1, 1, 3, 0, up=32, vp=32),
        conv("line_1x7_n70_28", "line", 70, 18, 18, 28, 28, 1, 7, 1, 0, 3, up=32, vp=32),
        conv("line_1x7_n140_28", "line", 140, 18, 18, 28, 28, 1, 7, 1, 0, 3, up=32, vp=32),    # two tiles per workgroup
        # ---- fc kernel
        conv("fc_2x2_n16_32", "fc", 16, 32, 32, 2, 2, 2, 2, 1, 0, 0),
        conv("fc_7x7_n40_window", "fc", 40, 64, 96, 7, 7, 7, 7, 1, 0, 0, Btot=128, boff=64),
        conv("fc_7x7_n17_32", "fc", 17, 32, 32, 7, 7, 7, 7, 1, 0, 0),
        conv("fc_7x7_n15_im2col", "im2col", 15, 32, 32, 7, 7, 7, 7, 1, 0, 0),
    ]
    assert len({c.name for c in L}) == len(L)
    return L


# What msml_conv_wgrad_plan answers for every case on a host with 256 CUs (msml_num_cus() without a device, and on an
# MI355X): family, variant, tile rows, tile columns, taps per workgroup, splits per layer, pixels per split, direct.
PLANS = {
    "halo128_n17_256": (4, 128, 0, 0, 0, 32, 0, 0),
    "halo128_n5_128x256": (4, 128, 0, 0, 0, 10, 0, 0),
    "halo128_n9_128_13x27": (4, 128, 0, 0, 0, 36, 0, 0),
    "halo128_n17_256_g3": (4, 128, 0, 0, 0, 10, 0, 0),
    "halo128_n17_256_g8": (4, 128, 0, 0, 0, 4, 0, 0),
    "halo128_n10_128_21x28_g4": (4, 128, 0, 0, 0, 15, 0, 0),
    "halo64_n2_64": (4, 64, 0, 0, 0, 4, 0, 0),
    "halo64_n3_64x192": (4, 64, 0, 0, 0, 6, 0, 0),
    "halo64_n12_64_13x27": (4, 64, 0, 0, 0, 48, 0, 0),
    "halo64_n130_64": (4, 64, 0, 0, 0, 256, 0, 0),
    "halo64_n20_64_21x28": (4, 64, 0, 0, 0, 120, 0, 0),
    "pair7_n5_64": (4, 7, 0, 0, 0, 3, 0, 0),
    "pair7_n33_64x256": (4, 7, 0, 0, 0, 17, 0, 0),
    "pair7_n67_256x64": (4, 7, 0, 0, 0, 34, 0, 0),
    "pair7_n601_64": (4, 7, 0, 0, 0, 256, 0, 0),
    "pair7_n1_64_im2col": (5, 0, 64, 64, 3, 1, 64, 1),
    "bnin_n17_256": (4, 128, 0, 0, 0, 32, 0, 0),
    "bnin_n17_256_prelu": (4, 128, 0, 0, 0, 32, 0, 0),
    "bnin_n12_64_13x27": (4, 64, 0, 0, 0, 48, 0, 0),
    "bnin_n12_64_13x27_prelu": (4, 64, 0, 0, 0, 48, 0, 0),
    "im2col_direct_n8_64_4x4": (5, 0, 64, 64, 3, 1, 128, 1),
    "im2col_slabs_n64_64_4x4": (5, 0, 64, 64, 3, 4, 256, 0),
    "im2col_n64_64_4x4_g2": (5, 0, 64, 64, 3, 2, 512, 0),
    "im2col_n64_64_4x4_g4": (5, 0, 64, 64, 3, 1, 1024, 1),
    "im2col_n64_128_4x4": (5, 0, 128, 128, 3, 4, 256, 0),
    "im2col_n40_512_4x4": (5, 0, 128, 128, 1, 3, 256, 0),
    "im2col_n4_64_15x15": (5, 0, 64, 64, 3, 4, 256, 0),
    "im2col_n4_64_20x30": (5, 0, 64, 64, 3, 10, 256, 0),
    "im2col_s2_n3_64x128_14": (5, 0, 128, 64, 3, 1, 192, 1),
    "im2col_s2_n3_64x128_9": (5, 0, 128, 64, 3, 1, 128, 1),
    "im2col_1x1s2_n4_64x128_14": (5, 0, 128, 64, 1, 1, 256, 1),
    "im2col_stem_n3_3x64_28": (5, 0, 64, 64, 3, 10, 256, 0),
    "im2col_window_n4_18of32_7x7": (5, 0, 128, 64, 3, 1, 256, 1),
    "im2col_window_n16_18of32_7x7": (5, 0, 128, 64, 3, 4, 256, 0),
    "im2col_rows_window_n64_4x4": (5, 0, 128, 64, 3, 4, 256, 0),
    "im2col_rows_window_s2_n40_9": (5, 0, 128, 64, 3, 4, 256, 0),
    "im2col_7x1_n2_14x14": (5, 0, 64, 64, 3, 2, 256, 0),
    "im2col_deconv1_n4": (5, 0, 64, 64, 3, 1, 64, 1),
    "im2col_decode_n3064_8_37x37": (5, 0, 64, 64, 3, 342, 12288, 0),
    "generic_f32_n3_64": (6, 0, 64, 64, 1, 3, 256, 0),
    "generic_f32_s2_n3_128_9": (6, 0, 128, 128, 1, 1, 128, 0),
    "generic_bf16_n64_64_4x4": (6, 0, 64, 64, 3, 4, 256, 0),
    "n32_3x3_n1_14x14": (2, 0, 0, 0, 0, 4, 0, 0),
    "n32_3x3_n2_19x33": (2, 0, 0, 0, 0, 30, 0, 0),
    "n32_3x3_n40_56x56": (2, 0, 0, 0, 0, 512, 0, 0),
    "n32_deconv4_n3_14x14": (2, 0, 0, 0, 0, 12, 0, 0),
    "n32_deconv4_n2_15x17": (2, 0, 0, 0, 0, 16, 0, 0),
    "line_7x1_n1_28_v32": (3, 0, 0, 0, 0, 4, 0, 0),
    "line_1x7_n1_28_v64": (3, 0, 0, 0, 0, 4, 0, 0),
    "line_7x1_n3_56": (3, 0, 0, 0, 0, 42, 0, 0),
    "line_1x7_n70_28": (3, 0, 0, 0, 0, 280, 0, 0),
    "line_1x7_n140_28": (3, 0, 0, 0, 0, 512, 0, 0),
    "fc_2x2_n16_32": (1, 0, 0, 0, 0, 1, 0, 1),
    "fc_7x7_n40_window": (1, 0, 0, 0, 0, 1, 0, 1),
    "fc_7x7_n17_32": (1, 0, 0, 0, 0, 1, 0, 1),
    "fc_7x7_n15_im2col": (5, 0, 64, 64, 3, 1, 64, 1),
}
REFUSED = conv("bnin_refused_n40_64_27x29", "bnin", 40, 64, 64, 27, 29, entry="bnin")      # MSML_ERR_UNSUPPORTED
GAP = conv("gap_n6_64_56x56", "halo64", 6, 64, 64, 56, 56)     # where the old bound passes faults (test_wgrad_cpu.py only)


def case_id(c):
    return c.name


def find(name):
    return next(c for c in cases() if c.name == name)


def plan(case):
    """(plan words as a dict with slab bytes, status) of the entry point's own shape query: no GPU."""
    words, slab = (ctypes.c_int * 8)(), ctypes.c_long()
    c = case

    def ask():
        return _lib.load().msml_conv_wgrad_plan(c.up, c.vp, c.A, c.Breal, c.Btot, c.boff, c.N, c.H, c.W, c.P, c.Q, c.R, c.S,
                                                c.stride, c.ph, c.pw, c.dtype, c.group, int(c.entry == "bnin"), words,
                                                ctypes.byref(slab))
    if c.switch:
        with _lib.option(c.switch, 1):
            rc = ask()
    else:
        rc = ask()
    return dict(zip(WORDS, words), slab=slab.value), rc


def cdiv(a, b):
    return -(-a // b)


def strips(case, pl):
    """Strips (halo, n32) or tiles (line) the family cuts the pixels into; None for the others."""
    c = case
    if pl["family"] == HALO:
        return (c.N + 1) // 2 if pl["variant"] == 7 else c.N * cdiv(c.H, 7) * cdiv(c.W, 14)
    if pl["family"] == N32:
        return c.N * cdiv(c.P, 4) * cdiv(c.Q, 16)
    if pl["family"] == LINE:
        return c.N * cdiv(c.H, 224 // c.H)
    return None


def chain(case, pl):
    """The largest number of pixel positions one workgroup accumulates into an element (module docstring)."""
    f = pl["family"]
    if f == HALO:
        return cdiv(strips(case, pl), pl["splits"]) * 112
    if f in (FAST, GENERIC):
        return pl["chunk"]
    if f == N32:
        return cdiv(strips(case, pl), pl["splits"]) * 64
    if f == LINE:
        return cdiv(strips(case, pl), pl["splits"]) * 224
    assert f == FC, f
    return cdiv(case.N, 16) * 16


def split_map(case, pl):
    """[N][P][Q] int64: the split-K slab that the u pixel (n, p, q) lands in."""
    c = case
    n = torch.arange(c.N).view(-1, 1, 1)
    p = torch.arange(c.P).view(1, -1, 1)
    q = torch.arange(c.Q).view(1, 1, -1)
    f = pl["family"]
    if f == HALO and pl["variant"] == 7:
        unit = (n // 2).expand(c.N, c.P, c.Q)
    elif f == HALO:
        unit = (n * cdiv(c.H, 7) + p // 7) * cdiv(c.W, 14) + q // 14
    elif f == N32:
        unit = (n * cdiv(c.P, 4) + p // 4) * cdiv(c.Q, 16) + q // 16
    elif f == LINE:
        b = 224 // c.H
        unit = n * cdiv(c.H, b) + (q if c.R == 7 else p) // b + 0 * (p + q)
    elif f in (FAST, GENERIC):
        return ((n * c.P + p) * c.Q + q) // pl["chunk"]
    else:
        return torch.zeros(c.N, c.P, c.Q, dtype=torch.int64)
    return unit // cdiv(strips(c, pl), pl["splits"])


# ------------------------------------------------------------------------------------------------- data
def _seed(case, layer, kind):
    c = case
    seed = 0
    for x in (c.up, c.vp, c.N, c.H, c.W, c.R, c.S, c.stride, layer, ("exact", "random").index(kind)):
        seed = (seed * 1000003 + x) % (2 ** 31 - 1)
    return seed


def tdtype(case):
    return torch.bfloat16 if case.dtype == BF16 else torch.float32


def bn_coefficients(case, kind, layer=0):
    """(scale, shift, alpha or None) f32 [vp] of the bnin cases.  exact: 2, -1 and 0.5 times 1/2, 1 or 2 by channel, so
    that PReLU(v * scale + shift) of an integer v in [-3, 3] is a multiple of 1/8 below 16: exact in bf16."""
    ch = torch.arange(case.vp)
    if kind == "exact":
        scale = 2.0 * 2.0 ** ((ch % 3) - 1).float()
        shift = -1.0 * 2.0 ** ((ch // 3 % 3) - 1).float()
        alpha = 0.5 * 2.0 ** ((ch // 9 % 3) - 1).float()
    else:
        g = torch.Generator().manual_seed(_seed(case, layer, kind) + 1)
        scale = torch.rand(case.vp, generator=g) + 0.5
        shift = torch.randn(case.vp, generator=g) * 0.5
        alpha = torch.rand(case.vp, generator=g) * 0.3
    return scale, shift, (alpha if case.alpha else None)


def bn_apply(v, scale, shift, alpha):
    """bf16(PReLU(v * scale + shift)) in f32 arithmetic: what msml_bn_act_fwd stores (up to an fma on random data)."""
    y = v.float() * scale + shift
    if alpha is not None:
        y = torch.where(y < 0, y * alpha, y)
    return y.bfloat16()


def make_data(case, kind, layer=0):
    """(u [N][P][Q][up], v [N][H][W][vp]) in the storage type, PAD in the pad channels.  kind: "exact" or "random"."""
    c = case
    g = torch.Generator().manual_seed(_seed(c, layer, kind))
    out = []
    for shape, real, lim in (((c.N, c.P, c.Q, c.up), c.A, 4), ((c.N, c.H, c.W, c.vp), c.Breal, 3)):
        t = torch.full(shape, PAD, dtype=torch.float32)
        if kind == "exact":
            lim = 1 if c.tri else lim
            t[..., :real] = torch.randint(-lim, lim + 1, shape[:3] + (real,), generator=g).float()
        else:
            t[..., :real] = torch.randn(shape[:3] + (real,), generator=g)
        out.append(t.to(tdtype(c)))
    return tuple(out)


def operands(case, u, v, coef=None):
    """(u, v) in float64 as the kernel multiplies them: for bnin, v after the BatchNorm(+PReLU) and its bf16 store."""
    if case.entry == "bnin":
        v = bn_apply(v, *coef)
    return u.double(), v.double()


def init_dw(case, accumulate, layer=0):
    """dW before the call: SENTINEL outside the column window; inside it small integers (accumulate) or NaN."""
    c = case
    dw = torch.full((c.A, c.Btot, c.R, c.S), SENTINEL, dtype=torch.float32)
    win = dw[:, c.boff:c.boff + c.Breal]
    if accumulate:
        g = torch.Generator().manual_seed(77 + layer)
        win.copy_(torch.randint(-5, 6, tuple(win.shape), generator=g).float())
    else:
        win.fill_(float("nan"))
    return dw


# ------------------------------------------------------------------------------------------------- the restatement
MUTANTS = {
    # name: (case it must be caught on, the checks that must fail there)
    "last_strip_row_dropped": ("halo128_n17_256", ("exact", "budget")),
    "one_pixel_one_tile_one_tap": ("halo64_n2_64", ("exact", "budget")),
    "halo_from_neighbour_image": ("halo64_n12_64_13x27", ("exact", "budget")),
    "pair_gap_column_read": ("pair7_n5_64", ("exact", "budget")),
    "strip_column_14_dropped": ("halo128_n9_128_13x27", ("exact", "budget")),
    "last_split_left_out": ("halo128_n17_256", ("exact", "budget")),
    "slab_rounded_to_bf16": ("halo64_n2_64", ("budget",)),
    "accumulate_overwrites": ("im2col_slabs_n64_64_4x4", ("exact", "budget")),
    "tap_transposed": ("halo64_n2_64", ("exact", "budget")),
    "boff_ignored": ("im2col_window_n4_18of32_7x7", ("exact", "budget")),
    "pad_channel_folded": ("n32_3x3_n2_19x33", ("exact", "budget")),
    "parity_off_by_one": ("im2col_s2_n3_64x128_9", ("exact", "budget")),
    "batchnorm_applied_to_padding": ("bnin_n12_64_13x27_prelu", ("exact", "budget")),
}
OUTPUT_MUTANTS = ("accumulate_overwrites", "boff_ignored")        # wrong in expected(), not in the sum


def _tap_ranges(c, r, s, shift=0):
    """u rows / columns [p0, p1) x [q0, q1) whose v pixel for tap (r, s) lies inside the map, and that pixel of p0, q0."""
    def rng(n_out, n_in, stride, pad, t):
        ok = [i for i in range(n_out) if 0 <= i * stride - pad + t + shift < n_in]
        if not ok:
            return 0, 0, 0
        assert ok == list(range(ok[0], ok[-1] + 1))
        return ok[0], ok[-1] + 1, ok[0] * stride - pad + t + shift
    return rng(c.P, c.H, c.stride, c.ph, r) + rng(c.Q, c.W, c.stride, c.pw, s)


def tap_matmuls(u, v, c, umask=None, shift=0):
    """One float64 matmul per tap over shifted slices.  umask(r, s): None or a [N or 1][P][Q] factor on u."""
    dw = torch.zeros(c.A, c.Breal, c.R, c.S, dtype=torch.float64)
    for r in range(c.R):
        for s in range(c.S):
            p0, p1, y0, q0, q1, x0 = _tap_ranges(c, r, s, shift)
            if p1 == p0 or q1 == q0:
                continue
            us = u[:, p0:p1, q0:q1, :c.A]
            vs = v[:, y0:y0 + (p1 - p0 - 1) * c.stride + 1:c.stride, x0:x0 + (q1 - q0 - 1) * c.stride + 1:c.stride, :c.Breal]
            m = umask(r, s) if umask is not None else None
            if m is not None:
                us = us * m[:, p0:p1, q0:q1, None]
            dw[:, :, r, s] = us.reshape(-1, c.A).t() @ vs.reshape(-1, c.Breal)
    return dw


def _unchecked(u, v, c):
    """The sum with v addressed as ((n * H + y) * W + x) without the map test: the halo of an image is its neighbours'
    pixels (or the next row's), only addresses outside the tensor are zero."""
    dw = torch.zeros(c.A, c.Breal, c.R, c.S, dtype=torch.float64)
    n = torch.arange(c.N).view(-1, 1, 1)
    p = torch.arange(c.P).view(1, -1, 1)
    q = torch.arange(c.Q).view(1, 1, -1)
    flat = torch.cat([v.reshape(-1, c.vp)[:, :c.Breal], torch.zeros(1, c.Breal, dtype=torch.float64)])
    for r in range(c.R):
        for s in range(c.S):
            idx = (n * c.H + p * c.stride - c.ph + r) * c.W + q * c.stride - c.pw + s
            idx = torch.where((idx < 0) | (idx >= c.N * c.H * c.W), torch.full_like(idx, c.N * c.H * c.W), idx)
            dw[:, :, r, s] = u[..., :c.A].reshape(-1, c.A).t() @ flat[idx.reshape(-1)]
    return dw


def dw_f64(u, v, case, pl=None, mutant=None, absolute=False, coef=None):
    """dW [A][Breal][R][S] float64 from u and v (float64 tensors, operands()); absolute=True: sum |u * v|, the magnitude
    the budget scales with.  mutant: one of MUTANTS (not the OUTPUT_MUTANTS), a wrong kernel; pl: the plan, for the
    mutants that depend on the split partition; coef: the BatchNorm coefficients, for the mutant that needs them."""
    c = case
    if absolute:
        assert mutant is None
        return tap_matmuls(u.abs(), v.abs(), c)
    if mutant is None:
        return tap_matmuls(u, v, c)
    if mutant == "batchnorm_applied_to_padding":         # the zero halo goes through the BatchNorm too: PReLU(shift)
        assert c.entry == "bnin" and c.ph == 1 and c.pw == 1
        edge = bn_apply(torch.zeros(1, 1, 1, c.vp), *coef).double()
        wide = edge.expand(c.N, c.H + 2, c.W + 2, c.vp).clone()
        wide[:, 1:-1, 1:-1] = v
        return tap_matmuls(u, wide, c._replace(H=c.H + 2, W=c.W + 2, ph=0, pw=0))
    p = torch.arange(c.P).view(1, -1, 1)
    q = torch.arange(c.Q).view(1, 1, -1)
    if mutant == "last_strip_row_dropped":               # the seventh k-step of every strip
        return tap_matmuls(u, v, c, lambda r, s: (p % 7 != 6).double().expand(1, c.P, c.Q))
    if mutant == "strip_column_14_dropped":              # halo column 14 = u column (q % 14) read at column shift s
        return tap_matmuls(u, v, c, lambda r, s: ((q % 14) + s != 14).double().expand(1, c.P, c.Q))
    if mutant == "last_split_left_out":                  # the last slab that holds pixels never reaches the reduce
        sm = split_map(c, pl)
        return tap_matmuls(u, v, c, lambda r, s: (sm != sm.max()).double())
    if mutant == "slab_rounded_to_bf16":                 # slab 0 is stored as bf16
        sm = split_map(c, pl)
        part = tap_matmuls(u, v, c, lambda r, s: (sm == 0).double())
        return tap_matmuls(u, v, c) - part + part.bfloat16().double()
    if mutant == "one_pixel_one_tile_one_tap":           # image 0, the centre pixel, rows 32-63 x columns 0-31, tap (1, 2)
        dw = tap_matmuls(u, v, c)
        py, px, r, s = c.P // 2, c.Q // 2, 1, 2
        y, x = py * c.stride - c.ph + r, px * c.stride - c.pw + s
        dw[32:64, 0:32, r, s] -= torch.outer(u[0, py, px, 32:64], v[0, y, x, 0:32])
        return dw
    if mutant == "halo_from_neighbour_image":
        return _unchecked(u, v, c)
    if mutant == "pair_gap_column_read":                 # 7 x 7 image pairs A | gap | B: the gap column is not zero --
        assert c.H == 7 and c.W == 7 and c.R == 3        # A's right padding reads B's first column, B's left A's last
        dw = tap_matmuls(u, v, c)
        npair = c.N // 2
        for r in range(3):
            p0, p1, y0, _, _, _ = _tap_ranges(c, r, 1)
            ua, ub = u[0:2 * npair:2, p0:p1, 6, :c.A], u[1:2 * npair:2, p0:p1, 0, :c.A]
            va, vb = v[0:2 * npair:2, y0:y0 + p1 - p0, 6, :c.Breal], v[1:2 * npair:2, y0:y0 + p1 - p0, 0, :c.Breal]
            dw[:, :, r, 2] += ua.reshape(-1, c.A).t() @ vb.reshape(-1, c.Breal)
            dw[:, :, r, 0] += ub.reshape(-1, c.A).t() @ va.reshape(-1, c.Breal)
        return dw
    if mutant == "tap_transposed":
        assert c.R == c.S
        return tap_matmuls(u, v, c).transpose(2, 3).contiguous()
    if mutant == "pad_channel_folded":                   # the pad channels of u are summed into its channel 0
        assert c.up > c.A
        u = u.clone()
        u[..., 0] += u[..., c.A:].sum(-1)
        return tap_matmuls(u, v, c)
    if mutant == "parity_off_by_one":
        assert c.stride == 2
        return tap_matmuls(u, v, c, shift=1)
    raise KeyError(mutant)


def expected(case, dw, init, accumulate, mutant=None):
    """The whole dW tensor [A][Btot][R][S] in float64 after the call, from the sum `dw` and the tensor before it."""
    c = case
    out = init.double().clone()
    off = 0 if mutant == "boff_ignored" else c.boff
    if accumulate and mutant != "accumulate_overwrites":
        out[:, off:off + c.Breal] = init[:, c.boff:c.boff + c.Breal].double() + dw
    else:
        out[:, off:off + c.Breal] = dw
    return out


def kfactor(case, pl, accumulate):
    return chain(case, pl) + pl["splits"] + 2 + (1 if accumulate else 0) + (1 if case.dtype == F32 else 0)


def budget(case, pl, mag, init, accumulate):
    """[A][Btot][R][S] float64: the error allowed per element; 0 outside the column window (the sentinel must survive)."""
    c = case
    b = torch.zeros(c.A, c.Btot, c.R, c.S, dtype=torch.float64)
    terms = mag + (init[:, c.boff:c.boff + c.Breal].double().abs() if accumulate else 0.0)
    b[:, c.boff:c.boff + c.Breal] = SAFETY * kfactor(c, pl, accumulate) * U32 * terms
    return b


def worst_ratio(got, want, bud):
    """max |got - want| / budget over the elements (an element with a zero budget must be exact; NaN counts as inf)."""
    err = (got.double() - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = torch.where(bud > 0, err / torch.where(bud > 0, bud, torch.ones_like(bud)),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


def exact_headroom(case, mag, quantum=1.0):
    """Largest sum |u * v| in units of the data's quantum: below 2^24 every partial sum of every order is exact in f32."""
    return float(mag.max()) / quantum


# ------------------------------------------------------------------------------------------------- shared references
_REF = {}


def reference(case, kind, layer=0, v_operand=None):
    """(u, v, coef, dW f64, sum |u v| f64) of one layer, computed once per (shape, kind, layer) and shared by every test
    (and by the cases of one shape: layer i of a group has the data of layer i of every other group of that shape).
    v_operand: the bf16 tensor the device's msml_bn_act_fwd made of v (bnin on random data), used instead of bn_apply."""
    c = case
    key = (c.entry == "bnin", c.alpha, c.dtype, c.tri) + tuple(c[6:22]) + (kind, layer, v_operand is not None)
    if key not in _REF:
        u, v = make_data(c, kind, layer)
        coef = bn_coefficients(c, kind, layer) if c.entry == "bnin" else None
        u64, v64 = operands(c, u, v, coef) if v_operand is None else (u.double(), v_operand.double())
        _REF[key] = (u, v, coef, dw_f64(u64, v64, c), dw_f64(u64, v64, c, absolute=True))
    return _REF[key]
