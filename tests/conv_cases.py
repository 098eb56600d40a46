"""The conv forward and backward-data kernels (msml_conv2d, msml_conv2d_acc, msml_conv2d_fused, msml_conv2d_bnbwd[_acc],
msml_conv2d_bnin[_acc], msml_deconv4_bwd_data): the case list, one float64 restatement of the formula in
include/msml_hip.h, the data generators, the derived error budget and the mutants the checks must catch.
tests/test_conv_cpu.py runs the restatement against torch, every case's route against the table below and every mutant
against its check; tests/test_gpu_conv_exact.py runs the kernels.

    out[n,oy,ox,ko] = bias[ko] + sum_seg sum_{r,s,c} in_seg[n,iy,ix,c] * w[ko][seg,r,s,c]
    transposed == 0: iy = oy*stride - pad_h + r
    transposed == 1: iy = (oy + pad_h - r)/stride when divisible

Epilogues, as the kernels apply them (every kernel of every family, read from the sources):
  msml_conv2d[_acc]   v = acc + bias; out = round(v); statistics = per-channel (sum v, sum v^2) of the f32 value v BEFORE it
                      is rounded to the storage type -- in row mode and in accumulator mode alike (STATDEF below).
  msml_conv2d_fused   z = acc*scale + shift; PReLU here unless a residual joins first (res_first); z is ROUNDED TO bf16
                      where a residual joins (the residual is added to the value as stored, in the copy-out layout of
                      every kernel: the order of the conv -> BatchNorm -> add chain the entry point replaces); then
                      + residual, PReLU if res_first, and the final rounding.
  msml_conv2d_bnbwd   out = bf16(acc); the three sums from the stored bf16 out (BnBwdFuse / bnb_accum of csrc/common.h):
                      neg = alpha given and z <= 0, g = neg ? dy*alpha : dy, q0 = sum g, q1 = sum g*xhat,
                      q2 = sum (neg ? dy*z : 0); z = x*scale + shift, xhat = x*invstd - mean*invstd.
  msml_conv2d_bnin    the conv of X = bf16(PReLU(in*scale + shift)), zero padding applied to X.

Exact data: bf16-representable integers with sum |x w| <= 256 for every output element, so every partial sum of every
summation order is an integer f32 holds and the stored bf16 is that integer: x in [-amp, amp] (amp 3, or 1 where the
statistics need it), w in {-1, 0, 1} with at most 85 nonzeros per reduction row (dense where K * amp <= 256), every
(r, s, c) position nonzero in some row and every tap in every row.  Input pad channels hold 7, output pad channels must
come out 0.  Epilogue values: scale in {+-0.5, +-1, +-2}, shift / bias / residual quarter-integers, alpha in {0.25, 0.5}.

Budget on random data: B = SAFETY * k * 2^-24 * sum |x w| on the accumulator, SAFETY = 2, k = R*S*(c0p + c1p) (+ 1 for
f32 operands) + one per epilogue operation; through the epilogue by |scale| and max(1, |alpha|); a stored value passes
within B + half an ulp of its type at |ref| + B (+ half a bf16 ulp of the value a residual joins).  Statistics: the sum of
the elements' budgets + SAFETY * pixels * 2^-24 * sum |terms|."""
import collections
import contextlib

import torch

from msml_amd import _lib

U32 = 2.0 ** -24
SAFETY = 2.0
PAD = 7.0                     # what the pad channels of every input hold
CUS = 256                     # msml_num_cus() on an MI355X and without a device
BF16, F32 = _lib.BF16, _lib.F32
BB, BF, FF = (BF16, BF16), (BF16, F32), (F32, F32)
STATDEF = "f32"               # the one definition every kernel follows: sums of the f32 value before the store
UNSUPPORTED = "MSML_ERR_UNSUPPORTED"

Case = collections.namedtuple(
    "Case", "name family entry dtype switch c0 c0p c1 c1p cout coutp N H W P Q R S stride ph pw tr "
            "bias scale alpha res res_first stats statdef amp kernel inst")


def cdiv(a, b):
    return -(-a // b)


def cpad(c):
    return cdiv(c, 32) * 32


def mk(name, family, kernel, inst, n, c0, cout, h, w, r=3, s=3, stride=1, ph=None, pw=None, tr=0, c1=0, entry="conv2d",
       dtype=BB, switch=None, c0p=None, c1p=None, coutp=None, bias=0, scale=0, alpha=0, res=0, res_first=0, stats=None,
       amp=3, opad=0):
    """One case.  kernel: the prefix msml_conv2d_kernel answers for the shape; inst: the instantiation the dispatch
    source launches for this call (route() restates the conditions).  transposed: P = (H - 1)*stride - 2*pad + R + opad."""
    ph = r // 2 if ph is None else ph
    pw = s // 2 if pw is None else pw
    if tr:
        p, q = (h - 1) * stride - 2 * ph + r + opad, (w - 1) * stride - 2 * pw + s + opad
    else:
        p, q = (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1
    if entry in ("conv2d_acc", "bnin_acc"):
        stats = "acc"
    return Case(name, family, entry, dtype, switch, c0, c0p or cpad(c0), c1, (c1p or cpad(c1)) if c1 else 0, cout,
                coutp or cpad(cout), n, h, w, p, q, r, s, stride, ph, pw, tr, bias, scale, alpha, res, res_first, stats,
                STATDEF, amp, kernel, inst)


WS, S2R, HALO, HALOP, H2, FAST, IGEMM = ("k_conv_ws", "k_conv_s2r", "k_conv_halo<", "k_conv_halo_p", "k_conv_halo2",
                                         "k_conv_fast", "k_conv_igemm")
LINE, D4 = "k_conv_line", "k_deconv4_fwd"


def cases():
    """The smallest shapes at which each path can still go wrong (docs/KERNELS.md, "Conv forward and backward-data kernel
    tests").  The comment of a case is the condition it sits on."""
    L = []
    add = lambda *a, **k: L.append(mk(*a, **k))
    # ---- k_conv_ws / k_conv_s2r<0>: 64 -> 64, 3x3, stride 1.  conv_fast.hip:603 tries k_conv_s2r first (stride 1, no bnb);
    # conv_s2r.hip:608-611 refuses bias / scale / alpha / residual / row-mode statistics / bnb at stride 1 -> k_conv_ws
    add("ws_n1_14_plain", "ws", WS, "k_conv_s2r<0, false>", 1, 64, 64, 14, 14)                           # one tile
    add("ws_n2_13x27_plain", "ws", WS, "k_conv_s2r<0, false>", 2, 64, 64, 13, 27)                        # partial rows and columns; 70 %: 7020 >= 6272
    add("ws_n2_13x27_acc", "ws", S2R, "k_conv_s2r<0, false>", 2, 64, 64, 13, 27, entry="conv2d_acc")     # (the query: k_conv_ws refuses 4 tiles > 3 rows)
    add("ws_n2_13x27_tr", "ws", WS, "k_conv_s2r<0, false>", 2, 64, 64, 13, 27, tr=1)                     # flipped taps
    add("ws_n2_13x27_bias", "ws", WS, "k_conv_ws<false>", 2, 64, 64, 13, 27, bias=1)
    add("ws_n2_13x27_fused", "ws", WS, "k_conv_ws<false>", 2, 64, 64, 13, 27, entry="fused", scale=1, alpha=1, res=1)
    add("ws_n2_13x27_fused_rf", "ws", WS, "k_conv_ws<false>", 2, 64, 64, 13, 27, entry="fused", scale=1, alpha=1, res=1, res_first=1)
    add("ws_n2_13x27_fused_tr", "ws", WS, "k_conv_ws<false>", 2, 64, 64, 13, 27, entry="fused", scale=1, tr=1)
    # row-mode statistics: conv_ws.hip:471 refuses more workgroups than rows (4 tiles > ceil(702 / 256) = 3): a 13 x 27 map
    # never has as many rows as tiles, the im2col kernel takes it -- a route edge
    add("ws_n2_13x27_rows", "ws", S2R, "k_conv_fast<bf16, 256 x 64>", 2, 64, 64, 13, 27, stats="rows")
    add("ws_n1_28_rows", "ws", WS, "k_conv_ws<false>", 1, 64, 64, 28, 28, stats="rows")                  # 4 tiles = ceil(784 / 256) rows
    add("ws_n3_14_rows_bias", "ws", WS, "k_conv_ws<false>", 3, 64, 64, 14, 14, stats="rows", bias=1)     # 3 tiles = ceil(588 / 256) rows
    add("ws_n2_13x27_bnbwd", "ws", WS, "k_conv_ws<true>", 2, 64, 64, 13, 27, tr=1, entry="bnbwd", alpha=1)
    add("ws_n2_13x27_bnbwd_acc", "ws", WS, "k_conv_ws<true>", 2, 64, 64, 13, 27, tr=1, entry="bnbwd_acc")
    add("ws_n17_56_plain", "ws", WS, "k_conv_s2r<0, false>", 17, 64, 64, 56, 56)                          # 272 tiles over 256 workgroups
    add("ws_n17_56_bias", "ws", WS, "k_conv_ws<false>", 17, 64, 64, 56, 56, bias=1)
    add("ws_n17_56_bnbwd_acc", "ws", WS, "k_conv_ws<true>", 17, 64, 64, 56, 56, tr=1, entry="bnbwd_acc", alpha=1, amp=1)
    # ---- k_conv_s2r stride 2 (conv_s2r.hip:578-581: even maps, the 70 % rule on the GEMM grid)
    add("s2r_fwd_n5_28", "s2r", S2R, "k_conv_s2r<1, false>", 5, 64, 64, 28, 28, stride=2)
    add("s2r_fwd_n4_26_acc", "s2r", S2R, "k_conv_s2r<1, false>", 4, 64, 64, 26, 26, stride=2, entry="conv2d_acc")   # 13 x 13 grid
    add("s2r_fwd_n65_56_acc", "s2r", S2R, "k_conv_s2r<1, false>", 65, 64, 64, 56, 56, stride=2, entry="conv2d_acc", amp=1)   # 260 tiles
    add("s2r_fwd_n5_28_rows", "s2r", S2R, "k_conv_fast<bf16, 256 x 64>", 5, 64, 64, 28, 28, stride=2, stats="rows")        # conv_s2r.hip:610
    add("s2r_bwd_n5_14", "s2r", S2R, "k_conv_s2r<2, false>", 5, 64, 64, 14, 14, stride=2, tr=1, opad=1)
    add("s2r_bwd_n5_14_bnbwd_acc", "s2r", S2R, "k_conv_s2r<2, true>", 5, 64, 64, 14, 14, stride=2, tr=1, opad=1, entry="bnbwd_acc", alpha=1)
    add("s2r_bwd_n65_28", "s2r", S2R, "k_conv_s2r<2, false>", 65, 64, 64, 28, 28, stride=2, tr=1, opad=1, amp=1)              # 260 tiles
    add("s2r_bwd_n65_28_bnbwd_acc", "s2r", S2R, "k_conv_s2r<2, true>", 65, 64, 64, 28, 28, stride=2, tr=1, opad=1, entry="bnbwd_acc", amp=1)
    # ---- k_conv_r32: 32 -> 32, 3x3, W in [8, 62], H >= 2 (conv_r32.hip:294-300); the name query does not know it
    for tr in (0, 1):
        t = "_tr" if tr else ""
        F = "true" if tr else "false"
        add("r32_n2_9x13_plain" + t, "r32", FAST, "k_conv_r32<PLAIN, %s>" % F, 2, 32, 32, 9, 13, tr=tr)
        add("r32_n2_9x13_acc" + t, "r32", FAST, "k_conv_r32<STATS, %s>" % F, 2, 32, 32, 9, 13, tr=tr, entry="conv2d_acc")
        add("r32_n2_9x13_bnbwd_acc" + t, "r32", FAST, "k_conv_r32<BNB, %s>" % F, 2, 32, 32, 9, 13, tr=tr, entry="bnbwd_acc", alpha=1)
    add("r32_n1_2x8_plain", "r32", FAST, "k_conv_r32<PLAIN, false>", 1, 32, 32, 2, 8)                     # H = 2, W = 8: the lower edges
    add("r32_n1_60x62_plain", "r32", FAST, "k_conv_r32<PLAIN, false>", 1, 32, 32, 60, 62)                # rows of 62: 68 KB of LDS
    add("r32_n1_60x62_acc_tr", "r32", FAST, "k_conv_r32<STATS, true>", 1, 32, 32, 60, 62, tr=1, entry="conv2d_acc")
    add("r32_n1030_8_plain", "r32", FAST, "k_conv_r32<PLAIN, false>", 1030, 18, 18, 8, 8)                 # strips of 7 rows, 2060 units, grid 512
    add("r32_n1030_8_bnbwd_acc", "r32", FAST, "k_conv_r32<BNB, false>", 1030, 18, 18, 8, 8, entry="bnbwd_acc", alpha=1, amp=1)
    add("r32_n2_9x13_rows", "r32", FAST, "k_conv_fast<bf16, 256 x 32>", 2, 32, 32, 9, 13, stats="rows")     # conv_r32.hip:298
    add("r32_n2_9x63_plain", "r32", FAST, "k_conv_fast<bf16, 256 x 32>", 2, 32, 32, 9, 63)                  # W = 63: past the upper edge
    # ---- k_conv_pw: 1x1, stride 1 (conv_pw.hip:337, 358-363), M = 105 = 7 x 15: no multiple of 32
    add("pw_32x64_plain", "pw", FAST, "k_conv_pw<32, 64, PLAIN, false>", 1, 32, 64, 7, 15, 1, 1)
    add("pw_64x32_aff", "pw", FAST, "k_conv_pw<64, 32, PLAIN, true>", 1, 64, 32, 7, 15, 1, 1, entry="fused", scale=1)
    add("pw_64x64_plain", "pw", FAST, "k_conv_pw<64, 64, PLAIN, false>", 1, 64, 64, 7, 15, 1, 1)
    add("pw_64x64_bias", "pw", FAST, "k_conv_pw<64, 64, PLAIN, true>", 1, 64, 64, 7, 15, 1, 1, bias=1)
    add("pw_64x64_add", "pw", FAST, "k_conv_pw<64, 64, ADD, true>", 1, 64, 64, 7, 15, 1, 1, entry="fused", scale=1, res=1)
    add("pw_64x64_acc", "pw", FAST, "k_conv_pw<64, 64, STATS, false>", 1, 64, 64, 7, 15, 1, 1, entry="conv2d_acc")
    add("pw_64x64_bnbwd_acc", "pw", FAST, "k_conv_pw<64, 64, BNB, false>", 1, 64, 64, 7, 15, 1, 1, tr=1, entry="bnbwd_acc", alpha=1)
    add("pw_64x128_acc_bias", "pw", FAST, "k_conv_pw<64, 128, STATS, true>", 1, 64, 128, 7, 15, 1, 1, entry="conv2d_acc", bias=1)
    add("pw_64x128_add", "pw", FAST, "k_conv_pw<64, 128, ADD, true>", 1, 64, 128, 7, 15, 1, 1, entry="fused", res=1)
    add("pw_128x64_bnbwd_acc", "pw", FAST, "k_conv_pw<128, 64, BNB, false>", 1, 128, 64, 7, 15, 1, 1, tr=1, entry="bnbwd_acc")
    add("pw_128x64_plain", "pw", FAST, "k_conv_pw<128, 64, PLAIN, false>", 1, 128, 64, 7, 15, 1, 1)
    add("pw_32x64_acc", "pw", FAST, "k_conv_pw<32, 64, STATS, false>", 1, 18, 64, 7, 15, 1, 1, entry="conv2d_acc")
    # pw_launch (conv_pw.hip:316-319): 64 -> 64 has NB = 2 blocks of 32 pixels per unit and NCG = 1, need = ceil(ceil(ceil(M / 32)
    # / 2) / 4) exceeds cus * pw_wgs_per_cu = 1024 from M = 262 145 on: 512 x 513 = 262 656 pixels, need = 1026
    add("pw_64x64_n1_512x513", "pw", FAST, "k_conv_pw<64, 64, PLAIN, false>", 1, 64, 64, 512, 513, 1, 1, amp=1)
    add("pw_64x64_rows", "pw", FAST, "k_conv_fast<bf16, 256 x 64, one stage>", 1, 64, 64, 7, 15, 1, 1, stats="rows")   # conv_pw.hip:360
    add("pw_64x64_alpha", "pw", FAST, "k_conv_fast<bf16, 256 x 64, one stage>", 1, 64, 64, 7, 15, 1, 1, entry="fused", alpha=1)   # :359
    # ---- k_conv_halo: c0p % 64 == 0 and >= 128, coutp % 128 == 0, 3x3 / stride 1, the 70 % rule (conv_halo.hip:970-976)
    A = dict(n=1, c0=128, cout=128, h=14, w=14)                                                              # one tile
    H128, H256 = "k_conv_halo<128, %s, m16>", "k_conv_halo<256, %s, m16>"
    add("halo_a_plain", "halo", HALO, H128 % "plain", **A)
    add("halo_a_bias", "halo", HALO, H128 % "plain", bias=1, **A)
    add("halo_a_fused", "halo", HALO, H128 % "plain", entry="fused", scale=1, alpha=1, res=1, **A)
    add("halo_a_fused_rf", "halo", HALO, H128 % "plain", entry="fused", scale=1, alpha=1, res=1, res_first=1, **A)
    add("halo_a_rows", "halo", HALO, H128 % "plain", stats="rows", **A)                                      # 1 tile, 2 rows: one zeroed
    add("halo_a_acc", "halo", HALO, H128 % "plain", entry="conv2d_acc", **A)
    add("halo_a_bnbwd", "halo", HALO, H128 % "FUSE", tr=1, entry="bnbwd", alpha=1, **A)
    add("halo_a_bnbwd_acc", "halo", HALO, H128 % "FUSE", tr=1, entry="bnbwd_acc", **A)
    add("halo_a_bnin", "halo", HALO, H128 % "bnin", entry="bnin", **A)
    add("halo_a_bnin_alpha_rows", "halo", HALO, H128 % "bnin", entry="bnin", alpha=1, stats="rows", **A)
    add("halo_a_tr", "halo", HALO, H128 % "plain", tr=1, **A)
    Bs = dict(n=2, c0=192, cout=256, h=13, w=27)                                                             # the wide tile, c0p % 128 != 0, partial tiles
    add("halo_b_plain", "halo", HALO, H256 % "plain", **Bs)
    add("halo_b_rows", "halo", HALO, H256 % "plain", stats="rows", **Bs)                                      # 4 tiles <= ceil(702 / 128) = 6 rows
    add("halo_b_bnbwd", "halo", HALO, H256 % "FUSE", tr=1, entry="bnbwd", alpha=1, **Bs)
    # (256 input channels: msml_bn_act_fwd, the unfused counterpart, needs C / 8 to divide 256 and refuses 192)
    add("halo_b_bnin_alpha", "halo", HALO, H256 % "bnin", entry="bnin", alpha=1, **dict(Bs, c0=256))
    add("halo_b_tr", "halo", HALO, H256 % "plain", tr=1, **Bs)
    add("halo_b_fused", "halo", HALO, H256 % "plain", entry="fused", scale=1, res=1, **Bs)
    Cs = dict(n=3, c0=128, cout=384, h=14, w=14)                                                             # three 128-column blocks
    add("halo_c_plain", "halo", HALO, H128 % "plain", **Cs)
    add("halo_c_acc_bias", "halo", HALO, H128 % "plain", entry="conv2d_acc", bias=1, **Cs)
    add("halo_d_9x13_plain", "halo", FAST, "k_conv_fast<bf16, 128 x 128>", 1, 128, 128, 9, 13)                 # 1170 < 1568: fails the 70 % rule
    add("halo_a_fused_m32", "halo", HALO, "k_conv_halo<128, plain, m32>", entry="fused", scale=1, alpha=1, res=1,
        switch=("MSML_HALO_M16", 0), **A)
    add("halo_b_plain_m32", "halo", HALO, "k_conv_halo<256, plain, m32>", switch=("MSML_HALO_M16", 0), **Bs)
    # ---- k_conv_halo_p: coutp = 128, c0p % 64 == 0, tiles >= 2 * 256 (conv_halo.hip:954-957), plain / acc / bnb acc / bnin acc
    Ps = dict(n=515, c0=64, cout=128, h=14, w=14, amp=1)                                                       # 515 tiles: two rounds and three more
    add("halop_n515_acc", "halo_p", HALOP, "k_conv_halo_p<plain>", entry="conv2d_acc", **Ps)
    add("halop_n515_bnbwd_acc", "halo_p", HALOP, "k_conv_halo_p<FUSE>", tr=1, entry="bnbwd_acc", alpha=1, **Ps)
    add("halop_n515_bnin_acc", "halo_p", HALOP, "k_conv_halo_p<bnin>", entry="bnin_acc", alpha=1, **Ps)
    Qs = dict(n=90, c0=128, cout=128, h=27, w=40, amp=1)                                                       # 540 partial tiles
    add("halop_n90_27x40_acc", "halo_p", HALOP, "k_conv_halo_p<plain>", entry="conv2d_acc", **Qs)
    add("halop_n90_27x40_bnin_acc", "halo_p", HALOP, "k_conv_halo_p<bnin>", entry="bnin_acc", **Qs)
    add("halop_n90_27x40_bias", "halo_p", HALOP, H128 % "plain", bias=1, **Qs)                                # conv_halo.hip:998: bias -> k_conv_halo
    # ---- k_conv_halo2: stride 2 and mosaics (conv_halo2.hip:548-572, 590-597)
    G = "k_conv_halo2<%d, geom %d, mos %d, %s>"
    add("h2_fwd_n1_28", "halo2", H2, G % (128, 1, 0, "plain"), 1, 128, 128, 28, 28, stride=2)
    add("h2_fwd_n3_26_acc", "halo2", H2, G % (128, 1, 0, "plain"), 3, 128, 128, 26, 26, stride=2, entry="conv2d_acc")   # 13 x 13 grid
    add("h2_fwd_n1_28_wide_aff", "halo2", H2, G % (256, 1, 0, "plain"), 1, 256, 256, 28, 28, stride=2, entry="fused", scale=1)
    add("h2_bwd_n2_14", "halo2", H2, G % (128, 2, 0, "plain"), 2, 128, 128, 14, 14, stride=2, tr=1, opad=1)
    add("h2_bwd_n2_14_bnbwd_acc", "halo2", H2, G % (128, 2, 0, "FUSE"), 2, 128, 128, 14, 14, stride=2, tr=1, opad=1, entry="bnbwd_acc", alpha=1)
    # fill7: ceil(N / 4) * (coutp / 128) * slices >= 160; N = 318 -> 80 mosaics, the last one holds two images
    add("h2_m7_n318_plain", "halo2", H2, G % (128, 0, 7, "plain"), 318, 256, 256, 7, 7, amp=1)
    add("h2_m7_n318_res", "halo2", H2, G % (128, 0, 7, "plain"), 318, 256, 256, 7, 7, amp=1, entry="fused", res=1)
    add("h2_m7_n318_fwd_acc", "halo2", H2, G % (128, 1, 7, "plain"), 318, 256, 256, 14, 14, stride=2, entry="conv2d_acc", amp=1)
    add("h2_m7_n158_bwd", "halo2", H2, G % (128, 2, 7, "plain"), 158, 256, 128, 7, 7, stride=2, tr=1, opad=1, amp=1)     # 40 mosaics x 4 slices
    add("h2_m7_n158_bwd_bnbwd_acc", "halo2", H2, G % (128, 2, 7, "FUSE"), 158, 256, 128, 7, 7, stride=2, tr=1, opad=1, entry="bnbwd_acc", amp=1)
    add("h2_m7_n317_plain", "halo2", H2, G % (128, 0, 7, "plain"), 317, 256, 256, 7, 7, amp=1)               # the first N of fill7: one image in the last mosaic
    # fill4: ceil(N / 6) * (coutp / 128) >= 160; N = 236 -> 40 mosaics, the last one holds two images
    add("h2_m4_n236_plain", "halo2", H2, G % (128, 0, 4, "plain"), 236, 512, 512, 4, 4, amp=1)
    add("h2_m4_n236_aff_acc", "halo2", H2, G % (128, 0, 4, "plain"), 236, 512, 512, 4, 4, amp=1, entry="conv2d_acc", bias=1)
    # refused epilogues (conv_halo2.hip:593, 595): alpha, res_first and row-mode statistics go to the im2col kernel
    add("h2_m7_n318_alpha", "halo2", H2, "k_conv_fast<bf16, 128 x 128>", 318, 256, 256, 7, 7, amp=1, entry="fused", alpha=1)
    add("h2_fwd_n1_28_rows", "halo2", H2, "k_conv_fast<bf16, 128 x 128>", 1, 128, 128, 28, 28, stride=2, stats="rows")
    add("h2_bwd_n2_14_res_first", "halo2", H2, "k_conv_fast<bf16, 128 x 128, parity>", 2, 128, 128, 14, 14, stride=2, tr=1, opad=1,
        entry="fused", alpha=1, res=1, res_first=1)
    # ---- k_conv_line: 7x1 / 1x7, H = W in {28, 56}, (64, 32), (32, 32), (32, 64) (conv_line.hip:188-192); 224 / H lines per tile:
    # H = 28 has 8 lines per tile and a partial last tile of 4
    modes = (dict(bias=1), dict(entry="fused", scale=1, res=1), dict(tr=1), dict(), dict(entry="fused", scale=1), dict(bias=1, tr=1))
    i = 0
    for (ci, co, cr, cor) in ((64, 32, 64, 18), (32, 32, 18, 18), (32, 64, 18, 64)):
        for (r, s) in ((7, 1), (1, 7)):
            for h in (28, 56):
                m = modes[i % len(modes)]
                add("line_%dx%d_%dx%d_%d_%s" % (ci, co, r, s, h, "_".join(sorted(m)) or "plain"), "line", LINE,
                    "k_conv_line<%d, %d>" % (ci, co), 1, cr, cor, h, h, r, s, **m)
                i += 1
    add("line_32x32_1x7_n130_28", "line", LINE, "k_conv_line<32, 32>", 130, 18, 18, 28, 28, 1, 7, amp=1)        # 520 tiles over 512 workgroups
    add("line_64x32_7x1_n65_28", "line", LINE, "k_conv_line<64, 32>", 65, 64, 18, 28, 28, 7, 1, bias=1, amp=1)  # one workgroup per CU, 260 tiles
    # ---- k_deconv4_fwd and msml_deconv4_bwd_data: two 18-of-32 segments, H in {14, 28, 56} (conv_d4.hip:158-160, 298)
    for h in (14, 28, 56):
        add("d4_fwd_n2_%d" % h, "d4", D4, "k_deconv4_fwd", 2, 18, 18, h, h, 4, 4, 2, 1, 1, tr=1, c1=18, bias=1)
        add("d4_bwd_n2_%d" % h, "d4", FAST, "k_deconv4_bwd", 2, 18, 36, 2 * h, 2 * h, 4, 4, 2, 1, 1, entry="deconv4_bwd_data", coutp=64)
    # ---- k_conv_fast, the im2col kernel (conv_fast.hip:617-714)
    add("fast_128x128_n1_64x128_9x13", "fast", FAST, "k_conv_fast<bf16, 128 x 128>", 1, 64, 128, 9, 13)
    add("fast_256x64_n5_128x64_9", "fast", FAST, "k_conv_fast<bf16, 256 x 64>", 5, 128, 64, 9, 9, bias=1)
    add("fast_256x32_n5_64x18_9", "fast", FAST, "k_conv_fast<bf16, 256 x 32>", 5, 64, 18, 9, 9, stats="rows")
    # small-M tiles (conv_fast.hip:666-670): default workgroups <= conv_small_m_wgs = 200 and M >= 2048 -- N = 128 at 4 x 4 is
    # M = 2048, 16 x 4 = 64 default workgroups; fill4 fails (22 mosaics x 4 < 160)
    add("fast_small_n128_512_4", "fast", FAST, "k_conv_fast<bf16, 64 x 128>", 128, 512, 512, 4, 4, amp=1)
    add("fast_small_n128_512_4_bnbwd_acc", "fast", FAST, "k_conv_fast<bf16, 64 x 128, FUSE>", 128, 512, 512, 4, 4, amp=1, tr=1, entry="bnbwd_acc", alpha=1)
    add("fast_small_n42_64_7_acc", "fast", FAST, "k_conv_fast<bf16, 64 x 64>", 42, 64, 64, 7, 7, entry="conv2d_acc")      # M = 2058; 7 x 7 fails the 70 % rule
    add("fast_small_n42_64x18_7", "fast", FAST, "k_conv_fast<bf16, 64 x 32>", 42, 64, 18, 7, 7)
    add("fast_n41_64_7_rows", "fast", FAST, "k_conv_fast<bf16, 256 x 64>", 41, 64, 64, 7, 7, stats="rows")                  # M = 2009 < 2048, and row mode
    add("fast_f32out_logits_n300", "fast", FAST, "k_conv_fast<f32, 128 x 128>", 300, 512, 1024, 1, 1, 1, 1, dtype=BF)    # the logits GEMM
    add("fast_2seg_n2_64+18_9", "fast", FAST, "k_conv_fast<bf16, 256 x 64>", 2, 64, 64, 9, 9, c1=18)                       # nsub[0] = 18: even
    # stride-2 transposed: the gather by output parity class (conv_fast.hip:648-657), even and odd sizes
    add("fast_par_3x3_n3_7to14", "fast", FAST, "k_conv_fast<bf16, 256 x 64, parity>", 3, 128, 64, 7, 7, stride=2, tr=1, opad=1)
    add("fast_par_3x3_n3_5to9", "fast", FAST, "k_conv_fast<bf16, 256 x 64, parity>", 3, 128, 64, 5, 5, stride=2, tr=1)
    add("fast_par_1x1_n3_7to14", "fast", FAST, "k_conv_fast<bf16, 256 x 64, parity>", 3, 128, 64, 7, 7, 1, 1, 2, tr=1, opad=1)
    add("fast_par_1x1_n3_7to13", "fast", FAST, "k_conv_fast<bf16, 256 x 64, parity>", 3, 128, 64, 7, 7, 1, 1, 2, tr=1)
    add("fast_par_2seg_n3_7to14", "fast", FAST, "k_conv_fast<bf16, 256 x 64, parity>", 3, 64, 64, 7, 7, stride=2, tr=1, opad=1, c1=18)
    add("fast_par_d4_n2_7to14", "fast", FAST, "k_conv_fast<bf16, 256 x 32, parity>", 2, 18, 18, 7, 7, 4, 4, 2, 1, 1, tr=1, c1=18, bias=1)   # H = 7: k_deconv4_fwd refuses
    add("fast_par_bnbwd_n3_7to14", "fast", FAST, "k_conv_fast<bf16, 256 x 64, FUSE, parity>", 3, 128, 64, 7, 7, stride=2, tr=1, opad=1, entry="bnbwd", alpha=1)
    add("fast_bnbwd_n5_128x64_9", "fast", FAST, "k_conv_fast<bf16, 256 x 64, FUSE>", 5, 128, 64, 9, 9, tr=1, entry="bnbwd")
    add("fast_1stage_1x1s2_n3_64x128", "fast", FAST, "k_conv_fast<bf16, 128 x 128, one stage>", 3, 64, 128, 14, 14, 1, 1, 2)   # stride 2: k_conv_pw refuses
    add("fast_7x7_n5_256", "fast", FAST, "k_conv_fast<bf16, 128 x 128>", 5, 256, 256, 7, 7)                            # below fill7
    add("fast_4x4_n7_512", "fast", FAST, "k_conv_fast<bf16, 128 x 128>", 7, 512, 512, 4, 4)                                   # below fill4 and M < 2048
    add("fast_fc_n40_512_7x7", "fast", FAST, "k_conv_fast<bf16, 128 x 128>", 40, 512, 512, 7, 7, 7, 7, 1, 0, 0, bias=1)       # the fc layer: K = 25 088
    add("fast_s4_n2_64_16", "fast", FAST, "k_conv_fast<bf16, 256 x 64>", 2, 64, 64, 16, 16, stride=4)
    # ---- k_conv_igemm, the generic kernel: f32 operands, or c0p % 32 != 0, or MSML_NO_FAST_CONV (conv_igemm.hip:434-449)
    add("igemm_f32_n2_64_9", "igemm", IGEMM, "k_conv_igemm<f32, f32, 256 x 64>", 2, 64, 64, 9, 9, dtype=FF, stats="rows")
    add("igemm_f32_s2_2seg_n2", "igemm", IGEMM, "k_conv_igemm<f32, f32, 128 x 128>", 2, 24, 128, 9, 9, stride=2, c1=8, c0p=24, c1p=8, dtype=FF, bias=1)
    add("igemm_f32_s4_n2_16", "igemm", IGEMM, "k_conv_igemm<f32, f32, 256 x 32>", 2, 40, 18, 16, 16, stride=4, c0p=40, dtype=FF)
    add("igemm_f32_tr_s2_n2_5to9", "igemm", IGEMM, "k_conv_igemm<f32, f32, 256 x 64>", 2, 64, 64, 5, 5, stride=2, tr=1, dtype=FF)
    add("igemm_bf16f32_c24_n2_9", "igemm", IGEMM, "k_conv_igemm<bf16, f32, 256 x 64>", 2, 24, 64, 9, 9, c0p=24, dtype=BF)
    add("igemm_bf16_c8_s2_n3_28", "igemm", IGEMM, "k_conv_igemm<bf16, bf16, 256 x 64>", 3, 3, 64, 28, 28, stride=2, c0p=8, stats="rows")   # the stems' 3-of-8
    add("igemm_bf16_c24_tr_n2_9", "igemm", IGEMM, "k_conv_igemm<bf16, bf16, 256 x 32>", 2, 24, 18, 9, 9, c0p=24, tr=1, bias=1)
    add("igemm_bf16_nofast_n2_64_14", "igemm", IGEMM, "k_conv_igemm<bf16, bf16, 256 x 64>", 2, 64, 64, 14, 14, switch=("MSML_NO_FAST_CONV", 1),
        entry="conv2d_acc")
    assert len({c.name for c in L}) == len(L)
    return L


# Shapes the entry point answers MSML_ERR_UNSUPPORTED for before any launch (no data is ever generated for them)
REFUSED = (
    # msml_conv2d_bnin: 9 x 13 fails the 70 % rule of msml_conv_halo_applies (conv_halo.hip:974)
    mk("refused_bnin_9x13", "refused", FAST, UNSUPPORTED, 1, 128, 128, 9, 13, entry="bnin"),
    # msml_conv2d_bnin: 64 input channels, c0p < 128 (conv_halo.hip:971)
    mk("refused_bnin_64", "refused", WS, UNSUPPORTED, 2, 64, 64, 14, 14, entry="bnin", stats="rows"),
    mk("refused_bnin_acc_9x13", "refused", FAST, UNSUPPORTED, 1, 128, 128, 9, 13, entry="bnin_acc"),
    # msml_conv2d_bnbwd has no *_applies: it refuses what msml_conv_fast_dispatch refuses.  96 channels are no family's
    # (r32: 32, pw: 1x1, s2r / ws: 64, halo / halo2: c0p % 64), and the im2col kernel refuses N*P*Q >= 2^24 (conv_fast.hip:628)
    mk("refused_bnbwd_96_4096", "refused", FAST, UNSUPPORTED, 1, 96, 96, 4096, 4096, tr=1, entry="bnbwd"),
)


def case_id(c):
    return c.name


def find(name):
    return next(c for c in cases() + list(REFUSED) if c.name == name)


# ------------------------------------------------------------------------------------------------- the route, restated
def tile_m(coutp):
    return 256 if coutp <= 64 else 128                 # msml_conv_tile_m, conv_igemm.hip:354


def tile_n(coutp):
    return 32 if coutp <= 32 else (64 if coutp <= 64 else 128)      # msml_conv_tile_n, conv_igemm.hip:355


def kop(c):
    return cdiv(c.coutp, tile_n(c.coutp)) * tile_n(c.coutp)


def _opt(c, name, default):
    return c.switch[1] if c.switch and c.switch[0] == name else default


def _bnb(c):
    return {"bnbwd": "rows", "bnbwd_acc": "acc"}.get(c.entry)


def _xin(c):
    return {"bnin": "coef", "bnin_acc": "acc"}.get(c.entry)


def _alpha(c):
    return bool(c.alpha) and c.entry == "fused"        # (the alpha of a bnbwd / bnin case is the BatchNorm's, not the epilogue's)


def _shift(c):
    return bool(c.bias) or c.entry == "fused"          # msml_conv2d_fused always passes its shift as the bias


def _real70(n, gh, gw):
    tiles = n * cdiv(gh, 14) * cdiv(gw, 14)
    return n * gh * gw * 10 >= tiles * 224 * 7          # "< 70 % real GEMM rows: im2col kernel wins"


def _same3x3(c):
    return (c.R, c.S, c.stride, c.ph, c.pw) == (3, 3, 1, 1, 1) and c.P == c.H and c.Q == c.W


def ws_applies(c, want_stats):                          # conv_ws.hip:462-473
    if not _same3x3(c) or c.c0p != 64 or c.coutp != 64:
        return False
    tiles = c.N * cdiv(c.H, 14) * cdiv(c.W, 14)
    if not _real70(c.N, c.H, c.W):
        return False
    if want_stats and min(tiles, CUS) > cdiv(c.N * c.P * c.Q, tile_m(c.coutp)):
        return False
    return True


def s2r_applies(c):                                     # conv_s2r.hip:566-584
    if (c.R, c.S, c.ph, c.pw, c.c0p, c.coutp) != (3, 3, 1, 1, 64, 64) or c.stride not in (1, 2):
        return False
    if c.stride == 1:
        if c.P != c.H or c.Q != c.W:
            return False
        gh, gw = c.H, c.W
    elif not c.tr:
        if c.H % 2 or c.W % 2 or c.P != c.H // 2 or c.Q != c.W // 2:
            return False
        gh, gw = c.P, c.Q
    else:
        if c.P != 2 * c.H or c.Q != 2 * c.W:
            return False
        gh, gw = c.H, c.W
    return _real70(c.N, gh, gw)


def halo_persist_shape(c):                              # conv_halo.hip:948-961
    if not _same3x3(c) or c.coutp != 128 or c.c0p % 64 or c.c0p < 64:
        return False
    tiles = c.N * cdiv(c.H, 14) * cdiv(c.W, 14)
    return tiles >= 2 * CUS and _real70(c.N, c.H, c.W)


def halo_applies(c, want_stats):                        # conv_halo.hip:964-980
    if not _same3x3(c) or c.c0p % 64 or c.c0p < 128 or c.coutp % 128:
        return False
    tiles = c.N * cdiv(c.H, 14) * cdiv(c.W, 14)
    if not _real70(c.N, c.H, c.W):
        return False
    return not (want_stats and tiles > cdiv(c.N * c.P * c.Q, tile_m(c.coutp)))


def halo2_tiling(c):                                    # conv_halo2.hip:543-573
    if (c.R, c.S, c.ph, c.pw) != (3, 3, 1, 1) or c.c0p % 64 or c.c0p < 128 or c.coutp % 128:
        return 0
    if c.stride == 1:
        if c.P != c.H or c.Q != c.W:
            return 0
        gh, gw = c.H, c.W
    elif c.stride == 2 and not c.tr:
        if c.H % 2 or c.W % 2 or c.P != c.H // 2 or c.Q != c.W // 2:
            return 0
        gh, gw = c.P, c.Q
    elif c.stride == 2:
        if c.P != 2 * c.H or c.Q != 2 * c.W:
            return 0
        gh, gw = c.H, c.W
    else:
        return 0
    cblk, slices = c.coutp // 128, 4 if (c.stride == 2 and c.tr) else 1
    if (gh, gw) == (7, 7):
        return 2 if cdiv(c.N, 4) * cblk * slices >= 160 else 0
    if (gh, gw) == (4, 4) and c.stride == 1:
        return 3 if cdiv(c.N, 6) * cblk >= 160 else 0
    if c.stride == 1:
        return 0
    return 1 if _real70(c.N, gh, gw) else 0


def line_applies(c):                                    # conv_line.hip:184-195
    if not ((c.R, c.S, c.ph, c.pw) in ((7, 1, 3, 0), (1, 7, 0, 3))):
        return False
    if c.stride != 1 or c.H != c.W or c.P != c.H or c.Q != c.W or c.H not in (28, 56):
        return False
    return (c.c0p, c.coutp) in ((64, 32), (32, 32), (32, 64))


def d4_applies(c):                                      # conv_d4.hip:156-163
    return bool(c.tr) and (c.R, c.S, c.stride, c.ph, c.pw) == (4, 4, 2, 1, 1) and (c.c0p, c.c1p, c.coutp) == (32, 32, 32) and \
        c.H == c.W and c.P == 2 * c.H and c.Q == 2 * c.W and c.H in (14, 28, 56)


def _halo_dispatch(c):                                  # conv_halo.hip:983-1079
    bnb, xin, stats = _bnb(c), _xin(c), c.stats
    m16 = _opt(c, "MSML_HALO_M16", 2)
    epi = _shift(c) or c.scale or _alpha(c) or c.res
    pshape = m16 >= 2 and not epi and (not xin or (xin == "acc" and not c.tr and not bnb and stats and c.c0p <= 1024)) and \
        stats in (None, "acc") and bnb in (None, "acc") and halo_persist_shape(c)
    if not pshape and not halo_applies(c, stats is not None):
        return None
    if bnb and (epi or stats):
        return None
    if xin and (bnb or c.tr or c.c0p > 1024):
        return None
    tiles = c.N * cdiv(c.H, 14) * cdiv(c.W, 14)
    mode = "bnin" if xin else ("FUSE" if bnb else "plain")
    if pshape:
        return "k_conv_halo_p<%s>" % mode, tiles
    wide = c.coutp % 256 == 0
    return "k_conv_halo<%d, %s, %s>" % (256 if wide else 128, mode, "m16" if m16 and (wide or m16 >= 2) else "m32"), tiles


def _fast_dispatch(c):
    """(instantiation, *rows_used of a bnbwd call) of msml_conv_fast_dispatch (conv_fast.hip:570-715), None when it refuses."""
    bnb, stats = _bnb(c), c.stats
    bias, in1, out_bf = _shift(c), c.c1p > 0, c.dtype[1] == BF16
    alpha = _alpha(c)
    epi = bias or c.scale or alpha or c.res
    if c.dtype[0] != BF16 or (bnb and (not out_bf or stats)) or ((c.scale or alpha or c.res) and not out_bf):
        return None
    if c.c0p % 32 or (in1 and c.c1p % 32):
        return None
    tiles14 = lambda gh, gw: c.N * cdiv(gh, 14) * cdiv(gw, 14)
    if not in1 and out_bf:
        # conv_r32.hip:288-318
        if (c.c0p, c.coutp) == (32, 32) and _same3x3(c) and not epi and stats != "rows" and not (bnb and (bnb != "acc" or stats)) and \
                8 <= c.W <= 62 and c.H >= 2:
            mode = "BNB" if bnb else ("STATS" if stats else "PLAIN")
            return "k_conv_r32<%s, %s>" % (mode, "true" if c.tr else "false"), 1
        # conv_pw.hip:343-378
        if (c.R, c.S, c.stride, c.ph, c.pw) == (1, 1, 1, 0, 0) and c.P == c.H and c.Q == c.W and not alpha and \
                not (c.res and c.res_first) and stats != "rows" and not (bnb and (bnb != "acc" or bias or c.scale or c.res or stats)) and \
                not (stats and c.res) and (c.c0p, c.coutp) in ((32, 64), (64, 32), (64, 64), (64, 128), (128, 64)):
            mode = "BNB" if bnb else ("ADD" if c.res else ("STATS" if stats else "PLAIN"))
            aff = "false" if bnb else ("true" if (bias or c.scale) else "false")
            return "k_conv_pw<%d, %d, %s, %s>" % (c.c0p, c.coutp, mode, aff), 1

        def s2r():                                      # conv_s2r.hip:602-630
            if not s2r_applies(c) or epi or (c.stride == 1 and bnb) or (stats and (stats != "acc" or (c.tr and c.stride == 2))):
                return None
            if bnb and (bnb != "acc" or not c.tr or stats):
                return None
            gh, gw = (c.H, c.W) if (c.tr or c.stride == 1) else (c.P, c.Q)
            mode = 0 if c.stride == 1 else (2 if c.tr else 1)
            return "k_conv_s2r<%d, %s>" % (mode, "true" if bnb else "false"), min(tiles14(gh, gw), CUS)
        if c.stride == 1 and not bnb and s2r():
            return s2r()
        # conv_ws.hip:488-517
        if ws_applies(c, stats is not None) and not (bnb and (epi or stats)):
            return "k_conv_ws<%s>" % ("true" if bnb else "false"), min(tiles14(c.H, c.W), CUS)
        r = _halo_dispatch(c)
        if r:
            return r
        # conv_halo2.hip:576-644
        t = halo2_tiling(c)
        geom = 0 if c.stride == 1 else (2 if c.tr else 1)
        if t and not (alpha or c.res_first) and not (bnb and (bias or c.scale)) and stats != "rows" and \
                not (bnb and (bnb != "acc" or c.res or stats)) and not (c.res and stats) and not (bnb and geom == 1):
            mos = {1: 0, 2: 7, 3: 4}[t]
            wide = c.coutp % 256 == 0 and not mos
            units = cdiv(c.N, 6 if t == 3 else 4) if mos else tiles14(*((c.P, c.Q) if geom == 1 else (c.H, c.W)))
            return "k_conv_halo2<%d, geom %d, mos %d, %s>" % (256 if wide else 128, geom, mos, "FUSE" if bnb else "plain"), \
                units * (4 if geom == 2 else 1)
        if s2r():
            return s2r()
    nsub0, nsub1 = c.R * c.S * (c.c0p // 32), c.R * c.S * (c.c1p // 32)
    if in1 and nsub0 & 1:
        return None
    M = c.N * c.P * c.Q
    if M >= 2 ** 24:
        return None
    parity = bool(c.tr) and c.stride == 2 and stats is None
    if parity and in1:
        for k in range(4):
            r0, s0 = ((k >> 1) + c.ph) & 1, ((k & 1) + c.pw) & 1
            nr, ns = ((c.R - r0 + 1) // 2 if c.R > r0 else 0), ((c.S - s0 + 1) // 2 if c.S > s0 else 0)
            parity = parity and (nr * ns * (c.c0p // 32)) % 2 == 0
    bn = tile_n(c.coutp)
    mtile = c.N * ((c.P + 1) // 2) * ((c.Q + 1) // 2) if parity else M
    def_wgs = cdiv(mtile, 128 if bn == 128 else 256) * cdiv(c.coutp, bn) * (4 if parity else 1)
    small = out_bf and def_wgs <= 200 and M >= 2048 and stats in (None, "acc") and bnb in (None, "acc")
    if bnb and epi:
        return None
    bm = 64 if small else (128 if bn == 128 else 256)
    one_stage = (nsub0 + nsub1 + 1) // 2 <= 1
    inst = "k_conv_fast<%s, %d x %d%s%s%s>" % ("bf16" if out_bf else "f32", bm, bn, ", FUSE" if bnb else "", ", parity" if parity else "",
                                              ", one stage" if one_stage else "")
    return inst, cdiv(mtile, bm) * (4 if parity else 1)


def route(c):
    """(instantiation or UNSUPPORTED, rows_used of a bnbwd call or None): the dispatch of the case's entry point."""
    no_fast = _opt(c, "MSML_NO_FAST_CONV", 0)
    bf = c.dtype == BB
    if c.entry == "deconv4_bwd_data":
        return "k_deconv4_bwd", None
    if c.entry in ("conv2d", "conv2d_acc"):             # conv_igemm.hip:423-449
        if bf and not c.c1p and not c.stats and not no_fast and line_applies(c):
            return "k_conv_line<%d, %d>" % (c.c0p, c.coutp), None
        if bf and c.c1p and not c.stats and not no_fast and d4_applies(c):
            return "k_deconv4_fwd", None
        r = None if no_fast else _fast_dispatch(c)
        if r:
            return r[0], None
        names = {BF16: "bf16", F32: "f32"}
        bn = tile_n(c.coutp)
        return "k_conv_igemm<%s, %s, %d x %d>" % (names[c.dtype[0]], names[c.dtype[1]], 128 if bn == 128 else 256, bn), None
    if c.entry == "fused":                              # conv_igemm.hip:494-499
        if not c.c1p and not c.alpha and not (c.res and c.res_first) and not no_fast and line_applies(c):
            return "k_conv_line<%d, %d>" % (c.c0p, c.coutp), None
        r = _fast_dispatch(c)
        return (r[0], None) if r else (UNSUPPORTED, None)
    if c.entry in ("bnbwd", "bnbwd_acc"):               # conv_igemm.hip:557-569
        r = _fast_dispatch(c)
        return r if r else (UNSUPPORTED, None)
    if c.entry == "bnin":                               # conv_igemm.hip:601-625
        if no_fast or c.c0p > 1024 or not halo_applies(c, c.stats is not None):
            return UNSUPPORTED, None
        r = _halo_dispatch(c)
        return (r[0], None) if r else (UNSUPPORTED, None)
    assert c.entry == "bnin_acc"                        # conv_igemm.hip:628-668
    if no_fast or c.c0p > 1024 or 256 % (c.c0p // 8):
        return UNSUPPORTED, None
    if not (_opt(c, "MSML_HALO_M16", 2) >= 2 and halo_persist_shape(c)) and not halo_applies(c, True):
        return UNSUPPORTED, None
    r = _halo_dispatch(c)
    return (r[0], None) if r else (UNSUPPORTED, None)


def switched(c):
    return _lib.option(c.switch[0], c.switch[1]) if c.switch else contextlib.nullcontext()


def kernel_name(c):
    """What msml_conv2d_kernel answers for the case's shape, with the case's switch set: no GPU."""
    with switched(c):
        if c.entry == "deconv4_bwd_data":
            return ""
        return _lib.value("msml_conv2d_kernel", c.c0p, c.c1p, c.coutp, c.N, c.H, c.W, c.P, c.Q, c.R, c.S, c.stride, c.ph, c.pw,
                          c.tr, c.dtype[0], c.dtype[1], int(c.stats is not None)).decode()


# ------------------------------------------------------------------------------------------------- data
def _seed(c, kind):
    seed = 0
    for x in (c.c0, c.c0p, c.c1, c.cout, c.N, c.H, c.W, c.P, c.R, c.S, c.stride, c.tr, c.amp, c.dtype[0],
              int(_xin(c) is not None), ("exact", "random").index(kind)):
        seed = (seed * 1000003 + x + 1) % (2 ** 31 - 1)
    return seed


def _gen(c, kind, tag):
    return torch.Generator().manual_seed((_seed(c, kind) + 7919 * tag) % (2 ** 31 - 1))


def in_dtype(c):
    return torch.bfloat16 if c.dtype[0] == BF16 else torch.float32


def out_dtype(c):
    return torch.bfloat16 if c.dtype[1] == BF16 else torch.float32


def xmax(c):
    """Largest |operand| of the exact data as the kernel multiplies it (behind the input BatchNorm: |{-1,0,1}*2 + {-2,0,2}|)."""
    return 4 if _xin(c) else c.amp


def nnz_per_row(c):
    K = c.R * c.S * (c.c0 + c.c1)
    if _xin(c) and c.amp == 1:
        return 12                                       # (the ~100 000-pixel cases: sum y^2 < 2^24 with E[X^2] ~ 5)
    return K if K * xmax(c) <= 256 else min(85, 256 // xmax(c))


def exact_weight(c):
    """[cout][c0 + c1][R][S] in {-1, 0, 1}: nnz_per_row nonzeros per reduction row -- a cyclic run that gives every row
    every tap and every (r, s, c) position a row, the rest at random positions."""
    K, T, g = c.R * c.S * (c.c0 + c.c1), c.R * c.S, _gen(c, "exact", 1)
    sign = (torch.randint(0, 2, (c.cout, K), generator=g) * 2 - 1).float()
    nnz = nnz_per_row(c)
    if nnz == K:
        return sign.view(c.cout, c.c0 + c.c1, c.R, c.S)
    run = max(T, cdiv(K, c.cout))
    assert run <= nnz, (c.name, run, nnz)
    score = torch.rand(c.cout, K, generator=g)
    pos = (torch.arange(c.cout).view(-1, 1) * run + torch.arange(run).view(1, -1)) % K
    sign.scatter_(1, pos, sign.gather(1, pos[:, :1]) * (1 - 2 * (torch.arange(run) % 2)).float().view(1, -1))   # (+ - + - ... along the run:
    score.scatter_(1, pos, -1.0)                         #  a per-channel constant of the operand does not add up over the taps)
    idx = score.topk(nnz, dim=1, largest=False).indices
    w = torch.zeros(c.cout, K)
    w.scatter_(1, idx, sign.gather(1, idx))
    return w.view(c.cout, c.c0 + c.c1, c.R, c.S)            # position p = channel * T + tap


def _padded(shape, real, fill, dtype):
    t = torch.full(shape, PAD, dtype=torch.float32)
    t[..., :real] = fill
    return t.to(dtype)


def _quarters(shape, g, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).float() / 4


def _choice(values, n, g):
    return torch.tensor(values)[torch.randint(0, len(values), (n,), generator=g)]


def _chan(c, real, n, pad=0.0):
    """A per-channel f32 vector [n] with `pad` in the pad channels (n - len(real) of them)."""
    t = torch.full((n,), pad)
    t[:real.numel()] = real
    return t


def make_data(c, kind):
    """Every operand of the call on the host, in the storage types; see the module docstring for the value sets."""
    d = make_inputs(c, kind)
    d.update(make_epilogue(c, kind))
    return d


def make_inputs(c, kind):
    """The input segments, the weight w [cout][c0 + c1][R][S] and the input BatchNorm's coefficients."""
    ex = kind == "exact"
    d = {}
    dt = in_dtype(c)
    for i, (cr, cp) in enumerate(((c.c0, c.c0p), (c.c1, c.c1p))):
        if not cp:
            d["x%d" % i] = None
            continue
        g = _gen(c, kind, 10 + i)
        shape = (c.N, c.H, c.W, cr)
        amp = 1 if _xin(c) else c.amp
        v = torch.randint(-amp, amp + 1, shape, generator=g).float() if ex else torch.randn(shape, generator=g)
        d["x%d" % i] = _padded((c.N, c.H, c.W, cp), cr, v, dt)
    if ex:
        w = exact_weight(c)
    else:
        w = torch.randn(c.cout, c.c0 + c.c1, c.R, c.S, generator=_gen(c, kind, 1)) * (2.0 / (c.R * c.S * (c.c0 + c.c1))) ** 0.5
    d["w"] = w.to(dt).float()
    if _xin(c):
        g = _gen(c, kind, 5)
        ci, cip = c.c0, c.c0p
        if ex:      # X = in * (+-2) + {-2, 0, 2}: even integers, halved where negative by alpha = 0.5
            d["in_scale"] = _chan(c, _choice([2.0, -2.0], ci, g), cip, 3.0)
            d["in_shift"] = _chan(c, _choice([-2.0, 0.0, 2.0], ci, g), cip, 3.0)
            al = torch.full((ci,), 0.5)
        else:
            d["in_scale"] = _chan(c, (torch.rand(ci, generator=g) + 0.5), cip, 3.0)
            d["in_shift"] = _chan(c, torch.randn(ci, generator=g) * 0.5, cip, 3.0)
            al = torch.rand(ci, generator=g) * 0.3
        d["in_alpha"] = _chan(c, al, cip, 3.0) if c.alpha else None
    return d


def make_epilogue(c, kind):
    """bias / scale / alpha / residual of the epilogue and the saved BatchNorm input and coefficients of a bnbwd call."""
    ex = kind == "exact"
    d = {}
    co, cp = c.cout, c.coutp
    g = _gen(c, kind, 2)
    if c.bias or c.entry == "fused":
        d["bias"] = _chan(c, _quarters((co,), g) if ex else torch.randn(co, generator=g) * 0.5, cp)
    if c.scale:
        d["scale"] = _chan(c, _choice([0.5, 1.0, 2.0, -0.5, -1.0, -2.0], co, g) if ex else
                           (torch.rand(co, generator=g) + 0.5) * (torch.randint(0, 2, (co,), generator=g) * 2 - 1).float(), cp, 3.0)
    if c.alpha and c.entry == "fused":
        d["alpha"] = _chan(c, _choice([0.25, 0.5], co, g) if ex else torch.rand(co, generator=g) * 0.5, cp, 3.0)
    if c.res:
        g = _gen(c, kind, 3)
        r = torch.zeros(c.N, c.P, c.Q, cp)
        r[..., :co] = _quarters((c.N, c.P, c.Q, co), g) if ex else torch.randn(c.N, c.P, c.Q, co, generator=g)
        d["res"] = r.bfloat16()
    if _bnb(c):
        g = _gen(c, kind, 4)
        small = c.amp == 1
        bx = torch.randint(-2, 3, (c.N, c.P, c.Q, co), generator=g).float() if ex else torch.randn(c.N, c.P, c.Q, co, generator=g)
        d["bn_x"] = _padded((c.N, c.P, c.Q, cp), co, bx, torch.bfloat16)
        if ex:
            d["bn_scale"] = _chan(c, _choice([1.0, 2.0, -1.0] if small else [0.5, 1.0, 2.0, -1.0], co, g), cp, 3.0)
            d["bn_shift"] = _chan(c, _choice([-1.0, 0.0, 1.0], co, g), cp, 3.0)
            d["bn_mean"] = _chan(c, _choice([-1.0, 0.0, 1.0], co, g), cp, 3.0)
            d["bn_invstd"] = _chan(c, _choice([1.0, 2.0] if small else [0.5, 1.0, 2.0], co, g), cp, 3.0)
            al = _choice([0.5] if small else [0.25, 0.5], co, g)
        else:
            d["bn_scale"] = _chan(c, torch.rand(co, generator=g) + 0.5, cp, 3.0)
            d["bn_shift"] = _chan(c, torch.randn(co, generator=g) * 0.3, cp, 3.0)
            d["bn_mean"] = _chan(c, torch.randn(co, generator=g) * 0.2, cp, 3.0)
            d["bn_invstd"] = _chan(c, torch.rand(co, generator=g) + 0.5, cp, 3.0)
            al = torch.rand(co, generator=g) * 0.5
        d["bn_alpha"] = _chan(c, al, cp, 3.0) if c.alpha else None
    return d


EPS = 1e-5


def bnin_acc_operands(c, d, kind):
    """msml_conv2d_bnin_acc derives its coefficients from (acc_in, count, gamma, beta, eps): operands that give exactly
    d["in_scale"] / d["in_shift"] on exact data (mean an integer, invstd = 2, gamma = scale / 2, beta = shift + mean*scale:
    sums s = 4 mean, ss = 4 (1/4 - eps + mean^2) at count 4, spread over two accumulator rows), the sums of the tensor on random data."""
    cip = c.c0p
    acc = torch.zeros(8, 2, cip, dtype=torch.float64)
    if kind == "exact":
        g = _gen(c, kind, 6)
        mean = _chan(c, _choice([-1.0, 0.0, 1.0], c.c0, g), cip, 0.0).double()
        eps_f = float(torch.tensor(EPS, dtype=torch.float32))
        acc[0, 0], acc[0, 1] = 4.0 * mean + 5.0, 4.0 * (0.25 - eps_f + mean * mean)
        acc[3, 0] = -5.0
        gamma = d["in_scale"] / 2
        beta = d["in_shift"] + mean.float() * d["in_scale"]
        return acc, 4.0, gamma, beta
    x = d["x0"].double().reshape(-1, cip)
    acc[1, 0], acc[1, 1] = x.sum(0), (x * x).sum(0)
    return acc, float(x.shape[0]), d["in_scale"], d["in_shift"]           # (random: gamma / beta reuse the two vectors)


def bn_apply(x, scale, shift, alpha):
    """bf16(PReLU(x * scale + shift)) in f32 arithmetic: what msml_bn_act_fwd stores (up to an fma on random data)."""
    y = x.float() * scale + shift
    if alpha is not None:
        y = torch.where(y < 0, y * alpha, y)
    return y.bfloat16()


# ------------------------------------------------------------------------------------------------- the restatement
def _axis(c, t, n_out, n_in, pad):
    """The (output, input) index pairs of one axis for tap t as two arithmetic progressions: (o0, o_step, i0, i_step, count)."""
    if c.tr:
        pairs = [((i * c.stride - pad + t), i) for i in range(n_in) if 0 <= i * c.stride - pad + t < n_out]
    else:
        pairs = [(o, o * c.stride - pad + t) for o in range(n_out) if 0 <= o * c.stride - pad + t < n_in]
    if not pairs:
        return None
    so, si = (c.stride, 1) if c.tr else (1, c.stride)
    assert pairs == [(pairs[0][0] + k * so, pairs[0][1] + k * si) for k in range(len(pairs))]
    return pairs[0][0], so, pairs[0][1], si, len(pairs)


def _sl(a0, step, n):
    return slice(a0, a0 + (n - 1) * step + 1, step)


def conv_f64(c, xs, w, tapmask=None, segoff=None):
    """sum_seg sum_{r,s,c} in_seg[n,iy,ix,c] * w[ko][seg,r,s,c] in float64, one matmul per tap and segment over the pixel
    pairs the formula joins.  xs: the segments [N][H][W][real channels]; w: [cout][c0 + c1][R][S].  tapmask(r, s): None or a
    factor [N or 1][P][Q] on that tap's contribution (mutants); segoff: the channel offset of each segment in w (mutants)."""
    out = torch.zeros(c.N, c.P, c.Q, w.shape[0], dtype=torch.float64)
    offs = segoff or [0, xs[0].shape[3]]
    for r in range(c.R):
        ya = _axis(c, r, c.P, c.H, c.ph)
        for s in range(c.S):
            xa = _axis(c, s, c.Q, c.W, c.pw)
            if ya is None or xa is None:
                continue
            oy, ox = _sl(ya[0], ya[1], ya[4]), _sl(xa[0], xa[1], xa[4])
            iy, ix = _sl(ya[2], ya[3], ya[4]), _sl(xa[2], xa[3], xa[4])
            for seg, x in enumerate(xs):
                cs = x.shape[3]
                part = (x[:, iy, ix, :].reshape(-1, cs) @ w[:, offs[seg]:offs[seg] + cs, r, s].t()).view(c.N, ya[4], xa[4], -1)
                if tapmask is not None:
                    m = tapmask(r, s)
                    if m is not None:
                        part = part * m[:, oy, ox, None]
                out[:, oy, ox, :] += part
    return out


def operands(c, d, x_operand=None, mutant=None):
    """(segments in float64 with their real channels, w in float64) as the kernel multiplies them: behind the input
    BatchNorm the bf16 X (x_operand: the tensor a device's msml_bn_act_fwd made of in0, used instead of bn_apply)."""
    xs = []
    for i, cr in ((0, c.c0), (1, c.c1)):
        x = d["x%d" % i]
        if x is None:
            continue
        if i == 0 and _xin(c):
            x = bn_apply(x, d["in_scale"], d["in_shift"], d["in_alpha"]) if x_operand is None else x_operand
        x = x.double()
        if mutant == "pad_channel_leaks" and i == 0:
            assert x.shape[3] > cr
            x = x.clone()
            x[..., 0] += x[..., cr:].sum(-1)
        xs.append(x[..., :cr])
    return xs, d["w"].double()


MUTANTS = {
    # name: (the case it must be caught on, the checks that must fail there)
    "right_halo_column_dropped": ("halo_b_plain", ("exact", "budget")),
    "partial_tile_last_row_tap_above": ("ws_n2_13x27_plain", ("exact", "budget")),
    "parity_class_swapped": ("s2r_bwd_n5_14", ("exact", "budget")),
    "taps_not_flipped": ("ws_n2_13x27_tr", ("exact", "budget")),
    "second_segment_first_offset": ("fast_2seg_n2_64+18_9", ("exact", "budget")),
    "mosaic_image_reads_neighbour": ("h2_m7_n318_plain", ("exact", "budget")),
    "second_tile_of_workgroup_skipped": ("ws_n17_56_plain", ("exact", "budget")),
    "padding_before_batchnorm": ("halo_a_bnin_alpha_rows", ("exact", "budget")),
    "residual_prelu_order": ("halo_a_fused", ("exact", "budget")),
    "accumulator_rounded_to_bf16": ("halo_a_bias", ("budget",)),
    "statistics_other_definition": ("pw_32x64_acc", ("budget",)),
    "one_product_lost": ("halo_a_plain", ("exact", "budget")),
    "bnbwd_z_positive": ("halo_a_bnbwd", ("exact", "budget")),
    "pad_channel_leaks": ("r32_n1030_8_plain", ("exact", "budget")),
}


def accumulate(c, d, x_operand=None, mutant=None, absolute=False):
    """The accumulator [N][P][Q][cout] in float64 (absolute: sum |x w|, which the budget scales with)."""
    xs, w = operands(c, d, x_operand, mutant)
    if absolute:
        return conv_f64(c, [x.abs() for x in xs], w.abs())
    if mutant == "padding_before_batchnorm":             # the zero halo goes through the BatchNorm too: PReLU(shift)
        assert _xin(c) and _same3x3(c)
        edge = bn_apply(torch.zeros(1, 1, 1, c.c0p), d["in_scale"], d["in_shift"], d["in_alpha"]).double()[..., :c.c0]
        wide = edge.expand(c.N, c.H + 2, c.W + 2, c.c0).clone()
        wide[:, 1:-1, 1:-1] = xs[0]
        return conv_f64(c._replace(H=c.H + 2, W=c.W + 2, ph=0, pw=0), [wide], w)
    oy = torch.arange(c.P).view(1, -1, 1)
    ox = torch.arange(c.Q).view(1, 1, -1)
    if mutant == "right_halo_column_dropped":            # column 14 of a 14-wide tile: output column 13 (mod 14), tap s = 2
        assert not c.tr and c.S == 3 and c.stride == 1
        return conv_f64(c, xs, w, lambda r, s: None if s != 2 else (ox % 14 != 13).double().expand(1, c.P, c.Q))
    if mutant == "partial_tile_last_row_tap_above":      # the last output row reads the input one row above its taps
        assert c.P % 14 and not c.tr and c.stride == 1
        out = conv_f64(c, xs, w)
        up = [torch.cat([torch.zeros_like(x[:, :1]), x[:, :-1]], 1) for x in xs]
        out[:, c.P - 1] = conv_f64(c, up, w)[:, c.P - 1]
        return out
    if mutant == "parity_class_swapped":                 # output classes (even row, odd column) and (odd row, even column)
        assert c.tr and c.stride == 2 and c.P % 2 == 0 and c.Q % 2 == 0 and c.P == c.Q
        out = conv_f64(c, xs, w)
        a, b = out[:, 0::2, 1::2].clone(), out[:, 1::2, 0::2].clone()
        out[:, 0::2, 1::2], out[:, 1::2, 0::2] = b, a
        return out
    if mutant == "taps_not_flipped":                     # the transposed gather with the forward tap order
        assert c.tr
        return conv_f64(c, xs, w.flip(2, 3))
    if mutant == "second_segment_first_offset":
        assert len(xs) == 2
        return conv_f64(c, xs, w, segoff=[0, 0])
    if mutant == "mosaic_image_reads_neighbour":         # the first image of the partly filled last mosaic: its right
        assert (c.H, c.W, c.R, c.stride) == (7, 7, 3, 1) and c.N % 4 == 2 and not c.tr     # padding column is its neighbour's column 0
        out = conv_f64(c, xs, w)
        n = c.N - 2
        for r in range(3):
            ya = _axis(c, r, c.P, c.H, c.ph)
            out[n, _sl(ya[0], 1, ya[4]), 6] += xs[0][n + 1, _sl(ya[2], 1, ya[4]), 0] @ w[:, :, r, 2].t()
        return out
    if mutant == "one_product_lost":                     # one output element loses one product of the centre tap
        assert not c.tr and c.stride == 1 and len(xs) == 1
        out = conv_f64(c, xs, w)
        y, x, r, s = c.P // 2, c.Q // 2, c.R // 2, c.S // 2
        prod = xs[0][0, y - c.ph + r, x - c.pw + s] * w[0, :, r, s]
        prod = prod[prod != 0]
        out[0, y, x, 0] -= prod[prod.abs().argsort()[prod.numel() // 2]]        # (the median one)
        return out
    if mutant == "second_tile_of_workgroup_skipped":     # tiles 256.. of a persistent launch are never written
        tiles_per_image = cdiv(c.H, 14) * cdiv(c.W, 14)
        assert c.N * tiles_per_image > CUS and CUS % tiles_per_image == 0
        out = conv_f64(c, xs, w)
        out[CUS // tiles_per_image:] = float("nan")
        return out
    return conv_f64(c, xs, w)


def bf16r(t):
    return t.float().bfloat16().double()                 # (the values here have at most 24 significant bits: one rounding)


def half_ulp(a, dtype):
    """Half a unit in the last place of `dtype` at the magnitude a (float64 tensor); 0 where a is 0."""
    _, e = torch.frexp(a)
    bits = 9 if dtype == torch.bfloat16 else 25          # a = m * 2^e, m in [0.5, 1): ulp = 2^(e - 8) for bf16, 2^(e - 24) for f32
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), e - bits), torch.zeros_like(a))


def kterms(c):
    return c.R * c.S * (c.c0p + c.c1p) + (1 if c.dtype[0] == F32 else 0) + sum(
        1 for f in (c.bias or c.entry == "fused", c.scale, c.alpha and c.entry == "fused", c.res) if f)


def _prelu(v, alpha):
    return torch.where(v < 0, v * alpha, v)


def epilogue(c, d, acc, mag, mutant=None):
    """From the accumulator to what the call stores: dict(final = the value before the last rounding [N][P][Q][coutp],
    B = its budget, pre / preB = the value the statistics are taken from and its budget).  Pad channels come out 0."""
    co = c.cout
    ch = lambda k: d[k][:co].double()
    if mutant == "accumulator_rounded_to_bf16":
        acc = bf16r(acc)
    k = SAFETY * kterms(c) * U32
    if c.entry == "fused":
        sc = ch("scale") if c.scale else torch.ones(co, dtype=torch.float64)
        v = acc * sc + ch("bias")
        B = k * (mag * sc.abs() + ch("bias").abs())
        res_first = c.res_first if mutant != "residual_prelu_order" else 1 - c.res_first
        al = ch("alpha") if c.alpha else None
        amax = torch.maximum(al.abs(), torch.ones_like(al)) if c.alpha else 1.0
        if al is not None and not (c.res and res_first):
            v, B = _prelu(v, al), B * amax
        pre, preB = v, B
        if c.res:
            r = d["res"][..., :co].double()
            B = B + half_ulp(v.abs() + B, torch.bfloat16) + SAFETY * U32 * (v.abs() + r.abs())
            v = bf16r(v) + r                             # the residual joins the value as stored
            if al is not None and res_first:
                v, B = _prelu(v, al), B * amax
    else:
        v, B = acc, k * mag
        if c.bias:
            v, B = acc + ch("bias"), k * (mag + ch("bias").abs())
        pre, preB = v, B
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:3] + (c.coutp - co,), dtype=torch.float64)], 3) if c.coutp > co else t
    return dict(final=pad(v), B=pad(B), pre=pad(pre), preB=pad(preB))


def stored(c, final):
    """The storage-type tensor the call writes for the value `final`: round to nearest even (f2bf of csrc/common.h)."""
    return final.float().to(out_dtype(c))


def statistics(c, e, definition=STATDEF):
    """((sum, sum of squares) [2][coutp] float64, its budget) of the value the definition names."""
    v, B = e["pre"], e["preB"]
    if definition == "stored":
        v = stored(c, v).double()
    n = c.N * c.P * c.Q
    flat, fb = v.reshape(-1, c.coutp), B.reshape(-1, c.coutp)
    s = torch.stack([flat.sum(0), (flat * flat).sum(0)])
    b = torch.stack([fb.sum(0) + SAFETY * n * U32 * flat.abs().sum(0),
                     (2 * flat.abs() * fb + fb * fb).sum(0) + SAFETY * (n + 1) * U32 * (flat * flat).sum(0)])
    return s, b


def bnb_sums(c, d, dy, mutant=None):
    """((sum g, sum g*xhat, sum dy*min(z, 0)) [3][coutp] float64, budget, sum |terms|) from the STORED dX `dy`
    [N][P][Q][coutp] and the saved BatchNorm input, as bnb_accum of csrc/common.h defines them.  The budget: f32 rounding of
    every term and of `pixels` additions, and, where z is within its own f32 rounding of 0, the jump of g there."""
    cp = c.coutp
    dy = dy.double().reshape(-1, cp)
    x = d["bn_x"].double().reshape(-1, cp)
    sc, sh, mean, inv = (d[k].double() for k in ("bn_scale", "bn_shift", "bn_mean", "bn_invstd"))
    al = d["bn_alpha"].double() if d["bn_alpha"] is not None else None
    z = x * sc + sh
    zerr = 2 * U32 * ((x * sc).abs() + sh.abs())
    neg = (z <= 0) if al is not None else torch.zeros_like(z, dtype=torch.bool)
    if mutant == "bnbwd_z_positive":
        neg = (z > 0) if al is not None else neg
    g = torch.where(neg, dy * (al if al is not None else 1.0), dy)
    xh = x * inv - mean * inv
    xhm = (x * inv).abs() + (mean * inv).abs()
    q = torch.stack([g.sum(0), (g * xh).sum(0), torch.where(neg, dy * z, torch.zeros_like(z)).sum(0)])
    terms = torch.stack([g.abs().sum(0), (g.abs() * xhm).sum(0), torch.where(neg, dy.abs() * ((x * sc).abs() + sh.abs()), torch.zeros_like(z)).sum(0)])
    n = dy.shape[0]
    b = SAFETY * (n + 4) * U32 * terms
    if al is not None:
        near = z.abs() <= zerr
        jump = torch.where(near, dy.abs() * (1 + al.abs()), torch.zeros_like(z))
        b = b + torch.stack([jump.sum(0), (jump * xhm).sum(0), torch.where(near, dy.abs() * (z.abs() + zerr), torch.zeros_like(z)).sum(0)])
    return q, b, terms


def worst_ratio(got, want, bud):
    """max |got - want| / budget over the elements (an element with a zero budget must be exact; NaN counts as inf)."""
    err = (got.double() - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = torch.where(bud > 0, err / torch.where(bud > 0, bud, torch.ones_like(bud)),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


def out_allowance(c, e):
    """The error a stored element may have: its budget plus half an ulp of the storage type at |ref| + budget."""
    return e["B"] + half_ulp(e["final"].abs() + e["B"], out_dtype(c))


# ------------------------------------------------------------------------------------------------- shared references
_REF = {}


def reference(c, kind, x_operand=None):
    """(data, accumulator f64, sum |x w| f64) of a case, computed once per (shape, data, kind) and shared by the cases and
    tests that differ only in the epilogue.  x_operand: see operands()."""
    key = (c.dtype[0], _xin(c) is not None, bool(c.alpha) if _xin(c) else None) + tuple(c[5:22]) + (c.amp, kind, x_operand is not None)
    if key not in _REF:
        d = make_inputs(c, kind)
        _REF[key] = (d, accumulate(c, d, x_operand), accumulate(c, d, x_operand, absolute=True))
    d0, acc, mag = _REF[key]
    d = dict(d0)
    d.update(make_epilogue(c, kind))                    # the epilogue operands of THIS case
    return d, acc, mag


def forget():
    _REF.clear()


def d4_split(c, t):
    """msml_deconv4_bwd_data writes the 36 channels of the restated conv as two 18-of-32 tensors: (dx0, dx1)."""
    z = torch.zeros(t.shape[:3] + (14,), dtype=t.dtype)
    return torch.cat([t[..., :18], z], 3), torch.cat([t[..., 18:36], z], 3)


# ------------------------------------------------------------------------------------------------- the two checks
EPILOGUE_MUTANTS = ("residual_prelu_order", "accumulator_rounded_to_bf16")


def expect(c, kind, x_operand=None, mutant=None):
    """What a call of the case must store: dict(d = operands, final / allow = the float64 value of every output element
    before the last rounding and the error it may have, out = the stored tensor, stats / stats_b = the statistics of
    c.statdef and their budget).  With a mutant: what that wrong kernel would store."""
    d, acc, mag = reference(c, kind, x_operand)
    if mutant is not None and mutant not in EPILOGUE_MUTANTS + ("statistics_other_definition", "bnbwd_z_positive"):
        acc = accumulate(c, d, x_operand, mutant)
    e = epilogue(c, d, acc, mag, mutant)
    r = dict(d=d, final=e["final"], allow=out_allowance(c, e), out=stored(c, e["final"]))
    if c.stats:
        other = {"f32": "stored", "stored": "f32"}[c.statdef]
        r["stats"], r["stats_b"] = statistics(c, e, other if mutant == "statistics_other_definition" else c.statdef)
    if _bnb(c):
        r["bnb"] = bnb_sums(c, d, r["out"], mutant)[0]
    return r


def exact_failures(c, want, got):
    """The outputs of `got` (out: the stored tensor; stats / bnb: float64 column sums) that are not bit-equal to `want`."""
    bad = []
    if not torch.equal(got["out"].double(), want["out"].double()):        # (a NaN is equal to nothing)
        n = int((got["out"].double() != want["out"].double()).sum())
        bad.append("out: %d of %d elements differ" % (n, want["out"].numel()))
    if c.stats and not torch.equal(got["stats"], want["stats"]):
        bad.append("statistics: %s" % (got["stats"] - want["stats"]).abs().max(1).values.tolist())
    if _bnb(c) and not torch.equal(got["bnb"], want["bnb"]):
        bad.append("bnbwd sums: %s" % (got["bnb"] - want["bnb"]).abs().max(1).values.tolist())
    return bad


def budget_ratios(c, want, got):
    """Worst |error| / budget of every output; the bnbwd sums are taken from the dX that `got` itself stored."""
    r = {"out": worst_ratio(got["out"], want["final"], want["allow"])}
    if c.stats:
        r["stats"] = worst_ratio(got["stats"], want["stats"], want["stats_b"])
    if _bnb(c):
        q, b, _ = bnb_sums(c, want["d"], got["out"])
        r["bnb"] = worst_ratio(got["bnb"], q, b)
    return r


def quantum(t):
    """The largest power of two 2^-k, k <= 12, that every element of t is a multiple of."""
    for k in range(13):
        q = 2.0 ** -k
        if bool((t / q == (t / q).round()).all()):
            return q
    raise AssertionError("not a dyadic tensor")
