"""The stem convs' backward-data to the image (msml_stem_bwd_data): the case list, a numpy / float64 restatement of the
adjoint, the derived error budget and the mutants the checks must catch.  tests/test_stem_bwd_cpu.py runs the restatement
against torch.nn.grad.conv2d_input and every mutant against the budget; tests/test_gpu_stem_bwd.py runs the kernel.

    dx[n][c][iy][ix] = sum over k, r, s of dy[n][oy][ox][k] * w[k][c][r][s],   iy = oy*stride - pad + r, ix = ox*stride - pad + s

dy is NHWC storage [N][P][Q][ldy] with Cout real channels, w OIHW, dx NCHW; pad = R // 2.

Budget (derived, not measured): the kernel accumulates the T = Cout * R * S terms of an element in f32, in whatever order
(the MFMA over channels, then the taps), so |err| <= (T - 1) u sum |dy * w| to first order with u = 2^-24; the bound used
is (T + 2) * 2^-24 * sum |dy * w| (+2: the store and the second-order terms).  The operands are compared as the kernel
sees them: w rounded to bf16 when dy is bf16, unrounded when dy is f32; the products of two bf16 values are exact in f32.
With small integers every partial sum is below 2^24 and the result is exact: zero tolerance."""
import collections

import numpy as np
import torch

from msml_amd import _lib

U32 = 2.0 ** -24
BIG = 2.0 ** 100            # what the pad channels of dy hold (exact in bf16): a kernel that reads them is far off

Case = collections.namedtuple("Case", "N C H W R stride Cout ldy")


def out_size(h, r, stride):
    return (h + 2 * (r // 2) - r) // stride + 1


def band(case):
    """Input rows per workgroup of the bf16 kernel (the library's own answer: a host-side query, no GPU)."""
    b = _lib.value("msml_stem_bwd_data_band", case.C, case.H, case.W, case.Cout, case.R, case.stride)
    assert b >= 1, case
    return b


def _band_plus_one():
    # 3x3 / C = 3 / stride 1 at W = 17: H = one row band + 1 (the band of a tall image of that width)
    return band(Case(3, 3, 64, 17, 3, 1, 64, 64)) + 1


def cases():
    """The smallest shapes that reach every branch: both N, every (C, R, stride) the stems have, odd and even sizes at
    stride 2 (both parities of the last row and column), a second band of one row, several tiles per wave (the prefetch
    of a wave's next tile), the three Cout / ldy pairs, and W = 128, the limit -- there tall enough for several bands
    (stride 1 and 2, 3x3 and 5x5), the last one partial."""
    return [
        Case(1, 3, 5, 5, 3, 1, 32, 32),
        Case(3, 3, _band_plus_one(), 17, 3, 1, 64, 64),
        Case(1, 3, 7, 7, 3, 2, 96, 128),
        Case(3, 3, 8, 10, 3, 2, 64, 64),
        Case(1, 1, 9, 8, 3, 2, 32, 32),
        Case(3, 1, 6, 6, 5, 1, 96, 128),
        Case(1, 1, 12, 33, 5, 1, 64, 64),
        Case(1, 3, 13, 128, 3, 1, 64, 64),
        Case(1, 3, 37, 128, 3, 2, 32, 32),
        Case(1, 1, 17, 128, 5, 1, 96, 128),
    ]


def case_id(c):
    return "n%d_c%d_%dx%d_k%d_s%d_co%d_ld%d" % c


def _round(t, dt):
    return t.to(dt).to(torch.float64)


def exact_data(case, dt, seed=0):
    """(dy [N,P,Q,ldy] of dtype dt with BIG in the pad channels, w [Cout,C,R,R] f32): small integers."""
    g = torch.Generator().manual_seed(1000 + seed)
    p, q = out_size(case.H, case.R, case.stride), out_size(case.W, case.R, case.stride)
    dy = torch.full((case.N, p, q, case.ldy), BIG, dtype=torch.float64)
    dy[..., :case.Cout] = torch.randint(-4, 5, (case.N, p, q, case.Cout), generator=g).double()
    w = torch.randint(-3, 4, (case.Cout, case.C, case.R, case.R), generator=g).float()
    return dy.to(dt), w


def random_data(case, dt, seed=0):
    """Normal dy rounded to dt (BIG in the pad channels) and a normal f32 w."""
    g = torch.Generator().manual_seed(2000 + seed)
    p, q = out_size(case.H, case.R, case.stride), out_size(case.W, case.R, case.stride)
    dy = torch.full((case.N, p, q, case.ldy), BIG, dtype=torch.float32)
    dy[..., :case.Cout] = torch.randn(case.N, p, q, case.Cout, generator=g)
    w = 0.1 * torch.randn(case.Cout, case.C, case.R, case.R, generator=g)
    return dy.to(dt), w


def operands(dy, w):
    """(dy, w) in float64 as the kernel sees them: w rounded to bf16 exactly when dy is bf16."""
    return dy.double().numpy(), _round(w, dy.dtype if dy.dtype is torch.bfloat16 else torch.float32).numpy()


MUTANTS = ("tap_transposed", "parity_off_by_one", "pad_channel_read", "last_band_dropped")

def applies(mutant, case):
    if mutant == "parity_off_by_one":
        return case.stride == 2
    if mutant == "pad_channel_read":
        return case.ldy > case.Cout
    return True


def adjoint_f64(dy, w, case, mutant=None, absolute=False):
    """dx [N,C,H,W] float64 from dy [N,P,Q,ldy] and w [Cout,C,R,R] (numpy float64); absolute=True: sum |dy * w|, the
    magnitude the budget scales with.  mutant: one of MUTANTS, a wrong kernel."""
    n, c, h, wd, r_, stride, cout, ldy = case
    pad = r_ // 2
    p, q = out_size(h, r_, stride), out_size(wd, r_, stride)
    assert dy.shape == (n, p, q, ldy) and w.shape == (cout, c, r_, r_)
    d = dy[..., :cout]
    if mutant == "pad_channel_read":                 # the channel loop runs to ldy, the filter row wraps around
        d = dy
        w = w[np.arange(ldy) % cout]
    if absolute:
        d, w = np.abs(d), np.abs(w)
    dx = np.zeros((n, c, h, wd), np.float64)
    shift = 1 if mutant == "parity_off_by_one" else 0
    for r in range(r_):
        for s in range(r_):
            wt = w[:, :, s, r] if mutant == "tap_transposed" else w[:, :, r, s]
            t = np.einsum("npqk,kc->ncpq", d, wt)
            iy = np.arange(p) * stride - pad + r + shift
            ix = np.arange(q) * stride - pad + s + shift
            oky, okx = (iy >= 0) & (iy < h), (ix >= 0) & (ix < wd)
            dx[np.ix_(range(n), range(c), iy[oky], ix[okx])] += t[:, :, oky][:, :, :, okx]
    if mutant == "last_band_dropped":
        b = band(case)
        dx[:, :, (h - 1) // b * b:] = 0.0
    return dx


def budget(mag, case):
    return (case.Cout * case.R * case.R + 2) * U32 * mag


def worst_ratio(got, want, mag, case):
    """max |got - want| / budget over the elements (an element with a zero budget must be exact)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    bud = budget(mag, case)
    ratio = np.where(bud > 0, err / np.where(bud > 0, bud, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())
