"""Shared by tests/test_head_cpu.py and tests/test_gpu_head.py: the case tables of the kernels between the embedding and
the weight update (msml_amd/csrc/head.hip, msml_transpose of layout.hip, msml_gemm_splitk of conv_wgrad.hip), float64
references, derived error budgets, a torch restatement of the kernels' f32 arithmetic (with single-fault mutants) and the
checks that compare ANY implementation of the entry points -- the restatement on the CPU, the library on the GPU -- with
the reference.  Conventions, U32 / UBF / U64 / SAFETY, f32() and the Report are those of tests/bn_cases.py.

References (f64, on exactly the operands the kernel receives; `float` parameters after an f32 round trip):
  rownorm        y = w / max(||w||, 1e-12);  dw = (dy - y <y, dy>) * inv  with the inv the caller hands over
  margin         Arc: s cos(theta + m - k (theta - a)), Cos: s (c - m + k (theta - a)), theta = acos c; other columns
                 s c; label -1: no target.  d logit / d cos by torch autograd in f64 through that expression.
  pfc            row max and sum exp(logit - max) over the C valid columns (compared as max and log-sum-exp: rowsum alone
                 is not unique); p = exp(l - gmax) / gsum, y = 0.9 at the target and 0.1 / (C - 1) elsewhere on rows with
                 a local target, dlogit = (p - y) inv_n, dcos = dlogit x the autograd factor, ptarget = p at the target or 0
  transpose      exact;  gemm_splitk: f64 GEMM of the bf16 operands;  sgd: g = grad coef + wd w, buf = first ? g :
                 mu buf + g, w -= lr buf;  grad_norm_clip: norm = scale sqrt(sum g^2), (norm, scale min(1, max / (norm + 1e-6)))

Budgets.  k * u32 * (sum of the magnitudes of the terms) + u_store * |ref|, k counted from the expression written next
to it; sums use n_chain * u32 * sum |term| with n_chain the longest f32 chain of the launch, from the launch geometry
restated here from the grid rules head.hip documents.  SAFETY = 2 multiplies every budget, nothing else does.
  1 - c^2.  margin_target computes 1 - c * c in f32; its relative error u32 (1 + c^2) / (1 - c^2) enters the budget of
  the derivative as that conditioning term.  The tables draw target cosines with (1 + c^2) / (1 - c^2) <= 2^10, i.e.
  |c| <= sqrt(1023 / 1025) = 0.99902391; they use CMAX = 1 - 2^-10 = 0.99902344.  Planted targets c = +-1 exactly check
  the forward value only (their derivative is infinite in the reference): the excused elements are counted and the
  count is asserted to equal the number planted.
  Library functions.  No ulp table of the device math library ships with the ROCm install (only its bitcode), so the
  bounds are the worst error of torch's CPU f32 function against f64 over the ranges the cases reach (measure_libm),
  x LIBM_FACTOR = 4 for the different implementation.  Measured (units of u32 = 2^-24 relative to the result):
  LIBM_MEASURED below; tests/test_head_cpu.py repeats the measurement.  __expf(x) additionally gets |x| u32 (argument scaling).
  Underflow.  A product, an exponential or a stored value (f32 and bf16 share the exponent range) below the normal range
  may lose FLT_MIN = 2^-126 absolutely (flushed, or rounded on the denormal grid); sums of n such terms get n * FLT_MIN.
  With s = 64 the probabilities of a 85 742-column row reach far below 2^-126, so the dcos budgets carry one FLT_MIN per
  product and one for the store.
"""
import math
import zlib

import torch
import torch.nn.functional as F

from tests.bn_cases import DT, SAFETY, U32, U64, UBF, Report, f32, u_store  # noqa: F401  (re-exported)

FLT_MIN = 2.0 ** -126
EPS_NORM = 1e-12
EPS_CLIP = 1e-6
CMAX = 1.0 - 2.0 ** -10
LIBM_FACTOR = 4.0
# worst |f32 function - f64 function| / (u32 |f64 function|) of torch's CPU kernels over measure_libm()'s ranges
LIBM_MEASURED = {"acos": 1.49, "cos": 1.09, "sin": 1.09, "sqrt": 1.05, "exp": 1.02, "tanh": 1.07, "log": 1.02}
ARC, COS = 0, 1
S = 64.0
M_OF = {ARC: 0.5, COS: 0.4}
AKS = ((0.0, 0.0), (1.2, 0.1))
EPS_LS = 0.1
GUARD_ROWS = 3


def L(fn):
    """Relative bound of a library function in units of u32."""
    return LIBM_FACTOR * LIBM_MEASURED[fn]


def measure_libm():
    """{fn: worst relative error in units of u32} of torch's CPU f32 functions over the ranges the cases reach."""
    n = 1 << 20
    g = torch.linspace(0.0, 1.0, n, dtype=torch.float64)
    rng = {"acos": ((2.0 * g - 1.0) * CMAX, torch.acos), "cos": (g * (math.pi + 1.0), torch.cos),
           "sin": (g * (math.pi + 1.0), torch.sin), "sqrt": (g * 4.0 + 2.0 ** -20, torch.sqrt),
           "exp": (-87.0 * g, torch.exp),
           # tests/ew_cases.py: the FM masks over [-12, 12], log(1 + exp(-|l0 - l1|)) of the segmentation loss over [1, 2]
           "tanh": ((2.0 * g - 1.0) * 12.0, torch.tanh), "log": (1.0 + g, torch.log)}
    out = {}
    for fn, (x, f) in rng.items():
        x32 = x.float()
        ref = f(x32.double())
        ok = ref.abs() > 2.0 ** -20              # relative error next to a zero of cos / sin is not what the bound is about
        out[fn] = float((((f(x32).double() - ref).abs() / ref.abs())[ok] / U32).max())
    return out


def kpad(k):
    return (k + 31) // 32 * 32


def w64(t):
    return None if t is None else t.double()


class Case:
    def __init__(self, name, kind="normal", dtype="f32", **p):
        self.name, self.kind, self.dtype, self.p = name, kind, dtype, p

    def __getattr__(self, k):
        try:
            return self.p[k]
        except KeyError:
            raise AttributeError(k)

    def gen(self, salt=0):
        return torch.Generator().manual_seed(zlib.crc32(self.name.encode()) + salt)


def with_dtype(case, dt):
    c = Case(case.name + "-" + dt, case.kind, dt, **case.p)
    return c


# ------------------------------------------------------------------------------------------------------ geometry
def cdiv(a, b):
    return -(-a // b)


def rownorm_v8(E, ld, aligned=True):
    return E % 512 == 0 and E <= 1024 and ld == E and aligned


def rownorm_chain(E, v8):
    """f32 adds behind one element of a row sum: a lane's own chain + the six wave_sum levels."""
    return (E // 64 if v8 else cdiv(E, 64)) + 6


def rowstats_v4(ld, aligned=True):
    return ld % 4 == 0 and aligned


def sgd_grid(n):
    return min(max(cdiv(n // 4, 256), 1), 4096)


def sumsq_rows(n):
    return min(cdiv(n, 256), 1024)


def sumsq_chain(n):
    """k_sumsq: iterations that feed s0 (unrolled + remainder) x (3 adds inside a float4 + 1 accumulate) + 1 product + the
    tail element + (s0 + s1) + (s2 + s3) + six wave levels + three adds of the block fold."""
    stride = sumsq_rows(n) * 256
    cnt = cdiv(n // 4, stride)
    return 4 * (cnt // 4 + cnt % 4) + 1 + 1 + 2 + 6 + 3


# ------------------------------------------------------------------------------------------------- margin: reference
def margin_expr(c, kind, s, m, a, k):
    th = torch.acos(c)
    if kind == ARC:
        return s * torch.cos(th + m - k * (th - a))
    return s * (c - m + k * (th - a))


def margin_params(kind, ak):
    return f32(S), f32(M_OF[kind]), f32(ak[0]), f32(ak[1])


def margin_target_reference(ct, kind, s, m, a, k):
    """(logit, d logit / d cos) of target cosines ct (f64), the derivative by autograd."""
    c = ct.clone().requires_grad_(True)
    out = margin_expr(c, kind, s, m, a, k)
    (d,) = torch.autograd.grad(out.sum(), c)
    return out.detach(), d


def margin_target_budget(ct, kind, s, m, a, k):
    """Budgets of margin_target()'s two results for target cosines ct (f64)."""
    th = torch.acos(ct)
    dth = L("acos") * U32 * th                                                    # theta = acosf(c)
    q = 1.0 - ct * ct
    den = torch.sqrt(q.clamp_min(1e-300))
    # dth = -1 / sqrtf(1 - c * c): the conditioning term of 1 - c * c (module text), sqrtf, the division: 1 op
    rel_dth = ((1.0 + ct * ct) / q.clamp_min(1e-300) + L("sqrt") + 1) * U32
    if kind == ARC:
        phi = th + m - k * (th - a)
        # phi = theta + m - k * (theta - a): 4 ops on |theta| + |m| + |k| (|theta| + |a|)
        dphi = (1.0 + abs(k)) * dth + 4 * U32 * (th + abs(m) + abs(k) * (th + abs(a)))
        out = s * torch.cos(phi)
        dout = s * dphi + (L("cos") + 1) * U32 * out.abs()                        # s * cosf(phi): 1 op
        d = s * torch.sin(phi) * (1.0 - k) / den
        # -s * sinf(phi) * (1 - k) * dth: 4 ops
        dd = (s * abs(1.0 - k) / den) * dphi + d.abs() * ((L("sin") + 4) * U32 + rel_dth)
    else:
        # s * (c - m + k * (theta - a)): 5 ops on |c| + |m| + |k| (|theta| + |a|)
        dout = s * abs(k) * dth + 5 * U32 * s * (ct.abs() + abs(m) + abs(k) * (th + abs(a)))
        # s * (1 + k * dth): 3 ops on 1 + |k dth|
        dd = s * (abs(k) / den) * rel_dth + 3 * U32 * s * (1.0 + abs(k) / den)
    return dout, dd


def margin_reference(cos, label, C, kind, s, m, a, k):
    """logits [N][C], their budget, d logit / d cos [N][C] and its budget, the target cosines [N] (0 without a target),
    the mask of planted targets (|c| == 1: derivative excused)."""
    c = w64(cos[:, :C])
    N = c.shape[0]
    logits, dl = s * c, U32 * (s * c).abs()                                       # s * c: 1 op
    d = torch.full_like(c, s)
    dd = torch.zeros_like(c)
    rows = (label >= 0).nonzero().flatten()
    ct = torch.zeros(N, dtype=torch.float64, device=c.device)
    excused = torch.zeros_like(c, dtype=torch.bool)
    if rows.numel():
        y = label[rows]
        t = c[rows, y]
        ct[rows] = t
        planted = t.abs() == 1.0
        safe = torch.where(planted, torch.zeros_like(t), t)
        out, dt = margin_target_reference(t, kind, s, m, a, k)
        bo, _ = margin_target_budget(t, kind, s, m, a, k)
        _, bd = margin_target_budget(safe, kind, s, m, a, k)
        logits[rows, y], dl[rows, y] = out, bo
        d[rows, y] = torch.where(planted, torch.zeros_like(dt), dt)
        dd[rows, y] = torch.where(planted, torch.zeros_like(bd), bd)
        excused[rows, y] = planted
    return {"logits": logits, "dl": dl, "d": d, "dd": dd, "ct": ct, "excused": excused}


# -------------------------------------------------------------------------------------------------------- drawing
def draw_labels(case, N, C, g):
    lab = torch.randint(0, C, (N,), generator=g)
    mode = case.p.get("labels", "mixed")
    if mode == "allneg":
        return torch.full((N,), -1, dtype=torch.int64)
    if N == 1:
        lab[0] = (0, C - 1, -1)[zlib.crc32(case.name.encode()) % 3]
        return lab
    lab[0], lab[1] = 0, C - 1
    lab[2::3] = -1
    return lab


def draw_cos(case, device="cpu"):
    """cos [N][ld] f32 (columns C..ld NaN), labels, dlogit [N][ld] f32 (columns C..ld NaN)."""
    N, C, ld = case.N, case.C, case.ld
    g = case.gen()
    spread = case.p.get("spread", "normal")
    if spread == "wide":
        cos = (torch.rand(N, ld, generator=g) * 2.0 - 1.0) * CMAX
        cos[:, 0] = CMAX
        if C > 2:
            cos[:, C // 2] = -CMAX
    elif spread == "narrow":
        cos = 0.1 * torch.randn(N, ld, generator=g)
    else:
        cos = 0.3 * torch.randn(N, ld, generator=g)
    cos = cos.clamp(-CMAX, CMAX)
    lab = draw_labels(case, N, C, g)
    rows = (lab >= 0).nonzero().flatten()
    if spread == "narrow" and rows.numel():                    # every other labelled row: the target is the row max
        top = rows[::2]
        cos[top, lab[top]] = 0.95
    planted = 0
    if case.p.get("planted") and rows.numel() >= 2:
        cos[rows[0], lab[rows[0]]], cos[rows[1], lab[rows[1]]] = 1.0, -1.0
        planted = 2
    dlogit = torch.randn(N, ld, generator=g)
    cos[:, C:] = float("nan")
    dlogit[:, C:] = float("nan")
    return cos.to(device), lab.to(device), dlogit.to(device), planted


# ------------------------------------------------------------------------------------------------------ case tables
CS_MARGIN = (1, 2, 255, 256, 257, 16384, 16385, 32768, 32769, 85742)
CS_ROWSTATS = CS_MARGIN + (3, 4, 5, 37, 63, 4096, 4097)


def margin_cases():
    """margin_fwd / margin_bwd / gather_target / pfc_grad (C > 1)."""
    out = []
    for C in CS_MARGIN:
        for ld in sorted({C, kpad(C)}):
            for ni, N in enumerate((1, 9, 256)):
                for kind in (ARC, COS):
                    for ak in AKS:
                        out.append(Case("margin-C%d-ld%d-N%d-%s-a%g" % (C, ld, N, "arc" if kind == ARC else "cos", ak[0]),
                                        N=N, C=C, ld=ld, ldo=(kpad(C), C)[(ni + kind) % 2], kind_=kind, ak=ak,
                                        planted=(N == 9 and C >= 255)))
    for C in (257, 16385):
        for kind in (ARC, COS):
            out.append(Case("margin-allneg-C%d-%d" % (C, kind), N=9, C=C, ld=kpad(C), ldo=kpad(C), kind_=kind, ak=AKS[1],
                            labels="allneg"))
    return out


def rowstats_cases():
    out = []
    for C in CS_ROWSTATS:
        for i, ld in enumerate(sorted({C, C + 1 if (C + 1) % 4 else C + 2, kpad(C)})):
            for spread in ("normal", "narrow", "wide"):
                kind = (ARC, COS)[(i + len(out)) % 2]
                ak = AKS[(len(out) // 2) % 2]
                N = 256 if (C == 85742 and ld == kpad(C) and spread == "normal") else 9
                out.append(Case("rowstats-C%d-ld%d-%s-%d-a%g" % (C, ld, spread, kind, ak[0]), N=N, C=C, ld=ld, kind_=kind,
                                ak=ak, spread=spread))
    out.append(Case("rowstats-allneg", N=9, C=257, ld=288, kind_=ARC, ak=AKS[1], labels="allneg"))
    return out


ROWNORM_ES = (1, 64, 320, 512, 1024, 1536)


def rownorm_cases():
    out = []
    for E in ROWNORM_ES:
        for R, Rp in ((301, 320), (7, 7), (2, 9)):
            for ld in sorted({E, kpad(E), E + 8}):
                out.append(Case("rownorm-E%d-R%d-Rp%d-ld%d" % (E, R, Rp, ld), R=R, Rp=Rp, E=E, ld=ld, misalign=False))
    out.append(Case("rownorm-E512-misaligned", R=301, Rp=320, E=512, ld=512, misalign=True))
    out.append(Case("rownorm-E1024-misaligned", R=7, Rp=8, E=1024, ld=1024, misalign=True))
    return out


TRANSPOSE_SHAPES = ((1, 1), (63, 65), (64, 64), (301, 512), (85742, 512))
GEMM_SHAPES = tuple((M, K) for M in (32, 100, 256) for K in (64, 2048, 85760))
# 1024 * 4096 + 3: n / 4 equals the 4096 x 256 threads of the capped grid (one full trip + the tail); the last one takes
# a second and a partial third grid-stride trip
SGD_NS = (1, 3, 4, 5, 1023, 1024 * 4096 + 3, 4 * (2 * 4096 * 256 + 5) + 3)
SGD_VARIANTS = ((1, 0.9, 5e-4, None), (0, 0.9, 5e-4, 0.37), (0, 0.0, 5e-4, None), (0, 0.9, 0.0, 0.37), (1, 0.9, 5e-4, 0.37))
NORM_NS = (1, 3, 5, 1024, 262144 - 1, 262144, 262144 * 4 * 4 + 7)


# ---------------------------------------------------------------------------------------------------- the checks
def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_rownorm_case(be, case, rep, device="cpu"):
    R, Rp, E, ld = case.R, case.Rp, case.E, case.ld
    g = case.gen()
    wt = 0.3 * torch.randn(R, E, generator=g)
    wt[R // 2] = 0.0                                            # an all-zero row
    if R > 1:
        wt[R - 1] = wt[R - 1] * (1e-20 / max(float(wt[R - 1].double().norm()), 1e-30))   # a row of norm ~1e-20
    wt = wt.to(device)
    eps = f32(EPS_NORM)
    wd = w64(wt)
    ss = (wd * wd).sum(1)
    norm = torch.sqrt(ss)
    inv = 1.0 / norm.clamp_min(eps)
    y = wd * inv[:, None]
    for dt in ("f32", "bf16"):
        c = with_dtype(case, dt)
        v8 = rownorm_v8(E, ld, not case.misalign)
        chain = rownorm_chain(E, v8)
        # ss += p * p: chain adds + 1 product, E products that may underflow; sqrtf; 1 / fmaxf(., eps): 1 op
        dss = (chain + 1) * U32 * ss + E * FLT_MIN
        hi = torch.sqrt(ss + dss) * (1.0 + L("sqrt") * U32)
        lo = torch.sqrt((ss - dss).clamp_min(0.0)) * (1.0 - L("sqrt") * U32)
        dinv = torch.maximum(1.0 / lo.clamp_min(eps) - inv, inv - 1.0 / hi.clamp_min(eps)) + U32 * inv
        dst, invk = be.rownorm_fwd(wt, Rp, ld, DT[dt], misalign=case.misalign)
        key = "rownorm_fwd"
        rep.check(key, "inv_norm", invk, inv, dinv, c)
        rep.check(key, "y", dst[:R, :E], y, wd.abs() * dinv[:, None] + U32 * y.abs() + u_store(DT[dt]) * y.abs() + 2 * FLT_MIN, c)   # p * inv: 1 op; product and store may underflow
        rep.exact(key, "columns E..ld", dst[:R, E:], torch.zeros(R, ld - E, device=dst.device), c)
        rep.exact(key, "rows R..Rp", dst[R:], torch.zeros(Rp - R, ld, device=dst.device), c)
        rep.exact(key, "zero row y", dst[R // 2, :E], torch.zeros(E, device=dst.device), c)
        rep.exact(key, "zero row inv", invk[R // 2].double(), torch.tensor(1.0 / eps, device=dst.device).float().double(), c)
    # backward: inv as the caller hands it over (the f32 rounding of the reference's), dy with ldy >= E
    c = with_dtype(case, "f32")
    inv32 = inv.float()
    i64 = inv32.double()
    for ldy in sorted({E, kpad(E) + 4}):
        dy = torch.randn(R, ldy, generator=g).to(device)
        dy[:, E:] = float("nan")
        gy = w64(dy[:, :E])
        yy = wd * i64[:, None]
        t = yy * gy
        dot = t.sum(1)
        v8 = rownorm_v8(E, E) and ldy % 4 == 0
        chain = rownorm_chain(E, v8)
        ddot = (chain + 2) * U32 * t.abs().sum(1)                                # dot += p * inv * g: chain adds + 2 products
        v = (gy - yy * dot[:, None]) * i64[:, None]
        # (g - p * inv * dot) * inv: 3 ops on |g| + |y dot| inside, the outer product: 1 op
        bv = i64[:, None] * (yy.abs() * ddot[:, None] + 3 * U32 * (gy.abs() + (yy * dot[:, None]).abs())) + U32 * v.abs()
        for accumulate in (0, 1):
            dw0 = torch.randn(R, E, generator=g).to(device)
            dw = be.rownorm_bwd(wt, inv32, dy, E, accumulate, dw0)
            ref = v + (w64(dw0) if accumulate else 0.0)
            rep.check("rownorm_bwd", "dw ldy=%d acc=%d" % (ldy, accumulate), dw, ref, bv + (U32 * ref.abs() if accumulate else 0.0), c)


def rownorm_reference_for_autograd(wt):
    """The two formulas check_rownorm_case uses, for the comparison with F.normalize + autograd."""
    norm = torch.sqrt((wt * wt).sum(1))
    inv = 1.0 / norm.clamp_min(EPS_NORM)
    y = wt * inv[:, None]
    return y, inv, lambda dy: (dy - y * (y * dy).sum(1)[:, None]) * inv[:, None]


def check_margin_case(be, case, rep, device="cpu"):
    """msml_gather_target, msml_margin_fwd, msml_margin_bwd (both storage types).  Returns (planted, excused)."""
    N, C, ld, ldo, kind = case.N, case.C, case.ld, case.ldo, case.kind_
    s, m, a, k = margin_params(kind, case.ak)
    cos, lab, dlogit, planted = draw_cos(case, device)
    r = margin_reference(cos, lab, C, kind, s, m, a, k)
    c = with_dtype(case, "f32")
    ct = be.gather_target(cos, lab)
    rep.exact("gather_target", "cos_t", ct, r["ct"], c)
    out = be.margin_fwd(cos, lab, C, kind, s, m, a, k)
    rep.check("margin_fwd", "logits", out[:, :C], r["logits"], r["dl"], c)
    if ld > C and not _bits_equal(out[:, C:], cos[:, C:]):
        rep.failures.append(("margin_fwd", "columns C..ld touched", c.name, float("inf")))
    gl = w64(dlogit[:, :C])
    ref = gl * r["d"]
    ex = r["excused"]
    excused = int(ex.sum())
    for dt in ("f32", "bf16"):
        c = with_dtype(case, dt)
        dcos = be.margin_bwd(dlogit, lab, ct, C, ldo, kind, s, m, a, k, DT[dt])
        got = torch.where(ex, torch.zeros_like(ref), dcos[:, :C].double())
        # g * d: 1 op; the product and the store may underflow
        rep.check("margin_bwd", "dcos", got, ref, gl.abs() * r["dd"] + U32 * ref.abs() + u_store(DT[dt]) * ref.abs() + 2 * FLT_MIN, c)
        rep.exact("margin_bwd", "columns C..ldo", dcos[:, C:], torch.zeros(N, ldo - C, device=dcos.device), c)
    return planted, excused


def pfc_reference(cos, lab, C, kind, s, m, a, k):
    r = margin_reference(cos, lab, C, kind, s, m, a, k)
    lg = r["logits"]
    mx = lg.max(1)[0]
    r["max"], r["sum"] = mx, torch.exp(lg - mx[:, None]).sum(1)
    r["lse"] = mx + torch.log(r["sum"])
    return r


def rowstats_budget(r, C, v4):
    """(budget of the row max, budget of max + log(sum))."""
    lg, dl = r["logits"], r["dl"]
    dmax = dl.max(1)[0]
    X = (lg.max(1)[0] - lg.min(1)[0]) + 2.0 * dmax                                # largest |l - max| of a row
    trips = cdiv(C, 4096) if v4 else cdiv(C, 256)
    adds = trips + (3 + 6 + 16 if v4 else 6 + 4)          # a thread's chain (+ 3 inside a float4) + wave levels + LDS fold
    rescales = trips + 2                                  # of a thread, then one per wave, one per workgroup
    # a term: l - mx (1 op: |x| u32 in the exponent), __expf (L + |x|); every rescale: __expf (L) and 1 product; the
    # |x| parts of the rescales of one level telescope to at most X: three levels; the store: 1 op
    rel = (adds + rescales * (L("exp") + 1) + L("exp") + 2.0 * X + 3.0 * X + 1) * U32 + C * FLT_MIN
    return dmax, dmax + rel


def check_rowstats_case(be, case, rep, device="cpu", count=None):
    N, C, ld, kind = case.N, case.C, case.ld, case.kind_
    s, m, a, k = margin_params(kind, case.ak)
    cos, lab, _, _ = draw_cos(case, device)
    r = pfc_reference(cos, lab, C, kind, s, m, a, k)
    c = with_dtype(case, "f32")
    if count is not None:
        rows = (lab >= 0).nonzero().flatten()
        if rows.numel():
            top = r["logits"][rows, lab[rows]] >= r["max"][rows]
            count["target_is_max"] += int(top.sum())
            count["target_not_max"] += int((~top).sum())
    res = {}
    for scalar in ((False, True) if ld % 4 == 0 else (True,)):
        v4 = not scalar
        bmax, blse = rowstats_budget(r, C, v4)
        rm, rs = be.pfc_rowstats(cos, C, lab, kind, s, m, a, k, misalign=scalar and ld % 4 == 0)
        key = "pfc_rowstats(16B)" if v4 else "pfc_rowstats(scalar)"
        rep.check(key, "rowmax", rm, r["max"], bmax, c)
        ok = bool(torch.isfinite(rs).all()) and bool((rs > 0).all())
        lse = rm.double() + torch.log(rs.double()) if ok else torch.full_like(r["lse"], float("nan"))
        rep.check(key, "max + log(sum)", lse, r["lse"], blse, c)
        res[v4] = (lse, blse)
    if len(res) == 2 and bool(torch.isfinite(res[True][0]).all()) and bool(torch.isfinite(res[False][0]).all()):
        rep.check("pfc_rowstats(16B vs scalar)", "max + log(sum)", res[True][0], res[False][0], res[True][1] + res[False][1], c)


def check_pfc_grad_case(be, case, rep, device="cpu"):
    """msml_pfc_grad with the global (gmax, gsum) a larger job would hand over.  Returns (planted, excused)."""
    N, C, ld, ldo, kind = case.N, case.C, case.ld, case.ldo, case.kind_
    s, m, a, k = margin_params(kind, case.ak)
    cos, lab, _, planted = draw_cos(case, device)
    r = pfc_reference(cos, lab, C, kind, s, m, a, k)
    odd = (torch.arange(N, device=cos.device) % 2).double()
    gmax = (r["max"] + odd).float()                      # rows of another rank may hold the global max
    gsum = (torch.exp(r["logits"] - gmax.double()[:, None]).sum(1) * (1.0 + odd)).float()
    eps_ls, inv_n = f32(EPS_LS), f32(1.0 / (3 * N))
    x = r["logits"] - gmax.double()[:, None]
    p = torch.exp(x) / gsum.double()[:, None]
    # __expf(l - M) * (1 / gsum): the budget of l, l - M (|x| u32), __expf (L + |x|), 1 / gsum and the product: 2 ops
    dp = p * (r["dl"] + (L("exp") + 2.0 * x.abs() + 2) * U32) + FLT_MIN / gsum.double()[:, None]
    has = (lab >= 0).double()[:, None]
    tgt = has * (eps_ls / (C - 1.0)) * torch.ones_like(p)
    rows = (lab >= 0).nonzero().flatten()
    pt = torch.zeros(N, dtype=torch.float64, device=cos.device)
    dpt = torch.zeros_like(pt)
    if rows.numel():
        tgt[rows, lab[rows]] = 1.0 - eps_ls
        pt[rows], dpt[rows] = p[rows, lab[rows]], dp[rows, lab[rows]]
    ref = (p - tgt) * inv_n * r["d"]
    # (prob - tgt) * inv_n * d: tgt itself 1 op, the difference 1 op on |p| + |tgt|, two products; each product and the
    # store may underflow
    bud = inv_n * r["d"].abs() * (dp + U32 * tgt + U32 * (p + tgt)) + ((p - tgt) * inv_n).abs() * r["dd"] + 2 * U32 * ref.abs() + \
        3 * FLT_MIN
    ex = r["excused"]
    for dt in ("f32", "bf16"):
        c = with_dtype(case, dt)
        dcos, ptk = be.pfc_grad(cos, C, lab, kind, s, m, a, k, gmax, gsum, eps_ls, inv_n, ldo, DT[dt])
        got = torch.where(ex, torch.zeros_like(ref), dcos[:, :C].double())
        rep.check("pfc_grad", "dcos", got, ref, bud + u_store(DT[dt]) * ref.abs(), c)
        rep.exact("pfc_grad", "columns C..ldo", dcos[:, C:], torch.zeros(N, ldo - C, device=dcos.device), c)
        rep.check("pfc_grad", "ptarget", ptk, pt, dpt + U32 * pt, c)
        if rows.numel() < N:
            none = (lab < 0).nonzero().flatten()
            rep.exact("pfc_grad", "ptarget of label -1", ptk[none], torch.zeros(none.numel(), device=ptk.device), c)
    return planted, int(ex.sum())


def check_transpose(be, R, C, ld_s, ld_d, dt, rep, device="cpu"):
    c = Case("transpose-%dx%d-lds%d-ldd%d" % (R, C, ld_s, ld_d), dtype=dt)
    g = c.gen()
    src = torch.randn(R, ld_s, generator=g).to(DT[dt]).to(device)
    full = be.transpose(src, C, ld_d, DT[dt])                   # [GUARD_ROWS + C + GUARD_ROWS][ld_d], pre-filled with 7
    G = GUARD_ROWS
    rep.exact("transpose", "dst[c][r]", full[G:G + C, :R], src[:, :C].t(), c)
    rep.exact("transpose", "rows R..ld_d", full[G:G + C, R:], torch.zeros(C, ld_d - R, device=full.device), c)
    rep.exact("transpose", "guard rows", torch.cat([full[:G], full[G + C:]]), torch.full((2 * G, ld_d), 7.0, device=full.device), c)


def check_gemm(be, M, K, rep, device="cpu"):
    c = Case("gemm-M%d-K%d" % (M, K), dtype="bf16")
    g = c.gen()
    a = (0.5 * torch.randn(M, K, generator=g)).bfloat16().to(device)
    wp = (0.05 * torch.randn(512, K, generator=g)).bfloat16().to(device)
    out = be.gemm_splitk(a, wp)
    ref = a.double() @ wp.double().t()
    rep.check("gemm_splitk", "out", out, ref, K * U32 * (a.double().abs() @ wp.double().abs().t()), c)   # K products and adds


def sgd_reference(wt, grad, buf, lr, mu, wd, first, coef):
    g = w64(grad) * coef + wd * w64(wt)
    b = g if first else mu * w64(buf) + g
    return w64(wt) - lr * b, b


def check_sgd(be, n, variant, rep, device="cpu"):
    first, mu, wd, coef = variant
    c = Case("sgd-n%d-first%d-mu%g-wd%g-coef%s" % (n, first, mu, wd, coef), dtype="f32")
    g = c.gen()
    wt, grad, buf = (torch.randn(n, generator=g).to(device) for _ in range(3))
    lr, mu, wd = f32(0.1), f32(mu), f32(wd)
    cf = 1.0 if coef is None else f32(coef)
    w2, b2 = be.sgd(wt, grad, buf, lr, mu, wd, first, None if coef is None else torch.tensor([coef], device=device))
    rw, rb = sgd_reference(wt, grad, buf, lr, mu, wd, first, cf)
    gr = w64(grad) * cf + wd * w64(wt)
    dg = 3 * U32 * ((w64(grad) * cf).abs() + (wd * w64(wt)).abs())                # grad * coef + wd * w: 3 ops
    db = dg if first else dg + 2 * U32 * ((mu * w64(buf)).abs() + gr.abs())      # mu * buf + g: 2 ops
    dw = lr * db + 2 * U32 * (w64(wt).abs() + (lr * rb).abs())                    # w - lr * b: 2 ops
    rep.check("sgd_momentum", "buf", b2, rb, db, c)
    rep.check("sgd_momentum", "w", w2, rw, dw, c)
    return w2, b2


def norm_reference(g, max_norm, scale):
    norm = scale * torch.sqrt((w64(g) ** 2).sum())
    return norm, scale * torch.clamp(max_norm / (norm + f32(EPS_CLIP)), max=1.0)


def check_norm_clip(be, n, above, scale, rep, device="cpu"):
    c = Case("norm-n%d-%s-scale%g" % (n, "above" if above else "below", scale), dtype="f32")
    g = torch.randn(n, generator=c.gen()).to(device)
    scale = f32(scale)
    n0 = float(torch.sqrt((w64(g) ** 2).sum())) * scale
    max_norm = f32(n0 * (0.5 if above else 2.0))
    out = be.grad_norm_clip(g, max_norm, scale)
    norm, coef = norm_reference(g, max_norm, scale)
    # sqrt of an all-positive sum: half its relative error; (float)sqrt and * scale: 2 ops; the f64 fold of the rows
    dn = norm * ((sumsq_chain(n) / 2.0 + 2) * U32 + (sumsq_rows(n) + 16) * U64)
    cc = max_norm / (norm + f32(EPS_CLIP))
    # max_norm / (norm + 1e-6f): 2 ops; min(1, .) does not amplify; * scale: 1 op
    dc = scale * cc * (dn / (norm + f32(EPS_CLIP)) + 2 * U32) + U32 * coef
    rep.check("grad_norm_clip", "norm", out[0], norm, dn, c)
    rep.check("grad_norm_clip", "coef", out[1], coef, dc, c)
    return out


# ------------------------------------------------------------------------- torch restatement of the kernels' arithmetic
MUTANTS = {   # name -> (key, what) of the check that must catch it
    "smooth_denominator_C": ("pfc_grad", "dcos"),
    "smooth_on_label_minus_1": ("pfc_grad", "dcos"),
    "ptarget_unwritten_minus_1": ("pfc_grad", "ptarget"),
    "rescale_dropped": ("pfc_rowstats", "max + log(sum)"),
    "pad_in_rowstats": ("pfc_rowstats", "rowmax"),
    "ldo_not_zeroed": ("margin_bwd", "columns C..ldo"),
    "minus_1_hits_last_column": ("margin_fwd", "logits"),
    "k_sign_flipped": ("margin_bwd", "dcos"),
    "sgd_first_ignored": ("sgd_momentum", "buf"),
    "sgd_tail_skipped": ("sgd_momentum", "buf"),
    "sumsq_tail_skipped": ("grad_norm_clip", "norm"),
    "clip_not_capped": ("grad_norm_clip", "coef"),
    "scale_not_on_coef": ("grad_norm_clip", "coef"),
}

_XOR = {o: torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)}


def _wave_sum(v):
    """wave_sum(): the xor butterfly over the last dimension (64 lanes); every lane ends with the same bits."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _XOR[o]]
    return v[..., 0]


def _t32(v):
    return torch.tensor(v, dtype=torch.float32)


class Restatement:
    """The entry points in torch: f32 operations in the kernels' order, the same kernel choice, trip structure, online
    rescale order, tail handling and zero fill.  `mutant` plants one fault (MUTANTS).  CPU tensors."""
    name = "restatement"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mut = mutant

    # ---- rownorm
    @staticmethod
    def _row_sum(t, v8):
        """t [R][E] f32 terms -> the kernels' row sums."""
        R, E = t.shape
        if v8:                                        # lane holds 8 contiguous values of each 512-wide piece
            q = t.view(R, E // 512, 64, 8)
            acc = torch.zeros(R, 64)
            for ch in range(E // 512):
                for j in range(8):
                    acc = acc + q[:, ch, :, j]
        else:
            trips = cdiv(E, 64)
            q = torch.cat([t, torch.zeros(R, trips * 64 - E)], 1).view(R, trips, 64)
            acc = torch.zeros(R, 64)
            for i in range(trips):
                acc = acc + q[:, i]
        return _wave_sum(acc)

    def rownorm_fwd(self, wt, Rp, ld, dtype, misalign=False):
        R, E = wt.shape
        ss = self._row_sum(wt * wt, rownorm_v8(E, ld, not misalign))
        inv = 1.0 / torch.clamp(torch.sqrt(ss), min=EPS_NORM)
        dst = torch.zeros(Rp, ld, dtype=dtype)
        dst[:R, :E] = (wt * inv[:, None]).to(dtype)
        return dst, inv

    def rownorm_bwd(self, wt, inv, dy, E, accumulate, dw0):
        g = dy[:, :E]
        v8 = rownorm_v8(E, E) and dy.shape[1] % 4 == 0
        dot = self._row_sum(wt * inv[:, None] * g, v8)
        v = (g - wt * inv[:, None] * dot[:, None]) * inv[:, None]
        return dw0 + v if accumulate else v

    # ---- margins
    def _target(self, c, kind, s, m, a, k):
        s, m, a, k = _t32(s), _t32(m), _t32(a), _t32(k)
        th = torch.acos(c)
        dth = -1.0 / torch.sqrt(torch.clamp(1.0 - c * c, min=1e-30))
        if kind == ARC:
            phi = th + m - k * (th - a)
            kk = (1.0 + k) if self.mut == "k_sign_flipped" else (1.0 - k)
            return s * torch.cos(phi), -s * torch.sin(phi) * kk * dth
        return s * (c - m + k * (th - a)), s * (1.0 + k * dth)

    def _logits(self, cos, lab, C, kind, s, m, a, k):
        """(logits [N][C], d logit / d cos [N][C]) in f32."""
        c = cos[:, :C]
        lg = _t32(s) * c
        d = torch.full_like(c, s)
        y = lab.clone()
        if self.mut == "minus_1_hits_last_column":
            y = torch.where(y < 0, y + C, y)
        rows = (y >= 0).nonzero().flatten()
        if rows.numel():
            o, dd = self._target(c[rows, y[rows]], kind, s, m, a, k)
            lg[rows, y[rows]], d[rows, y[rows]] = o, dd
        return lg, d

    def gather_target(self, cos, lab):
        out = torch.zeros(cos.shape[0])
        rows = (lab >= 0).nonzero().flatten()
        out[rows] = cos[rows, lab[rows]]
        return out

    def margin_fwd(self, cos, lab, C, kind, s, m, a, k):
        out = cos.clone()
        out[:, :C] = self._logits(cos, lab, C, kind, s, m, a, k)[0]
        return out

    def margin_bwd(self, dlogit, lab, ct, C, ldo, kind, s, m, a, k, dtype):
        N = dlogit.shape[0]
        fill = float("nan") if self.mut == "ldo_not_zeroed" else 0.0
        out = torch.full((N, ldo), fill, dtype=dtype)
        d = torch.full((N, C), s, dtype=torch.float32)
        rows = (lab >= 0).nonzero().flatten()
        if rows.numel():
            d[rows, lab[rows]] = self._target(ct[rows], kind, s, m, a, k)[1]
        out[:, :C] = (dlogit[:, :C] * d).to(dtype)
        return out

    # ---- PartialFC
    def pfc_rowstats(self, cos, C, lab, kind, s, m, a, k, misalign=False):
        N, ld = cos.shape
        v4 = rowstats_v4(ld, not misalign)
        width = ld if self.mut == "pad_in_rowstats" else C
        lg = torch.full((N, ld), float("-inf"))
        lg[:, :C] = self._logits(cos, lab, C, kind, s, m, a, k)[0]
        if width > C:
            lg[:, C:width] = _t32(s) * cos[:, C:width]
        ninf = float("-inf")
        if v4:
            trips, T = cdiv(width, 4096), 1024
            q = torch.cat([lg, torch.full((N, trips * 4096 - ld), ninf)], 1) if trips * 4096 >= ld else lg[:, :trips * 4096]
            q = q.reshape(N, trips, T, 4)
            mx, sm = torch.full((N, T), ninf), torch.zeros(N, T)
            for i in range(trips):
                l4 = q[:, i]
                act = l4[..., 0] != ninf                          # a thread whose first column is valid takes the trip
                nm = torch.maximum(torch.maximum(torch.maximum(l4[..., 0], l4[..., 1]), torch.maximum(l4[..., 2], l4[..., 3])), mx)
                nms = torch.where(act, nm, torch.zeros_like(nm))
                e = [torch.exp(l4[..., j] - nms) for j in range(4)]
                resc = torch.ones_like(sm) if self.mut == "rescale_dropped" else torch.exp(torch.where(act, mx - nms, torch.zeros_like(mx)))
                new = sm * resc + ((e[0] + e[1]) + (e[2] + e[3]))
                sm, mx = torch.where(act, new, sm), torch.where(act, nm, mx)
        else:
            trips, T = cdiv(width, 256), 256
            q = torch.cat([lg[:, :width], torch.full((N, trips * 256 - width), ninf)], 1).view(N, trips, T)
            mx, sm = torch.full((N, T), ninf), torch.zeros(N, T)
            for i in range(trips):
                l = q[:, i]
                act = l != ninf
                up = act & (l > mx)
                ls = torch.where(act, l, torch.zeros_like(l))
                mxs = torch.where(mx == ninf, ls, mx)
                resc = torch.ones_like(sm) if self.mut == "rescale_dropped" else torch.where(mx == ninf, torch.zeros_like(sm), torch.exp(mxs - ls))
                s_up = sm * resc + 1.0
                s_keep = sm + torch.exp(ls - mxs)
                sm = torch.where(up, s_up, torch.where(act, s_keep, sm))
                mx = torch.where(up, l, mx)
        W = T // 64
        mxw, smw = mx.view(N, W, 64), sm.view(N, W, 64)
        wm = mxw.max(2)[0]
        wms = torch.where(wm == ninf, torch.zeros_like(wm), wm)
        ws = _wave_sum(torch.where(mxw == ninf, torch.zeros_like(smw), smw * torch.exp(torch.where(mxw == ninf, torch.zeros_like(mxw), mxw - wms[..., None]))))
        M = wm.max(1)[0]
        S = torch.zeros(N)
        for i in range(W):
            S = S + torch.where(wm[:, i] == ninf, torch.zeros(N), ws[:, i] * torch.exp(torch.where(wm[:, i] == ninf, torch.zeros(N), wm[:, i] - M)))
        return M, S

    def pfc_grad(self, cos, C, lab, kind, s, m, a, k, gmax, gsum, eps_ls, inv_n, ldo, dtype):
        N = cos.shape[0]
        lg, d = self._logits(cos, lab, C, kind, s, m, a, k)
        inv_s = 1.0 / gsum
        prob = torch.exp(lg - gmax[:, None]) * inv_s[:, None]
        eps, den = _t32(eps_ls), _t32(float(C if self.mut == "smooth_denominator_C" else C - 1))
        has = torch.ones(N, dtype=torch.bool) if self.mut == "smooth_on_label_minus_1" else (lab >= 0)
        tgt = torch.where(has[:, None], (eps / den).expand(N, C), torch.zeros(N, C)).clone()
        y = torch.where(lab < 0, lab + C, lab) if self.mut == "minus_1_hits_last_column" else lab
        rows = (y >= 0).nonzero().flatten()
        pt = torch.full((N,), float("nan"))
        if self.mut != "ptarget_unwritten_minus_1":
            pt[lab < 0] = 0.0
        if rows.numel():
            tgt[rows, y[rows]] = 1.0 - eps
            pt[rows] = prob[rows, y[rows]]
        out = torch.zeros(N, ldo, dtype=dtype)
        out[:, :C] = ((prob - tgt) * _t32(inv_n) * d).to(dtype)
        return out, pt

    # ---- layout / GEMM
    def transpose(self, src, C, ld_d, dtype):
        R = src.shape[0]
        full = torch.full((2 * GUARD_ROWS + C, ld_d), 7.0, dtype=dtype)
        full[GUARD_ROWS:GUARD_ROWS + C] = 0.0
        full[GUARD_ROWS:GUARD_ROWS + C, :R] = src[:, :C].t()
        return full

    def gemm_splitk(self, a, wp):
        from msml_amd import _lib
        M, K = a.shape
        ks = _lib.value("msml_gemm_splitk_workspace", M, wp.shape[0], K) // (M * wp.shape[0] * 4)
        per = cdiv(cdiv(K, ks), 32) * 32
        out = torch.zeros(M, wp.shape[0])
        for i in range(0, K, per):
            out = out + a[:, i:i + per].float() @ wp[:, i:i + per].float().t()
        return out

    # ---- optimizer
    def sgd(self, wt, grad, buf, lr, mu, wd, first, coef, dev=False):
        n = wt.numel()
        lr, mu, wd = _t32(lr), _t32(mu), _t32(wd)
        cf = coef[0] if coef is not None else _t32(1.0)
        if self.mut == "sgd_first_ignored":
            first = 0
        g = grad * cf + wd * wt
        b = g if first else mu * buf + g
        w2 = wt - lr * b
        if self.mut == "sgd_tail_skipped" and n % 4:
            b[n - n % 4:], w2[n - n % 4:] = buf[n - n % 4:], wt[n - n % 4:]
        return w2, b

    def grad_norm_clip(self, g, max_norm, scale):
        n = g.numel()
        rows = sumsq_rows(n)
        stride, n4 = rows * 256, n // 4
        cnt = cdiv(n4, stride)                                 # float4 trips of the busiest thread
        x = torch.cat([g[:n4 * 4], torch.zeros(cnt * stride * 4 - n4 * 4)]).view(cnt, stride, 4)
        have = (torch.arange(cnt).view(cnt, 1) * stride + torch.arange(stride).view(1, stride)) < n4
        mine = have.sum(0)                                     # trips of each thread
        un = mine // 4
        sq = lambda a: ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]) + a[..., 3] * a[..., 3]
        s4 = [torch.zeros(stride) for _ in range(4)]
        for i in range(cnt):
            v = sq(x[i])
            in_un = i < 4 * un                                 # this trip belongs to a thread's unrolled part
            for j in range(4):
                take = (in_un & (i % 4 == j)) | (~in_un & (i < mine) & (j == 0))
                s4[j] = torch.where(take, s4[j] + v, s4[j])
        if n % 4 and self.mut != "sumsq_tail_skipped":
            t = g[n4 * 4:]
            s4[0][:n % 4] = s4[0][:n % 4] + t * t
        sums = (s4[0] + s4[1]) + (s4[2] + s4[3])
        red = _wave_sum(sums.view(rows, 4, 64))
        part = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
        sc = _t32(scale)
        norm = torch.sqrt(part.double().sum()).float() * sc
        cc = _t32(max_norm) / (norm + _t32(EPS_CLIP))
        if self.mut != "clip_not_capped":
            cc = torch.clamp(cc, max=1.0)
        return torch.stack([norm, cc if self.mut == "scale_not_on_coef" else cc * sc])
