"""Shared by tests/test_ew_cpu.py and tests/test_gpu_ew.py: the case tables of the element-wise and loss kernels of
msml_amd/csrc/fm.hip, seg.hip, lightcnn.hip and x3.hip, float64 references, derived error budgets, a torch restatement of
the kernels' f32 arithmetic (with single-fault mutants) and the checks that compare ANY implementation of the entry points
-- the restatement on the CPU, the library on the GPU -- with the reference.  Conventions (U32 / UBF / U64 / SAFETY, f32(),
Report, LIBM_FACTOR, FLT_MIN) are those of tests/bn_cases.py and tests/head_cases.py.

References (f64, on exactly the operands the kernel receives: storage-rounded tensors widened to f64, `float` parameters
after an f32 round trip):
  fm_fuse        M = tanh(x) | sigmoid(x);  z = arith(yf, M) + yf;  dx = dz * d arith / dM * M',  dyf = dz * (d arith / dyf + 1)
  fm_act, mul, axpb, mse (sum (a - b)^2 / count, count the REAL element count: pad channels are zero in both tensors)
  dropout        keep(i) = drop_hash(seed, i) >= thr, an integer restatement (numpy uint64, wrapping); y = x / (1 - p) if kept
  dap            mean over channels 0..8 and 9..17; mask = mean_1 > mean_0 on the kernel's own f32 means
  seg loss       oracle.model.consensus_loss on f64 logits, d loss / d logit by f64 autograd
  pool2          F.max_pool2d(x, 2) + F.avg_pool2d(x, 2) of torch's CPU kernels in f64, backward by f64 autograd
  mfm_bwd        the gradient rule of torch.max(a, b) on the stored selector: exact (select and 0.5 * d)
  x3             hi = bf16(v), lo = bf16(v - hi) (0 where hi is infinite), hi again, with torch's RNE casts: exact;
                 add / bn_act / fm_fuse: f64 on the loaded values hi + lo

Domains, stated here and asserted on the drawn inputs:
  FM            x in [-12, 12] with both saturated ends and +-0 planted.  `div` divides by M: its cases draw x with
                |M| >= M_MIN = 2^-6 (tanh: |x| >= 2^-5, no +-0; sigmoid: x >= -4)
  seg loss      mask values in {0, 1}; |logit_0 - logit_1| <= 30, so every f32 probability is >= 9e-14 and the reference's
                count of non-zero entries of p * I equals the kernel's 2 * sup
  mfm_bwd       |dy| >= 2^-100 (0.5 * d stays normal);  pool2_bwd  |dy| >= 0.25 (a misrouted gradient is far over budget)

Budgets.  k * u32 * (sum of the magnitudes of the terms) + u_store * |ref|, k counted from the expression written next to
it; 1 - M^2 and M (1 - M) follow the same rule, which makes their budget absolute (the f32 tanh saturates to 1 where the
f64 one does not).  __expf(x) carries L(exp) + |x|.  Sums use n_chain * u32 * sum |term| with n_chain from the launch
geometry: 8 terms per lane in k_mse_partial (the rest of that sum is f64), ceil(HW / 256) + 6 wave levels + 3 in
k_seg_sums, 8 adds in k_dap_fwd.  One FLT_MIN per product and per store.  SAFETY = 2 multiplies every budget, nothing
else does.
  Stores.  u_store is that of the earlier files (u32 = 2^-24, bn_cases.UBF = 2^-9 for bf16): with SAFETY the bf16 bound is
  2^-8 |ref|, exactly the half ulp of an 8-bit significand that an RNE store can reach, so a truncating or double-rounding
  store (up to one ulp) fails.  The split-bf16 store adds U_SPLIT = 2^-18 |ref|, 2^-17 with SAFETY: hi is v rounded to 8
  bits (|v - hi| <= 2^-8 of v's binade 2^e), v - hi is exact in f32, lo is that difference rounded to 8 bits: exact when
  it is the power of two 2^(e-8), otherwise it lies below 2^(e-8) and is off by at most 2^-8 * 2^(e-9);
  tests/test_ew_cpu.py measures exactly 2^-17.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.head_cases import (DT, FLT_MIN, SAFETY, U32, U64, UBF, Case, L, Report, _t32, _wave_sum, cdiv, f32,  # noqa: F401
                              u_store)

TANH, SIGMOID = 0, 1
ADD, SUB, MUL, DIV = 0, 1, 2, 3
ACT_NAME = ("tanh", "sigmoid")
ARITH_NAME = ("add", "sub", "mul", "div")
FM_LANES = 2048 * 256                      # fm_grid / x3_grid: 2048 workgroups of 256 lanes, 8 elements per lane
FM_CAP = FM_LANES * 8
FM_NS = (8, 16, 2040, 2048, 2056, 8 * (FM_LANES - 1), 8 * FM_LANES, 8 * (FM_LANES + 5))
M_MIN = 2.0 ** -6
U_SPLIT = 2.0 ** -18
NAN = float("nan")


def fm_grid(n8):
    return min(cdiv(n8, 256), 2048)


def _big(n):
    return n >= 1 << 20


# =========================================================================================================== fm.hip
def fm_cases():
    """fm_fuse_fwd / _bwd: every (act, arith) pair at every size in both dtypes."""
    out = []
    for i, n in enumerate(FM_NS):
        for act in (TANH, SIGMOID):
            for arith in (ADD, SUB, MUL, DIV):
                for dt in ("f32", "bf16"):
                    out.append(Case("fm-n%d-%s-%s-%s" % (n, ACT_NAME[act], ARITH_NAME[arith], dt), dtype=dt, n=n, act=act,
                                    arith=arith))
    return out


def ew_cases():
    """fm_act_fwd / _bwd, mul_fwd / _bwd, axpb."""
    out = []
    for i, n in enumerate(FM_NS):
        for dt in ("f32", "bf16"):
            out.append(Case("ew-n%d-%s" % (n, dt), dtype=dt, n=n, act=TANH, arith=ADD))
    return out


def draw_fm(case, device="cpu"):
    """x, yf, dz in the case's storage type (domain: module text)."""
    n, act, arith = case.n, case.act, case.arith
    g = case.gen()
    u = torch.rand(n, generator=g)
    if arith == DIV and act == TANH:
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -torch.ones(n), torch.ones(n))
        x = sign * (2.0 ** -5 + (12.0 - 2.0 ** -5) * u)
        plant = (12.0, -12.0, 2.0 ** -5, -2.0 ** -5)
    elif arith == DIV:
        x = -4.0 + 16.0 * u
        plant = (12.0, -4.0, 0.0, -0.0)
    else:
        x = 24.0 * u - 12.0
        plant = (12.0, -12.0, 0.0, -0.0)
    x[:4] = torch.tensor(plant)
    yf, dz = torch.randn(n, generator=g), torch.randn(n, generator=g)
    dt = DT[case.dtype]
    return tuple(t.to(dt).to(device) for t in (x, yf, dz))


def act_terms(x, act):
    """M = act(x), its budget, M' = dM / dx and its budget, for x in f64."""
    if act == TANH:
        m = torch.tanh(x)
        dm = L("tanh") * U32 * m.abs()
        g = 1.0 - m * m
        dg = 2.0 * m.abs() * dm + 2 * U32 * (1.0 + m * m)            # 1 - m * m: 2 ops on 1 + m^2
    else:
        m = torch.sigmoid(x)
        # 1 / (1 + __expf(-x)): e = (1 - m) / m carries L + |x| and weighs e / (1 + e) = 1 - m; the sum and the division: 2 ops
        dm = m * ((L("exp") + x.abs()) * (1.0 - m) + 2) * U32
        g = m * (1.0 - m)
        dg = dm * ((1.0 - m) + m) + U32 * m * (1.0 + m) + U32 * g   # 1 - m: 1 op on 1 + m; the product: 1 op
    return m, dm, g, dg


def fuse_reference(x, y, d, act, arith, us):
    """(z, budget), (dx, budget), (dyf, budget) of the FM fusion for f64 x, yf, dz; us: what the store adds per |ref|."""
    m, dm, g, dg = act_terms(x, act)
    if arith in (ADD, SUB):
        r = y + m if arith == ADD else y - m
        dr = dm + U32 * (y.abs() + m.abs())                                            # y +- m: 1 op
        dY, ddY = 2.0 * d, torch.zeros_like(d)                                         # 2 * d: exact
        dM, ddM = (d if arith == ADD else -d), torch.zeros_like(d)
    elif arith == MUL:
        r = y * m
        dr = y.abs() * dm + U32 * r.abs() + FLT_MIN                                    # y * m: 1 op
        dY = d * (m + 1.0)
        ddY = d.abs() * (dm + U32 * (m.abs() + 1.0)) + U32 * dY.abs() + FLT_MIN        # d * (m + 1): 2 ops
        dM = d * y
        ddM = U32 * dM.abs() + FLT_MIN                                                 # d * y: 1 op
    else:
        im = 1.0 / m
        dim = dm * im * im + U32 * im.abs()                                            # 1 / m: 1 op
        r = y / m
        dr = y.abs() * dm * im * im + U32 * r.abs() + FLT_MIN                          # y / m: 1 op
        dY = d * (im + 1.0)
        ddY = d.abs() * (dim + U32 * (im.abs() + 1.0)) + U32 * dY.abs() + FLT_MIN      # d * (im + 1): 2 ops
        dM = -d * y * im * im
        ddM = 2.0 * (d * y * im).abs() * dim + 3 * U32 * dM.abs() + 3 * FLT_MIN        # -d * y * im * im: 3 ops
    z = r + y
    bz = dr + U32 * (r.abs() + y.abs()) + us * z.abs() + FLT_MIN                       # r + y: 1 op; the store
    dx = dM * g
    bdx = dM.abs() * dg + g.abs() * ddM + U32 * dx.abs() + us * dx.abs() + 2 * FLT_MIN  # dM * M': 1 op; the store
    bdy = ddY + us * dY.abs() + FLT_MIN
    return (z, bz), (dx, bdx), (dY, bdy)


def check_fm_case(be, case, rep, device="cpu"):
    x, yf, dz = draw_fm(case, device)
    m = act_terms(x.double(), case.act)[0]
    assert float(x.abs().max()) <= 12.0
    if case.arith == DIV:
        assert float(m.abs().min()) >= M_MIN, "div domain"
    (z, bz), (dx, bdx), (dy, bdy) = fuse_reference(x.double(), yf.double(), dz.double(), case.act, case.arith,
                                                   u_store(DT[case.dtype]))
    rep.check("fm_fuse_fwd", "z", be.fm_fuse_fwd(x, yf, case.act, case.arith), z, bz, case)
    kx, ky = be.fm_fuse_bwd(dz, x, yf, case.act, case.arith)
    rep.check("fm_fuse_bwd", "dx", kx, dx, bdx, case)
    rep.check("fm_fuse_bwd", "dyf", ky, dy, bdy, case)


AXPBS = ((-1.0, 1.0), (0.37, -2.5))          # 1 - M ('invert') and a general pair


def check_ew_case(be, case, rep, device="cpu"):
    x, b, g = draw_fm(case, device)
    xd, bd, gd = x.double(), b.double(), g.double()
    us = u_store(DT[case.dtype])
    for act in (TANH, SIGMOID):
        m, dm, gp, dgp = act_terms(xd, act)
        rep.check("fm_act_fwd", "m " + ACT_NAME[act], be.fm_act_fwd(x, act), m, dm + us * m.abs() + FLT_MIN, case)
        ref = gd * gp
        # g * M': 1 op; the product and the store may underflow
        rep.check("fm_act_bwd", "dx " + ACT_NAME[act], be.fm_act_bwd(g, x, act), ref,
                  gd.abs() * dgp + U32 * ref.abs() + us * ref.abs() + 2 * FLT_MIN, case)
    ref = xd * bd
    rep.check("mul_fwd", "out", be.mul_fwd(x, b), ref, (U32 + us) * ref.abs() + 2 * FLT_MIN, case)
    for na, nb in ((1, 1), (1, 0), (0, 1)):
        da, db = be.mul_bwd(g, x, b, na, nb)
        assert (da is None) == (not na) and (db is None) == (not nb)
        for what, got, r in (("da", da, gd * bd), ("db", db, gd * xd)):
            if got is not None:
                rep.check("mul_bwd", "%s need=%d%d" % (what, na, nb), got, r, (U32 + us) * r.abs() + 2 * FLT_MIN, case)
    for a, c in AXPBS:
        a, c = f32(a), f32(c)
        ref = a * xd + c
        # a * x + b: 2 ops on |a x| + |b|
        rep.check("axpb", "y a=%g" % a, be.axpb(x, a, c), ref, 2 * U32 * ((a * xd).abs() + abs(c)) + us * ref.abs() + 2 * FLT_MIN,
                  case)


# ---- MSE
MSE_REAL, MSE_CP = 5, 8


def mse_cases():
    out = []
    for i, rows in enumerate((1, 2, 257, FM_LANES, FM_LANES + 5)):          # n = rows * 8: one lane per row
        for dt in ("f32", "bf16"):
            out.append(Case("mse-rows%d-%s" % (rows, dt), dtype=dt, rows=rows, g=(1.0, 0.37)[len(out) % 2]))
    return out


def mse_reference(a, b, count):
    return ((a - b) ** 2).sum() / count


def check_mse_case(be, case, rep, device="cpu"):
    rows, gen = case.rows, case.gen()
    a, b = torch.randn(rows, MSE_CP, generator=gen), torch.randn(rows, MSE_CP, generator=gen)
    a[:, MSE_REAL:], b[:, MSE_REAL:] = 0.0, 0.0                              # pad channels: zero in both
    a, b = (t.to(DT[case.dtype]).to(device) for t in (a, b))
    count = float(rows * MSE_REAL)
    n8 = rows
    nb = fm_grid(n8)
    ad, bd = a.double(), b.double()
    s = ((ad - bd) ** 2).sum()
    ref = s / count
    # a lane: d = u - v (1 op, twice in d * d), the product, the 8-term f32 chain: 11 u32 on sum d^2; the rest in f64: a
    # thread's trips, the 256-lane tree, the nb partials; (float)(s / count): 1 op
    bud = (11 * U32 + (cdiv(n8, nb * 256) + 8 + nb + 1) * U64) * ref + U32 * ref + rows * MSE_CP * FLT_MIN / count
    rep.check("mse_fwd", "loss", be.mse_fwd(a, b, count).reshape(()), ref, bud, case)
    g = torch.tensor([case.g], dtype=torch.float32, device=device)
    us = u_store(DT[case.dtype])
    r = (2.0 / count) * g.double() * (ad - bd)
    for na, nb_ in ((1, 1), (1, 0), (0, 1)):
        da, db = be.mse_bwd(a, b, g, count, na, nb_)
        assert (da is None) == (not na) and (db is None) == (not nb_)
        # c = (float)(2 / count) * g: 2 ops; c * (u - v): 2 ops
        for what, got, rr in (("da", da, r), ("db", db, -r)):
            if got is not None:
                rep.check("mse_bwd", "%s need=%d%d" % (what, na, nb_), got, rr, (4 * U32 + us) * rr.abs() + 2 * FLT_MIN, case)
                rep.exact("mse_bwd", "%s pad channels" % what, got[:, MSE_REAL:], torch.zeros(rows, MSE_CP - MSE_REAL, device=device),
                          case)


# ---- dropout: integer restatement of drop_hash
_M64 = (1 << 64) - 1
_GOLD, _C1, _C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
DROP_PS = (0.0, 0.4, 0.5, 0.999)
DROP_SEEDS = (0, 1, 123, 2 ** 63 - 1, -1)


def drop_hash(seed, idx):
    """drop_hash(seed, i) of fm.hip for idx (numpy uint64), wrapping 64-bit arithmetic."""
    z = np.uint64(seed & _M64) + idx * np.uint64(_GOLD)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_C1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_C2)
    return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def drop_thr(p):
    return np.uint32(int(float(np.float32(p)) * 4294967296.0))          # (unsigned int)((double)(float)p * 2^32)


def keep_mask(seed, n, p, strict=False):
    h = drop_hash(seed, np.arange(n, dtype=np.uint64))
    return torch.from_numpy(h > drop_thr(p) if strict else h >= drop_thr(p))


def planted_seed(i, thr):
    """A seed (as the signed long of the ABI) with drop_hash(seed, i) == thr exactly: the finalizer run backwards."""
    def unshift(v, s):                      # z from v = z ^ (z >> s)
        z = v
        for _ in range(64 // s + 1):
            z = v ^ (z >> s)
        return z
    z = unshift((int(thr) << 32) | 0x2545F491, 31)
    z = unshift(z * pow(_C2, -1, 1 << 64) & _M64, 27)
    z = unshift(z * pow(_C1, -1, 1 << 64) & _M64, 30)
    seed = (z - i * _GOLD) & _M64
    return seed - (1 << 64) if seed >= 1 << 63 else seed


PLANTED_DROPS = ((16, 0.5, 5), (16, 0.0, 9), (2056, 0.4, 2051))       # (n, p, the element whose hash equals thr)


def dropout_cases():
    out = []

    def add(n, p, seed, dt, planted=None):
        out.append(Case("drop-n%d-p%g-seed%d-%s" % (n, p, seed, dt), dtype=dt, n=n, prob=p, seed=seed, planted=planted))
    for n in FM_NS:
        for dt in ("f32", "bf16"):
            add(n, 0.4, 123, dt)
    for p in DROP_PS:
        for seed in DROP_SEEDS:
            for dt in ("f32", "bf16"):
                add(2056, p, seed, dt)
    for j, p in enumerate(DROP_PS):                                     # element indices past 2^22
        for dt in ("f32", "bf16"):
            add(FM_NS[-1], p, DROP_SEEDS[j + 1], dt)
    for n, p, i in PLANTED_DROPS:
        for dt in ("f32", "bf16"):
            add(n, p, planted_seed(i, drop_thr(p)), dt, planted=i)
    return out


def check_dropout_case(be, case, rep, device="cpu"):
    n, p, seed = case.n, case.prob, case.seed
    v = torch.randn(n, generator=case.gen())
    x = (torch.where(v < 0, -torch.ones(n), torch.ones(n)) * (0.5 + v.abs())).to(DT[case.dtype]).to(device)   # never 0
    keep = keep_mask(seed, n, p).to(device)
    if case.planted is not None:
        assert int(drop_hash(seed, np.array([case.planted], dtype=np.uint64))[0]) == int(drop_thr(p)) and bool(keep[case.planted])
    y = be.dropout(x, p, seed)
    rep.exact("dropout", "keep mask", y != 0, keep, case)
    p32 = f32(p)
    ref = torch.where(keep, x.double() / (1.0 - p32), torch.zeros(n, dtype=torch.float64, device=device))
    # scale = 1 / (1 - p): 2 ops; x * scale: 1 op
    rep.check("dropout", "y", y, ref, (3 * U32 + u_store(DT[case.dtype])) * ref.abs(), case)
    if p == 0.0:
        rep.exact("dropout", "p = 0 returns x", y, x, case)
    rep.exact("dropout_dev", "equals dropout", be.dropout(x, p, seed, dev=True), y, case)


# ========================================================================================================== seg.hip
DAP_SHAPES = ((1, 1, 1), (2, 7, 7), (3, 1, 85), (2, 112, 112), (3, 1, 349527))      # the last: over the 4096-block cap
DAP_CPS = (24, 32, 64)


def dap_cases():
    out = []
    for i, (N, H, W) in enumerate(DAP_SHAPES):
        for j, Cp in enumerate(DAP_CPS):
            for dt in ("f32", "bf16"):
                out.append(Case("dap-%dx%dx%d-Cp%d-%s" % (N, H, W, Cp, dt), dtype=dt, N=N, H=H, W=W, Cp=Cp))
    return out


def check_dap_case(be, case, rep, device="cpu"):
    N, H, W, Cp = case.N, case.H, case.W, case.Cp
    gen = case.gen()
    npix = N * H * W
    x = torch.randn(npix, Cp, generator=gen)
    ties = sorted({0, npix // 2, npix - 1})
    x[ties, 9:18] = x[ties, 0:9]                                        # planted exact ties
    x[:, 18:] = NAN                                                     # pad channels must not reach seg
    x = x.to(DT[case.dtype]).to(device).view(N, H, W, Cp)
    xd = x.double().view(npix, Cp)
    ref = torch.stack([xd[:, 0:9].sum(1), xd[:, 9:18].sum(1)], 1) / 9.0
    mag = torch.stack([xd[:, 0:9].abs().sum(1), xd[:, 9:18].abs().sum(1)], 1)
    ref, mag = (t.view(N, H * W, 2).permute(0, 2, 1).reshape(N, 2, H, W) for t in (ref, mag))
    seg, mask = be.dap_fwd(x, True)
    # s += x_j: 8 adds on sum |x|; s / 9: 1 op
    rep.check("dap_fwd", "seg", seg, ref, 8 * U32 * mag / 9.0 + U32 * ref.abs(), case)
    rep.exact("dap_fwd", "mask == (seg1 > seg0)", mask.view(N, H, W), seg[:, 1] > seg[:, 0], case)
    rep.exact("dap_fwd", "planted ties give 0", mask.view(-1)[ties], torch.zeros(len(ties), device=device), case)
    seg2, none = be.dap_fwd(x, False)
    assert none is None
    rep.exact("dap_fwd", "seg without mask", seg2, seg, case)
    dseg = torch.randn(N, 2, H, W, generator=gen).to(device)
    dx = be.dap_bwd(dseg, Cp, DT[case.dtype]).view(npix, Cp)
    gd = dseg.double().view(N, 2, H * W).permute(0, 2, 1).reshape(npix, 2) / 9.0
    r = torch.cat([gd[:, 0:1].expand(npix, 9), gd[:, 1:2].expand(npix, 9)], 1)
    rep.check("dap_bwd", "dx", dx[:, :18], r, (U32 + u_store(DT[case.dtype])) * r.abs() + FLT_MIN, case)    # g / 9: 1 op
    rep.exact("dap_bwd", "pad channels", dx[:, 18:], torch.zeros(npix, Cp - 18, device=device), case)


# ---- consensus loss
SEG_SHAPES = ((1, 1, 1), (1, 7, 9), (3, 8, 8), (1, 15, 17), (3, 16, 16), (1, 1, 257), (3, 112, 112), (256, 1, 1), (257, 7, 9),
              (513, 8, 8), (256, 1, 257), (3, 15, 17))
SEG_PATTERNS = ("mixed", "all0", "all1", "noblob0", "single")
SEG_AB = ((10.0, 5.0), (0.0, 5.0), (10.0, 0.0), (1.5, 0.25))
SEG_REDUCE = ((0, 0), (0, 1), (1, 0), (1, 1))            # (reduce_pixel_all, reduce_pixel_kl_all)
SEG_OVER_CAP = (257, 112, 112)                          # 3.2 M pixels: k_seg_grad's 4096 x 256 threads take four trips
MAX_DIFF = 30.0


def seg_cases():
    out = []
    for i, (N, H, W) in enumerate(SEG_SHAPES):
        for j, (ma, ka) in enumerate(SEG_REDUCE):
            pat, ab = SEG_PATTERNS[(i + j) % 5], SEG_AB[(i + 2 * j) % 4]
            out.append(Case("seg-%dx%dx%d-%s-mean%d-kl%d-a%g-b%g" % (N, H, W, pat, ma, ka, ab[0], ab[1]), N=N, H=H, W=W, pattern=pat,
                            mean_all=ma, kl_all=ka, ab=ab))
    N, H, W = SEG_OVER_CAP
    for (ma, ka), pat, ab in (((0, 0), "mixed", SEG_AB[0]), ((1, 1), "noblob0", SEG_AB[3])):
        out.append(Case("seg-%dx%dx%d-%s-mean%d-kl%d-a%g-b%g" % (N, H, W, pat, ma, ka, ab[0], ab[1]), N=N, H=H, W=W, pattern=pat,
                        mean_all=ma, kl_all=ka, ab=ab))
    return out


def draw_seg(case):
    """logit [N][2][H][W] f32, mask [N][H][W] int64, on the CPU."""
    N, H, W, pat = case.N, case.H, case.W, case.pattern
    g = case.gen()
    l0 = 3.0 * torch.randn(N, H, W, generator=g)
    d = (8.0 * torch.randn(N, H, W, generator=g)).clamp(-MAX_DIFF, MAX_DIFF)
    l0.view(-1)[0], d.view(-1)[0] = 15.0, MAX_DIFF                 # the ends of the domain, exact in f32
    if l0.numel() > 1:
        l0.view(-1)[-1], d.view(-1)[-1] = -15.0, -MAX_DIFF
    logit = torch.stack([l0, (l0.double() - d.double()).float()], 1).contiguous()
    msk = (torch.rand(N, H, W, generator=g) < 0.4).long()
    if pat == "all0":
        msk.zero_()
    elif pat == "all1":
        msk.fill_(1)
    elif pat == "noblob0":
        msk[N // 2] = 1                                       # one image without blob 0 (N == 1: the same as all1)
    elif pat == "single":
        msk[0] = 0
        msk[0].view(-1)[(H * W) // 2] = 1                     # image 0: blob 1 is one pixel (H * W == 1: its only one)
    # the domain
    assert bool(((msk == 0) | (msk == 1)).all())
    while float((logit[:, 0].double() - logit[:, 1].double()).abs().max()) > MAX_DIFF:       # the f32 rounding of l0 - d
        over = (logit[:, 0].double() - logit[:, 1].double()).abs() > MAX_DIFF
        logit[:, 1] = torch.where(over, logit[:, 0], logit[:, 1])
    p = torch.softmax(logit, 1)
    assert float(p.min()) >= 9e-14
    for s in (0, 1):
        ind = (msk == s).unsqueeze(1).float()
        assert int((p * ind != 0).sum()) == 2 * int(ind.sum()), "the reference's non-zero count is not 2 * sup"
    return logit, msk


def consensus_expr(logit, msk, alpha, beta, mean_all, kl_all):
    """The expression of oracle.model.consensus_loss inside the domain (non-zero entries of p * I == the blob's pixels) with
    the logarithms of absent blobs taken of 1 instead of masked afterwards: the same value, and a finite autograd gradient
    where the oracle's is 0 * inf = NaN (an image without the blob under reduce_pixel = 'all': -log(pbar = 0) is masked by
    a torch.where, whose backward still sees the infinite derivative)."""
    N, _, H, W = logit.shape
    p, lp = torch.softmax(logit, 1), torch.log_softmax(logit, 1)
    vals = [s for s in (0, 1) if bool((msk == s).any())]
    total = 0.0
    for s in vals:
        ind = (msk == s).unsqueeze(1).to(p.dtype)
        sup = ind.sum((2, 3))                                              # N,1
        has = sup > 0
        pbar = (p * ind).sum((2, 3)) / (float(H * W) if mean_all else sup.clamp_min(1.0))
        safe = torch.where(has, pbar, torch.ones_like(pbar))
        nll = torch.where(has[:, 0], -torch.log(safe[:, s]), torch.zeros_like(safe[:, s]))
        kl = (ind * safe[:, :, None, None] * (torch.log(safe)[:, :, None, None] - lp)).sum()
        total = total + alpha * nll.mean() + beta * kl / (float(N * H * W) if kl_all else 2.0 * ind.sum())
    return total / float(len(vals))


def seg_reference(logit, msk, alpha, beta, mean_all, kl_all, parts=False):
    """(loss, dlogit) of oracle.model.consensus_loss in f64 with f64 autograd; the elements of dlogit that autograd leaves
    NaN (consensus_expr's text; tests/test_ew_cpu.py shows the two agree everywhere else) come from consensus_expr."""
    from oracle.model import consensus_loss
    lg = logit.double().requires_grad_(True)
    loss = consensus_loss(lg, msk, alpha, beta, "all" if mean_all else "idx", "all" if kl_all else "idx")
    (d,) = torch.autograd.grad(loss, lg)
    lg2 = logit.double().requires_grad_(True)
    loss2 = consensus_expr(lg2, msk, alpha, beta, mean_all, kl_all)
    (d2,) = torch.autograd.grad(loss2, lg2)
    if parts:
        return loss.detach(), d, loss2.detach(), d2
    return loss.detach(), torch.where(torch.isnan(d), d2, d)


def seg_budget(logit, msk, alpha, beta, mean_all, kl_all):
    """(budget of the loss, budget of dlogit [N][2][H][W]): the per-pixel errors of k_seg_sums through its f32 chains into
    the five sums, those through the f64 expressions of k_seg_loss (first order) into the loss and the coefficients, the
    coefficients and k_seg_grad's own softmax through its f32 expression."""
    N, _, H, W = logit.shape
    HW = H * W
    lg = logit.double().view(N, 2, HW)
    a, b = lg[:, 0], lg[:, 1]
    mx = torch.maximum(a, b)
    dab = (a - b).abs()
    e = torch.exp(-dab)
    ls = torch.log1p(e)
    lse = mx + ls
    lp = torch.stack([a - lse, b - lse], 1)                                                  # [N][2][HW]
    p = torch.exp(lp)
    # expf(l - mx): the difference 1 op (|d| u32 in the exponent), expf L; 1 + e: 1 op; logf: its argument's error and L
    de = e * (L("exp") + dab) * U32
    dls = (de + U32 * (1.0 + e)) / (1.0 + e) + L("log") * U32 * ls
    dlse = dls + U32 * lse.abs()                                                             # mx + log: 1 op
    dlp = dlse[:, None] + U32 * lp.abs()                                                     # l - lse: 1 op
    dp = p * (dlp + L("exp") * U32)                                                          # expf(lp)
    chain = cdiv(HW, 256) + 6 + 3                               # a thread's trips, the wave levels, the four waves
    ind = torch.stack([msk.view(N, HW) == 0, msk.view(N, HW) != 0], 1).double()              # [N][s][HW]
    sup = ind.sum(2)                                                                         # [N][s]
    P = torch.einsum("nsx,nkx->nsk", ind, p)                                                 # [N][s][k]
    Ls = torch.einsum("nsx,nkx->nsk", ind, lp)
    dP = torch.einsum("nsx,nkx->nsk", ind, dp) + chain * U32 * P
    dL = torch.einsum("nsx,nkx->nsk", ind, dlp) + chain * U32 * torch.einsum("nsx,nkx->nsk", ind, lp.abs())
    has = sup > 0
    D = torch.full_like(sup, float(HW)) if mean_all else sup.clamp_min(1.0)
    Ps = torch.where(has[..., None], P, torch.ones_like(P))
    pb = Ps / D[..., None]
    A = sup[..., None] * (torch.log(pb) + 1.0) - Ls                                          # d kl / d pbar_k
    dA = sup[..., None] * dP / Ps + dL
    tot = sup.sum(0)                                                                         # [s]
    nb = max(int((tot > 0).sum()), 1)
    Z = torch.full_like(tot, float(N * HW)) if kl_all else (2.0 * tot).clamp_min(1.0)        # [s]
    hs = has.double()
    sel = torch.eye(2, dtype=torch.float64)                                                  # [s][k]: k == s
    dnll = (dP / Ps * sel).sum(2)
    dkl = (A.abs() / D[..., None] * dP + pb * dL).sum(2)
    dloss = (hs * (alpha / N * dnll + beta * dkl / Z)).sum() / nb
    gA = (beta * A / D[..., None] / Z[None, :, None] - sel * alpha / (N * Ps)) / nb
    gB = beta * pb / Z[None, :, None] / nb
    dgA = (beta * dA / D[..., None] / Z[None, :, None] + sel * alpha * dP / (N * Ps * Ps)) / nb + U32 * gA.abs()   # (float)
    dgB = beta * dP / D[..., None] / Z[None, :, None] / nb + U32 * gB.abs()
    # k_seg_grad: e_k = expf(l_k - mx), inv = 1 / (e0 + e1), p_k = e_k * inv: L + |d| for e_k, the sum, the division, the product
    dpg = p * (2 * L("exp") + 2 * dab[:, None] + 3) * U32
    pix = lambda c: torch.einsum("nsk,nsx->nkx", c * hs[..., None], ind)                     # the coefficient of each pixel's blob
    cA, cB, dcA, dcB = pix(gA), pix(gB), pix(dgA), pix(dgB)
    t = cA * p - cB
    # t_k = gA_k * p_k - gB_k: 2 ops
    dt = p * dcA + cA.abs() * dpg + dcB + 2 * U32 * ((cA * p).abs() + cB.abs())
    dot = t.sum(1, keepdim=True)
    ddot = dt.sum(1, keepdim=True) + U32 * t.abs().sum(1, keepdim=True)
    # t_k - p_k * dot: 2 ops
    dd = dt + dot.abs() * dpg + p * ddot + 2 * U32 * (t.abs() + (p * dot).abs()) + 4 * FLT_MIN
    return dloss, dd.view(N, 2, H, W), has


def check_seg_case(be, case, rep, device="cpu"):
    logit, msk = draw_seg(case)
    alpha, beta = f32(case.ab[0]), f32(case.ab[1])
    ref, dref = seg_reference(logit, msk, alpha, beta, case.mean_all, case.kl_all)
    dloss, dd, has = seg_budget(logit, msk, alpha, beta, case.mean_all, case.kl_all)
    loss, dlogit, ws = be.seg_loss(logit.to(device), msk.to(device), alpha, beta, case.mean_all, case.kl_all, True)
    key = "seg_consensus_loss_r"
    rep.check(key, "loss", loss.reshape(()).cpu(), ref, dloss + U32 * ref.abs(), case)        # (float)total: 1 op
    rep.check(key, "dlogit", dlogit.cpu(), dref, dd, case)
    coef = ws.cpu()[20 * 0 + 10 * case.N:].view(case.N, 2, 5)
    rep.exact(key, "coef of absent blobs", coef[~has], torch.zeros(int((~has).sum()), 5), case)
    loss2, none, _ = be.seg_loss(logit.to(device), msk.to(device), alpha, beta, case.mean_all, case.kl_all, False)
    assert none is None
    rep.exact(key, "loss without dlogit", loss2.cpu(), loss.cpu(), case)
    if not case.mean_all and not case.kl_all:
        l3, d3 = be.seg_loss_plain(logit.to(device), msk.to(device), alpha, beta)
        rep.exact("seg_consensus_loss", "loss equals _r(0, 0)", l3.cpu(), loss.cpu(), case)
        rep.exact("seg_consensus_loss", "dlogit equals _r(0, 0)", d3.cpu(), dlogit.cpu(), case)


# ====================================================================================================== lightcnn.hip
POOL_HW = ((2, 2), (2, 6), (6, 2), (4, 4), (14, 10))
POOL_CPS = (8, 24, 64)
_LO, _HI = -1.0, 2.0
POOL_WINDOWS = ([(1.0, 1.0, 1.0, 1.0)] +
                [tuple(_HI if k == i else _LO for k in range(4)) for i in range(4)] +
                [tuple(_HI if k in (i, j) else _LO for k in range(4)) for i in range(4) for j in range(i + 1, 4)] +
                [(0.0, -0.0, -0.0, -0.0), (-0.0, 0.0, -0.0, 0.0)] +
                [tuple(NAN if k == i else 0.5 - 0.125 * k for k in range(4)) for i in range(4)])


def pool_cases():
    out = []
    for H, W in POOL_HW:
        for cp in POOL_CPS:
            for N in (1, 3):
                for dt in ("f32", "bf16"):
                    out.append(Case("pool-%dx%dx%dx%d-%s" % (N, H, W, cp, dt), dtype=dt, N=N, H=H, W=W, cp=cp))
    return out


def draw_pool(case, device="cpu"):
    """x [N][H][W][cp] (image 0: planted windows, pattern (window * cp + channel + salt) mod 17; the rest random), dy."""
    N, H, W, cp = case.N, case.H, case.W, case.cp
    g = case.gen()
    x = torch.randn(N, H, W, cp, generator=g)
    P, Q = H // 2, W // 2
    pat = torch.tensor(POOL_WINDOWS)                                      # [17][4]
    idx = (torch.arange(P * Q * cp) + int(torch.randint(0, 17, (1,), generator=g))) % len(POOL_WINDOWS)
    win = pat[idx].view(P, Q, cp, 2, 2)                                   # window positions (0,0) (0,1) (1,0) (1,1)
    x[0] = win.permute(0, 3, 1, 4, 2).reshape(H, W, cp)
    v = torch.randn(N, P, Q, cp, generator=g)
    dy = torch.where(v < 0, -torch.ones_like(v), torch.ones_like(v)) * (0.25 + v.abs())
    dt = DT[case.dtype]
    return x.to(dt).to(device), dy.to(dt).to(device)


def pool_reference(x, dy):
    """F.max_pool2d + F.avg_pool2d of NHWC x in f64 on the CPU and its autograd gradient for dy: (y, dx), NHWC."""
    xc = x.detach().cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(xc, 2) + F.avg_pool2d(xc, 2)
    (dx,) = torch.autograd.grad(y, xc, dy.detach().cpu().double().permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1).contiguous(), dx.permute(0, 2, 3, 1).contiguous()


def check_pool_case(be, case, rep, device="cpu"):
    x, dy = draw_pool(case, device)
    check_pool_outputs(be.pool2_fwd(x), be.pool2_bwd(dy, x), x, dy, case, rep, device)


def check_pool_outputs(y, dx, x, dy, case, rep, device="cpu"):
    yr, dxr = pool_reference(x, dy)
    yr, dxr = yr.to(device), dxr.to(device)
    assert bool(torch.isfinite(dxr).all())
    us = u_store(DT[case.dtype])
    N, H, W, cp = x.shape
    xa = torch.nan_to_num(x.double().abs(), nan=0.0).view(N, H // 2, 2, W // 2, 2, cp).sum((2, 4))
    nan = torch.isnan(yr)
    rep.exact("pool2_fwd", "NaN windows", torch.isnan(y), nan, case)
    zero = torch.zeros_like(yr)
    # ((a + b) + c + d) * 0.25: 3 adds on sum |x| / 4; m + avg: 1 op on |m| + |avg| <= 1.25 sum |x|
    rep.check("pool2_fwd", "y", torch.where(nan, zero, y.double()), torch.where(nan, zero, yr),
              (0.75 + 1.25) * U32 * xa + us * torch.where(nan, zero, yr).abs() + FLT_MIN, case)
    ga = dy.double().abs()[:, :, None, :, None, :].expand(N, H // 2, 2, W // 2, 2, cp).reshape(N, H, W, cp)
    # (arg == w ? g : 0) + 0.25 * g: 2 ops on 1.25 |g|
    rep.check("pool2_bwd", "dx", dx, dxr, 2 * U32 * 1.25 * ga + us * dxr.abs() + FLT_MIN, case)


MFM_SHAPES = ((1, 8, 8), (4, 8, 8), (12, 16, 32), (48, 64, 128), (96, 128, 256), (128, 128, 256))     # (C, cp, czp)
MFM_MS = (1, 3, 257)


def mfm_cases():
    return [Case("mfm-C%d-cp%d-czp%d-M%d-%s" % (C, cp, czp, M, dt), dtype=dt, C=C, cp=cp, czp=czp, M=M)
            for C, cp, czp in MFM_SHAPES for M in MFM_MS for dt in ("f32", "bf16")]


def draw_mfm(case, device="cpu"):
    C, cp, M = case.C, case.cp, case.M
    g = case.gen()
    dy = torch.randn(M, cp, generator=g)
    dy = torch.where(dy.abs() < 2.0 ** -100, torch.ones_like(dy), dy)
    dy[:, C:] = NAN
    sel = torch.randint(0, 4, (M, cp), generator=g).to(torch.uint8)
    sel[:, C:] = 0xFF
    return dy.to(DT[case.dtype]).to(device), sel.to(device)


def mfm_reference(dy, sel, C, czp):
    """The gradient rule of torch.max(a, b) (test_ew_cpu shows it is): sel 1 / 2: the first / second half won, 0: a tie,
    half to each, 3: unordered (a NaN), all of it to both.  [M][czp], channels >= 2C zero; exact in dy's type."""
    d, s = dy[:, :C], sel[:, :C]
    zero = torch.zeros_like(d)
    half = torch.where(s == 0, 0.5 * d, zero)
    first = torch.where((s == 3) | (s == 1), d, half)
    second = torch.where((s == 3) | (s == 2), d, half)
    return torch.cat([first, second, torch.zeros(dy.shape[0], czp - 2 * C, dtype=dy.dtype, device=dy.device)], 1)


def check_mfm_case(be, case, rep, device="cpu", count=None):
    dy, sel = draw_mfm(case, device)
    assert float(dy[:, :case.C].abs().min()) >= 2.0 ** -100
    if count is not None:
        for v in range(4):
            count[v] += int((sel[:, :case.C] == v).sum())
    dz = be.mfm_bwd(dy, sel, case.C, case.czp)
    ref = mfm_reference(dy, sel, case.C, case.czp)
    rep.exact("mfm_bwd", "dz", dz[:, :2 * case.C], ref[:, :2 * case.C], case)
    rep.exact("mfm_bwd", "channels >= 2C", dz[:, 2 * case.C:], ref[:, 2 * case.C:], case)


# =========================================================================================================== x3.hip
X3_CS = (8, 24, 64, 512)
X3_MS = (1, 3, 257)
X3_SHAPES = tuple((M, C) for C in X3_CS for M in X3_MS) + ((FM_LANES + 5, 8),)          # the last: over the 2048-block cap
FLT_MAX = 3.4028234663852886e38
X3_SPECIAL_BITS = (0x7F7FFFFF, 0xFF7FFFFF,            # +-FLT_MAX: round to the bf16 infinity
                   0x7F7F8000, 0x7F7F7FFF,            # the first finite value that does, the last that does not
                   0x7F800000, 0xFF800000,            # +-inf
                   0x00000000, 0x80000000,            # +-0
                   0x00000001, 0x80000001, 0x00400000, 0x007FFFFF, 0x00012345, 0x807FC000)     # f32 subnormals
# How the device's bf16 conversion treats an f32 subnormal: "keep" (RNE on the bit pattern, torch's cast).
X3_SUBNORMAL = "keep"


def x3_split(v):
    """[M][C] f32 -> [M][3C] bf16 planes hi | lo | hi with torch's RNE casts (the reference of msml_x3_from_f32)."""
    hi = v.bfloat16()
    lo = torch.where(torch.isinf(hi.float()), torch.zeros_like(v), v - hi.float()).bfloat16()
    return torch.cat([hi, lo, hi], 1)


def x3_value(t, C):
    """The f64 value a split tensor [M][3C] carries."""
    return t[:, :C].double() + t[:, C:2 * C].double()


def x3_cases():
    return [Case("x3-M%d-C%d" % (M, C), dtype="bf16", M=M, C=C, idx=i) for i, (M, C) in enumerate(X3_SHAPES)]


_BN_VARIANTS = [(sc, sh, al, res) for sc in (0, 1) for sh in (0, 1) for al in (0, 1) for res in (None, 0, 1)]   # res: res_first


def x3_bn_variants(case):
    """The (scale, shift, alpha, residual) combinations of msml_x3_bn_act_fwd a case runs: the 12 shapes under the cap take
    two each, in table order, which are all 24 (tests/test_ew_cpu.py asserts it); the shape over the cap takes everything
    present with the residual on either side, and nothing present."""
    if case.M * case.C > FM_CAP:
        return [(1, 1, 1, 1), (1, 1, 1, 0), (0, 0, 0, None)]
    return [_BN_VARIANTS[2 * case.idx], _BN_VARIANTS[2 * case.idx + 1]]


def _check_split(rep, key, what, out, ref, budget, C, case):
    """A split output against an f64 reference: the value hi + lo within budget + the split store, plane 3 == plane 1,
    |lo| <= 2^-8 |hi| (lo is a remainder of the rounding to hi: at most half an ulp of hi)."""
    val = x3_value(out, C)
    rep.check(key, what, val, ref, budget + U_SPLIT * ref.abs() + 2 * FLT_MIN, case)
    rep.exact(key, what + ": third plane", out[:, 2 * C:], out[:, :C], case)
    rep.exact(key, what + ": |lo| <= half an ulp of hi", out[:, C:2 * C].double().abs() <= 2.0 ** -8 * out[:, :C].double().abs(),
              torch.ones_like(val, dtype=torch.bool), case)


def check_x3_case(be, case, rep, device="cpu"):
    M, C, g = case.M, case.C, case.gen()
    src = torch.randn(M, C, generator=g) * torch.exp(4.0 * torch.randn(M, C, generator=g))
    sp = torch.tensor(X3_SPECIAL_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    k = min(sp.numel(), M * C)
    src.view(-1)[:k] = torch.roll(sp, case.idx)[:k]
    src = src.to(device)
    # ---- from_f32 / to_f32: exact
    planes = be.x3_from_f32(src)
    want = x3_split(src)
    for i, nm in enumerate(("hi", "lo", "third plane")):
        ok = torch.equal(planes[:, i * C:(i + 1) * C].contiguous().view(torch.int16), want[:, i * C:(i + 1) * C].contiguous().view(torch.int16))
        rep.exact("x3_from_f32", nm + " bits", torch.tensor(float(ok)), torch.tensor(1.0), case)
    back = be.x3_to_f32(want, C)
    wb = want[:, :C].float() + want[:, C:2 * C].float()
    ok = torch.equal(back.contiguous().view(torch.int32), wb.contiguous().view(torch.int32))
    rep.exact("x3_to_f32", "hi + lo bits", torch.tensor(float(ok)), torch.tensor(1.0), case)
    # +-inf and the finite values that round to the bf16 infinity come back as the infinity (not NaN)
    big = src.abs() >= 2.0 ** 128 - 2.0 ** 119
    rep.exact("x3_to_f32", "overflow reads back as inf", back[big], torch.sign(src[big]) * float("inf"), case)
    # ---- add / bn_act_fwd / fm_fuse_fwd on proper splits of finite data
    a, b, r = (x3_split(torch.randn(M, C, generator=g)).to(device) for _ in range(3))
    av, bv, rv = x3_value(a, C), x3_value(b, C), x3_value(r, C)
    _check_split(rep, "x3_add", "out", be.x3_add(a, b, C), av + bv, U32 * (av + bv).abs(), C, case)
    for sc, sh, al, res in x3_bn_variants(case):
        scale = (1.0 + 0.5 * torch.randn(C, generator=g)).to(device) if sc else None
        shift = torch.randn(C, generator=g).to(device) if sh else None
        alpha = (0.25 + 0.1 * torch.randn(C, generator=g)).to(device) if al else None
        s64 = scale.double() if sc else torch.ones(C, dtype=torch.float64, device=device)
        h64 = shift.double() if sh else torch.zeros(C, dtype=torch.float64, device=device)
        z = av * s64 + h64
        bud = 2 * U32 * ((av * s64).abs() + h64.abs()) + FLT_MIN                      # v * sc + sh: 2 ops
        if res == 1:
            bud = bud + U32 * (z.abs() + rv.abs())
            z = z + rv
        if al:
            neg = z <= 0
            bud = torch.where(neg, bud * alpha.double().abs() + U32 * (z * alpha.double()).abs() + FLT_MIN, bud)   # z * alpha: 1 op
            # an element within its own budget of 0, but not 0, may take either branch: both agree to |z| |1 - alpha|
            bud = bud + torch.where(z.abs() <= 2 * bud, z.abs() * (1.0 - alpha.double()).abs(), torch.zeros_like(z))
            z = torch.where(neg, z * alpha.double(), z)
        if res == 0:
            bud = bud + U32 * (z.abs() + rv.abs())
            z = z + rv
        out = be.x3_bn_act(a, scale, shift, alpha, r if res is not None else None, int(bool(res)), C)
        _check_split(rep, "x3_bn_act_fwd", "y sc%d sh%d al%d res%s" % (sc, sh, al, res), out, z, bud, C, case)
    for act in (TANH, SIGMOID):
        for arith in (ADD, SUB, MUL, DIV):
            fc = Case("%s-%s-%s" % (case.name, ACT_NAME[act], ARITH_NAME[arith]), dtype="f32", n=M * C, act=act, arith=arith)
            x, yf, _ = draw_fm(fc)
            xs, ys = x3_split(x.view(M, C)).to(device), x3_split(yf.view(M, C)).to(device)
            xv, yv = x3_value(xs, C), x3_value(ys, C)
            if arith == DIV:
                assert float(act_terms(xv, act)[0].abs().min()) >= M_MIN, "div domain"
            (zr, bz), _, _ = fuse_reference(xv, yv, yv, act, arith, 0.0)
            _check_split(rep, "x3_fm_fuse_fwd", "z %s %s" % (ACT_NAME[act], ARITH_NAME[arith]), be.x3_fm_fuse(xs, ys, act, arith, C),
                         zr, bz, C, case)


# ------------------------------------------------------------------------- torch restatement of the kernels' arithmetic
MUTANTS = {   # name -> (family in CHECKS, key, what) of the check that must catch it
    "sub_dM_sign": ("fm", "fm_fuse_bwd", "dx"),
    "mul_dyf_without_plus_1": ("fm", "fm_fuse_bwd", "dyf"),
    "tanh_1_minus_M": ("fm", "fm_fuse_bwd", "dx"),
    "grid_tail_dropped": ("fm", "fm_fuse_fwd", "z"),
    "drop_strict_greater": ("dropout", "dropout", "keep mask"),
    "dap_divides_by_8": ("dap", "dap_fwd", "seg"),
    "dap_tie_gives_1": ("dap", "dap_fwd", "planted ties give 0"),
    "seg_mean_all_divides_by_sup": ("seg", "seg_consensus_loss_r", "loss"),
    "seg_nblobs_2": ("seg", "seg_consensus_loss_r", "loss"),
    "seg_absent_coef_kept": ("seg", "seg_consensus_loss_r", "coef of absent blobs"),
    "pool_last_max_wins": ("pool", "pool2_bwd", "dx"),
    "pool_nan_loses": ("pool", "pool2_bwd", "dx"),
    "mfm_tie_full_to_both": ("mfm", "mfm_bwd", "dz"),
    "mfm_pad_not_zeroed": ("mfm", "mfm_bwd", "channels >= 2C"),
    "x3_third_plane_lo": ("x3", "x3_from_f32", "third plane bits"),
    "x3_lo_truncated": ("x3", "x3_from_f32", "lo bits"),
    "x3_lo_of_infinite_hi": ("x3", "x3_from_f32", "lo bits"),          # lo = v - hi = inf - inf: x3_store before the fix
}


def _act32(x, act):
    if act == SIGMOID:
        return 1.0 / (1.0 + torch.exp(-x))
    return torch.tanh(x)


def _trunc_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


class Restatement:
    """The entry points in torch: f32 operations in the kernels' order, the kernels' stores.  `mutant` plants one fault."""
    name = "restatement"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mut = mutant

    def _tail(self, out):
        if self.mut == "grid_tail_dropped":                 # no grid-stride loop: elements past the capped grid stay unwritten
            out = out.clone()
            out.view(-1)[FM_CAP:] = NAN
        return out

    # ---- fm.hip
    def fm_fuse_fwd(self, x, yf, act, arith):
        m, y = _act32(x.float(), act), yf.float()
        r = (y + m, y - m, y * m, y / m)[arith]
        return self._tail((r + y).to(x.dtype))

    def fm_fuse_bwd(self, dz, x, yf, act, arith):
        m, y, d = _act32(x.float(), act), yf.float(), dz.float()
        if act == SIGMOID:
            g = m * (1.0 - m)
        else:
            g = 1.0 - m if self.mut == "tanh_1_minus_M" else 1.0 - m * m
        if arith in (ADD, SUB):
            dY, dM = 2.0 * d, (d if arith == ADD or self.mut == "sub_dM_sign" else -d)
        elif arith == MUL:
            dY, dM = d * (m if self.mut == "mul_dyf_without_plus_1" else m + 1.0), d * y
        else:
            im = 1.0 / m
            dY, dM = d * (im + 1.0), -d * y * im * im
        return self._tail((dM * g).to(x.dtype)), self._tail(dY.to(x.dtype))

    def fm_act_fwd(self, x, act):
        return self._tail(_act32(x.float(), act).to(x.dtype))

    def fm_act_bwd(self, dm, x, act):
        m = _act32(x.float(), act)
        return self._tail((dm.float() * (m * (1.0 - m) if act == SIGMOID else 1.0 - m * m)).to(x.dtype))

    def mul_fwd(self, a, b):
        return self._tail((a.float() * b.float()).to(a.dtype))

    def mul_bwd(self, g, a, b, need_a, need_b):
        return (self._tail((g.float() * b.float()).to(a.dtype)) if need_a else None,
                self._tail((g.float() * a.float()).to(a.dtype)) if need_b else None)

    def axpb(self, x, a, b):
        return self._tail((_t32(a) * x.float() + _t32(b)).to(x.dtype))

    def mse_fwd(self, a, b, count):
        d = a.float().view(-1, 8) - b.float().view(-1, 8)
        q = torch.zeros(d.shape[0])
        for j in range(8):                                   # a lane's 8-term f32 chain; everything after it is f64
            q = q + d[:, j] * d[:, j]
        return (q.double().sum() / count).float().reshape(1)

    def mse_bwd(self, a, b, g, count, need_a, need_b):
        c = torch.tensor(2.0 / count, dtype=torch.float64).float() * g[0]
        x = c * (a.float() - b.float())
        return (x.to(a.dtype) if need_a else None, (-x).to(a.dtype) if need_b else None)

    def dropout(self, x, p, seed, dev=False):
        keep = keep_mask(seed, x.numel(), p, strict=self.mut == "drop_strict_greater").view(x.shape)
        scale = _t32(1.0) / (_t32(1.0) - _t32(p))
        return torch.where(keep, x.float() * scale, torch.zeros(())).to(x.dtype)

    # ---- seg.hip
    def dap_fwd(self, x, with_mask):
        N, H, W, Cp = x.shape
        v = x.float().view(-1, Cp)
        s = [torch.zeros(v.shape[0]), torch.zeros(v.shape[0])]
        for j in range(9):
            s[0], s[1] = s[0] + v[:, j], s[1] + v[:, 9 + j]
        den = 8.0 if self.mut == "dap_divides_by_8" else 9.0
        s0, s1 = s[0] / den, s[1] / den
        seg = torch.stack([s0, s1], 1).view(N, H * W, 2).permute(0, 2, 1).reshape(N, 2, H, W).contiguous()
        mask = (s1 >= s0 if self.mut == "dap_tie_gives_1" else s1 > s0).to(torch.uint8).view(N, H, W)
        return seg, (mask if with_mask else None)

    def dap_bwd(self, dseg, Cp, dtype):
        N, _, H, W = dseg.shape
        g = (dseg / 9.0).view(N, 2, H * W).permute(0, 2, 1).reshape(-1, 2)
        dx = torch.zeros(g.shape[0], Cp)
        dx[:, 0:9], dx[:, 9:18] = g[:, 0:1], g[:, 1:2]
        return dx.to(dtype).view(N, H, W, Cp)

    def seg_loss(self, logit, msk, alpha, beta, mean_all, kl_all, want_grad):
        N, _, H, W = logit.shape
        HW = H * W
        l0, l1 = logit[:, 0].reshape(N, HW), logit[:, 1].reshape(N, HW)
        mx = torch.maximum(l0, l1)
        lse = mx + torch.log(torch.exp(l0 - mx) + torch.exp(l1 - mx))
        lp0, lp1 = l0 - lse, l1 - lse
        s1 = msk.reshape(N, HW) != 0
        w = torch.stack([~s1, s1], 1).float()                                                # [N][s][HW]
        terms = torch.stack([torch.ones_like(l0), torch.exp(lp0), torch.exp(lp1), lp0, lp1], 1)   # [N][5][HW]
        q = w[:, :, None] * terms[:, None]                                                   # [N][s][5][HW]
        trips = cdiv(HW, 256)
        q = torch.cat([q, torch.zeros(N, 2, 5, trips * 256 - HW)], 3).view(N, 2, 5, trips, 256)
        acc = torch.zeros(N, 2, 5, 256)
        for i in range(trips):                               # a thread's chain, then the wave butterflies, then the four waves
            acc = acc + q[:, :, :, i]
        red = _wave_sum(acc.view(N, 2, 5, 4, 64))
        sums = ((red[..., 0] + red[..., 1]) + red[..., 2]) + red[..., 3]                     # [N][s][5] f32
        q = sums.double()
        sup, has = q[..., 0], q[..., 0] > 0
        D = torch.full_like(sup, float(HW)) if (mean_all and self.mut != "seg_mean_all_divides_by_sup") else sup
        Ds = torch.where(has, D, torch.ones_like(D))
        pb = torch.where(has[..., None], q[..., 1:3] / Ds[..., None], torch.ones(1, dtype=torch.float64))     # [N][s][k]
        sel = torch.eye(2, dtype=torch.float64)
        nll = -(torch.log(pb) * sel).sum(2)
        kl = (sup[..., None] * pb * torch.log(pb) - pb * q[..., 3:5]).sum(2)
        hs = has.double()
        tot, nlls, kls = (sup * hs).sum(0), (nll * hs).sum(0), (kl * hs).sum(0)
        nblobs = 2 if self.mut == "seg_nblobs_2" else int((tot > 0).sum())
        Z = torch.full_like(tot, float(N) * HW) if kl_all else 2.0 * tot
        Zs = torch.where(tot > 0, Z, torch.ones_like(Z))
        total = torch.where(tot > 0, alpha * nlls / N + beta * kls / Zs, torch.zeros_like(tot)).sum()
        loss = (total / max(nblobs, 1)).float().reshape(1)
        A = sup[..., None] * (torch.log(pb) + 1.0) - q[..., 3:5]
        inv_nb = 1.0 / max(nblobs, 1)
        gA = (beta * (A / Ds[..., None]) / Zs[None, :, None] - sel * alpha / (N * pb * Ds[..., None])) * inv_nb
        gB = beta * pb / Zs[None, :, None] * inv_nb
        coef = torch.cat([torch.ones(N, 2, 1, dtype=torch.float64), gA, gB], 2)
        valid = has & (nblobs > 0)
        fill = NAN if self.mut == "seg_absent_coef_kept" else 0.0
        coef = torch.where(valid[..., None], coef, torch.full_like(coef, fill)).float()      # [N][s][5]
        ws = torch.cat([sums.reshape(-1), coef.reshape(-1)])
        if not want_grad:
            return loss, None, ws
        e0, e1 = torch.exp(l0 - mx), torch.exp(l1 - mx)
        inv = 1.0 / (e0 + e1)
        p0, p1 = e0 * inv, e1 * inv
        c = torch.where(s1[..., None], coef[:, 1][:, None], coef[:, 0][:, None])             # [N][HW][5]
        t0, t1 = c[..., 1] * p0 - c[..., 3], c[..., 2] * p1 - c[..., 4]
        dot = t0 + t1
        d = torch.stack([t0 - p0 * dot, t1 - p1 * dot], 1).view(N, 2, H, W)
        return loss, d, ws

    def seg_loss_plain(self, logit, msk, alpha, beta):
        loss, d, _ = self.seg_loss(logit, msk, alpha, beta, 0, 0, True)
        return loss, d

    # ---- lightcnn.hip
    def _pool_arg(self, v):
        """v [..., 4] f32 in window order -> (max, arg) by the kernel's update rule."""
        if self.mut == "pool_nan_loses":
            v = torch.where(torch.isnan(v), torch.full_like(v, float("-inf")), v)
        m, arg = v[..., 0], torch.zeros(v.shape[:-1], dtype=torch.int64)
        for w in range(1, 4):
            c = v[..., w]
            take = (c >= m if self.mut == "pool_last_max_wins" else c > m) | torch.isnan(c)
            m, arg = torch.where(take, c, m), torch.where(take, torch.full_like(arg, w), arg)
        return m, arg

    @staticmethod
    def _windows(x):
        N, H, W, cp = x.shape
        return x.float().view(N, H // 2, 2, W // 2, 2, cp).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, cp, 4)

    def pool2_fwd(self, x):
        v = self._windows(x)
        m, _ = self._pool_arg(v)
        avg = ((v[..., 0] + v[..., 1]) + v[..., 2] + v[..., 3]) * 0.25
        return (m + avg).to(x.dtype)

    def pool2_bwd(self, dy, x):
        N, H, W, cp = x.shape
        _, arg = self._pool_arg(self._windows(x))
        g = dy.float()
        o = torch.stack([torch.where(arg == w, g, torch.zeros(())) + 0.25 * g for w in range(4)], -1)       # [N][P][Q][cp][4]
        return o.view(N, H // 2, W // 2, cp, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, cp).to(x.dtype)

    def mfm_bwd(self, dy, sel, C, czp):
        out = mfm_reference(dy.float(), sel, C, czp)
        if self.mut == "mfm_tie_full_to_both":
            tie = torch.cat([sel[:, :C] == 0, sel[:, :C] == 0], 1)
            out[:, :2 * C] = torch.where(tie, 2.0 * out[:, :2 * C], out[:, :2 * C])
        if self.mut == "mfm_pad_not_zeroed":
            out[:, 2 * C:] = NAN
        return out.to(dy.dtype)

    # ---- x3.hip
    def _split(self, v):
        hi = v.bfloat16()
        rem = v - hi.float()
        if self.mut != "x3_lo_of_infinite_hi":
            rem = torch.where(torch.isinf(hi.float()), torch.zeros_like(v), rem)
        lo = _trunc_bf16(rem) if self.mut == "x3_lo_truncated" else rem.bfloat16()
        return torch.cat([hi, lo, lo if self.mut == "x3_third_plane_lo" else hi], 1)

    @staticmethod
    def _load(t, C):
        return t[:, :C].float() + t[:, C:2 * C].float()

    def x3_from_f32(self, src):
        return self._split(src)

    def x3_to_f32(self, t, C):
        return self._load(t, C)

    def x3_add(self, a, b, C):
        return self._split(self._load(a, C) + self._load(b, C))

    def x3_bn_act(self, x, scale, shift, alpha, res, res_first, C):
        z = self._load(x, C) * (scale if scale is not None else _t32(1.0)) + (shift if shift is not None else _t32(0.0))
        if res is not None and res_first:
            z = z + self._load(res, C)
        if alpha is not None:
            z = torch.where(z > 0, z, z * alpha)
        if res is not None and not res_first:
            z = z + self._load(res, C)
        return self._split(z)

    def x3_fm_fuse(self, x, yf, act, arith, C):
        m, y = _act32(self._load(x, C), act), self._load(yf, C)
        r = (y + m, y - m, y * m, y / m)[arith]
        return self._split(r + y)


CHECKS = {"fm": (check_fm_case, fm_cases), "ew": (check_ew_case, ew_cases), "mse": (check_mse_case, mse_cases),
          "dropout": (check_dropout_case, dropout_cases), "dap": (check_dap_case, dap_cases), "seg": (check_seg_case, seg_cases),
          "pool": (check_pool_case, pool_cases), "mfm": (check_mfm_case, mfm_cases), "x3": (check_x3_case, x3_cases)}


# ------------------------------------------------------------------------------------------------------- refusals
SHAPE, DTYPE, UNSUP, WORKSPACE = -1, -2, -4, -5


def refusal_table(p, pl=None):
    """[(entry point, arguments without the stream, expected status)]: every one is refused on the host, in front of the
    launch, by an MSML_CHECK of fm.hip / seg.hip / lightcnn.hip / x3.hip (or the dtype dispatch).  p: a valid pointer of at
    least 16 KiB (a tensor on the GPU; without a GPU the address of a host buffer, which a refusing call never
    dereferences); pl: one for the `const long*` parameters."""
    pl = p if pl is None else pl
    n, F32, BAD = 64, 0, 7
    # name -> (pointer arguments, indices of those that may be null, arguments from (pointers, n, dtype, act, arith))
    fm = {
        "msml_fm_fuse_fwd": (3, (), lambda q, n, dt, a, r: (*q, n, a, r, dt)),
        "msml_fm_fuse_bwd": (5, (), lambda q, n, dt, a, r: (*q, n, a, r, dt)),
        "msml_fm_act_fwd": (2, (), lambda q, n, dt, a, r: (*q, n, a, dt)),
        "msml_fm_act_bwd": (3, (), lambda q, n, dt, a, r: (*q, n, a, dt)),
        "msml_mul_fwd": (3, (), lambda q, n, dt, a, r: (*q, n, dt)),
        "msml_mul_bwd": (5, (3, 4), lambda q, n, dt, a, r: (*q, n, dt)),
        "msml_axpb": (2, (), lambda q, n, dt, a, r: (*q, n, 1.0, 0.0, dt)),
        "msml_mse_fwd": (4, (), lambda q, n, dt, a, r: (q[0], q[1], n, 40.0, q[2], q[3], 2048, dt)),
        "msml_mse_bwd": (5, (3, 4), lambda q, n, dt, a, r: (q[0], q[1], q[2], 40.0, q[3], q[4], n, dt)),
        "msml_dropout": (2, (), lambda q, n, dt, a, r: (*q, n, 0.5, 1, dt)),
        "msml_dropout_dev": (3, (), lambda q, n, dt, a, r: (q[0], q[1], n, 0.5, q[2], dt)),
    }
    out = []
    for name, (k, optional, args) in fm.items():
        q = [p] * k
        if name == "msml_dropout_dev":
            q[2] = pl
        for bad_n in (0, 7, 12, -8):
            out.append((name, args(q, bad_n, F32, 0, 0), SHAPE))
        out.append((name, args(q, n, BAD, 0, 0), DTYPE))
        for i in range(k):
            if i not in optional:
                qq = list(q)
                qq[i] = None
                # msml_mse_fwd reports its loss / workspace pointers with the workspace code
                out.append((name, args(qq, n, F32, 0, 0), WORKSPACE if name == "msml_mse_fwd" and i >= 2 else SHAPE))
        if "_fm_" in name:
            for a in (-1, 2):
                out.append((name, args(q, n, F32, a, 0), UNSUP))
        if "fm_fuse" in name:
            for r in (-1, 4):
                out.append((name, args(q, n, F32, 0, r), UNSUP))
    for bad_p in (-0.1, 1.0, NAN):
        out.append(("msml_dropout", (p, p, n, bad_p, 1, F32), SHAPE))
        out.append(("msml_dropout_dev", (p, p, n, bad_p, pl, F32), SHAPE))
    # n = 8 * 256 * 3: three partials
    out.append(("msml_mse_fwd", (p, p, 8 * 256 * 3, 40.0, p, p, 2, F32), WORKSPACE))
    for bad_count in (0.0, -1.0):
        out.append(("msml_mse_fwd", (p, p, n, bad_count, p, p, 2048, F32), WORKSPACE))
        out.append(("msml_mse_bwd", (p, p, p, bad_count, p, p, n, F32), SHAPE))
    # seg.hip
    seg = lambda N, ws: (p, pl, N, 2, 4, 10.0, 5.0, 0, 0, p, p, p, ws)
    out += [("msml_seg_consensus_loss_r", seg(3, 59), WORKSPACE), ("msml_seg_consensus_loss_r", seg(0, 60), SHAPE),
            ("msml_seg_consensus_loss", (p, pl, 3, 2, 4, 10.0, 5.0, p, p, p, 59), WORKSPACE),
            ("msml_seg_consensus_loss", (p, pl, 0, 2, 4, 10.0, 5.0, p, p, p, 60), SHAPE),
            ("msml_dap_fwd", (p, p, None, 1, 2, 2, 16, F32), SHAPE), ("msml_dap_fwd", (None, p, None, 1, 2, 2, 24, F32), SHAPE),
            ("msml_dap_fwd", (p, p, None, 1, 2, 2, 24, BAD), DTYPE), ("msml_dap_bwd", (p, p, 1, 2, 2, 20, F32), SHAPE),
            ("msml_dap_bwd", (p, None, 1, 2, 2, 24, F32), SHAPE)]
    # lightcnn.hip
    for name, ptrs in (("msml_pool2_fwd", (p, p)), ("msml_pool2_bwd", (p, p, p))):
        for N, H, W, cp in ((1, 3, 2, 8), (1, 2, 3, 8), (1, 0, 2, 8), (1, 2, 2, 12), (0, 2, 2, 8)):
            out.append((name, (*ptrs, N, H, W, cp, F32), SHAPE))
        out.append((name, (*ptrs, 1, 2, 2, 8, BAD), DTYPE))
        out.append((name, (None,) + ptrs[1:] + (1, 2, 2, 8, F32), SHAPE))
    for M, cp, C, czp in ((4, 8, 8, 8), (4, 3, 4, 8), (4, 8, 4, 12), (0, 8, 4, 8)):    # czp < 2C, cp < C, czp % 8
        out.append(("msml_mfm_bwd", (p, p, p, M, cp, C, czp, F32), SHAPE))
    out += [("msml_mfm_bwd", (p, None, p, 4, 8, 4, 8, F32), SHAPE), ("msml_mfm_bwd", (p, p, p, 4, 8, 4, 8, BAD), DTYPE)]
    # x3.hip
    x3 = {"msml_x3_add": (3, lambda q, M, C: (*q, M, C)), "msml_x3_from_f32": (2, lambda q, M, C: (*q, M, C)),
          "msml_x3_to_f32": (2, lambda q, M, C: (*q, M, C)),
          "msml_x3_fm_fuse_fwd": (3, lambda q, M, C: (*q, M, C, 0, 0)),
          "msml_x3_bn_act_fwd": (2, lambda q, M, C: (q[0], None, None, None, None, 0, q[1], M, C))}
    for name, (k, args) in x3.items():
        q = [p] * k
        out += [(name, args(q, 4, 12), SHAPE), (name, args(q, 0, 8), SHAPE), (name, args(q, 4, 0), SHAPE)]
        for i in range(k):
            qq = list(q)
            qq[i] = None
            out.append((name, args(qq, 4, 8), SHAPE))
    out += [("msml_x3_fm_fuse_fwd", (p, p, p, 4, 8, 2, 0), UNSUP), ("msml_x3_fm_fuse_fwd", (p, p, p, 4, 8, 0, 4), UNSUP)]
    return out
