"""Shared by tests/test_bn_cpu.py and tests/test_gpu_bn.py: the case table of the BatchNorm kernel family
(msml_amd/csrc/bn.hip), a float64 reference, the derived error budgets, a torch restatement of the kernels' f32
arithmetic (with single-fault mutants) and the checks that compare ANY implementation of the entry points -- the
restatement on the CPU, the library on the GPU -- with the reference.

Reference.  Every entry point is compared with the float64 evaluation of the operation it documents, on exactly the
operands it is given (storage-rounded tensors widened to f64, f32 coefficients widened to f64):
  statistics     m = sum x / n, var = sum x^2 / n - m^2, invstd = 1 / sqrt(var + eps), running statistics as nn.BatchNorm
  forward        y = prelu(x * scale + shift [+ r], alpha) [+ r]
  backward       g = dy * prelu'(z) (alpha where z <= 0), xhat = (x - mean) * invstd,
                 dx = scale * (g - sum g / n - xhat * sum g xhat / n) [+ add], dbeta = sum g, dgamma = sum g xhat,
                 dalpha = sum dy min(z, 0), dres = g
`autograd_reference` is F.batch_norm + F.prelu + residual with torch autograd in f64; tests/test_bn_cpu.py shows that it
equals the nn.BatchNorm2d / nn.PReLU modules and that the formulas above equal it, before anything is checked against them.

Budgets.  No tolerance here is a tuned constant: every bound is k * u32 * (sum of the magnitudes of the terms of the
expression) + u_store * |ref|, k counted from the expression written next to it, u32 = 2^-24, ubf = 2^-9; sums use the
recursive-summation bound n_chain * u32 * sum |term| with n_chain the longest f32 chain of the launch (trips of a thread +
lanes of the LDS fold, from the library's own row queries); var / invstd propagate those through E[x^2] - m^2 and
1 / sqrt(var + eps) as an interval.  SAFETY = 2 multiplies every budget, nothing else does.
PReLU's derivative jumps at z = 0: an element whose |z| is within the budget of z itself, but not exactly 0, may take
either branch (its jump |dy| |1 - alpha| joins the budget; such elements are counted).  z == 0 exactly is never excused.
"""
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
UBF = 2.0 ** -9
U64 = 2.0 ** -53
SAFETY = 2.0
EPS = 1e-5
FOLD_MIN_ROWS, FOLD_ROWS, ACC_ROWS = 512, 32, 8     # bn.hip / common.h
EW_GRID_CAP = 768                                   # ew_grid(): workgroups of the element-wise launches
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CS_APPLY = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)        # C / 8 divides 256
CS_REDUCE_ONLY = (24, 96, 192, 320)                          # 256 / (C / 8) not a power of two: thread 255 idle


def f32(v):
    """The double value of float(v) after a round trip through f32 (what a `float` parameter of the ABI carries)."""
    return float(torch.tensor(v, dtype=torch.float32))


def u_store(dtype):
    return UBF if dtype == torch.bfloat16 else U32


Case = namedtuple("Case", "name M C dtype alpha residual res_first affine kind rows tag")


def py_of(C):
    return max(1, 256 // (C // 8))


def stats_rows(M, C):
    """msml_bn_stats_rows (asked from the library: the grid rule under test is the library's, not a copy)."""
    from msml_amd import _lib
    return _lib.value("msml_bn_stats_rows", M, C)


def ew_rows(M, C):
    from msml_amd import _lib
    return _lib.value("msml_bn_act_fwd_stats_rows", M, C)


def slab_chain(M, C, rows):
    """Longest f32 chain of a slab_reduce launch: pixels per thread of the slab + the PY-lane LDS fold."""
    per = -(-M // rows)
    return -(-per // py_of(C)) + py_of(C)


def grid_chain(M, C, g):
    """Longest f32 chain of a STATS / NEXT emission: grid-stride trips of a thread + the 256 / (C/8) lanes that share a
    channel chunk in the workgroup."""
    n8 = M * (C // 8)
    return -(-n8 // (g * 256)) + max(1, 256 // (C // 8))


# ------------------------------------------------------------------------------------------------------ case table
_VARIANTS = [  # alpha, residual, res_first, affine
    (True, True, False, True), (True, False, False, True), (False, False, False, True), (True, True, True, True),
    (False, True, False, True), (True, True, True, False), (False, False, False, False), (True, False, False, False)]


def _m_values(C):
    """(tag, M): the slab boundaries of red_rows() / slab_reduce for this C."""
    p = py_of(C) * 16
    out = [("m1", 1), ("m2", 2), ("m7", 7), ("row-1", p - 1), ("row", p), ("row+1", p + 1)]
    if C in (8, 64, 2048, 24):
        out += [("rows512", 512 * p), ("rows513", 512 * p + 1)]
    if C in (64, 2048, 96):
        # capped: red_rows() clamps at 1024 rows with a remainder: per = p + 1 and, for p <= 1022, (1023 * per >= M) the
        # last block owns an empty slab
        out += [("rows1024", 1024 * p), ("capped", 1024 * p + 1)]
    return out


def slab_geometry_ok(case):
    """The partial-row count the library reports for a case is the one its tag promises (a change of the grid rule or of
    MSML_RED_PPT must not hollow the boundary cases out silently)."""
    if case.rows is not None:           # row count given by the caller, not by the grid rule
        return True
    rows = stats_rows(case.M, case.C)
    per = -(-case.M // rows)
    want = {"m1": 1, "m2": 1, "m7": 1, "row-1": 1, "row": 1, "row+1": 2, "rows512": 512, "rows513": 513, "rows1024": 1024,
            "capped": 1024}.get(case.tag)
    if want is None:
        return True
    return rows == want and (case.tag != "capped" or ((rows - 1) * per >= case.M and case.M > 1024 * py_of(case.C) * 16))


def case_table(group):
    """group: 'reduce' (msml_bn_stats / _acc / msml_bias_grad: every C), 'apply' (entry points with an apply loop),
    'rows' (msml_bn_act_bwd_apply* with the row count given), 'lattice', 'big'."""
    cases, k = [], 0
    if group in ("reduce", "apply"):
        for C in CS_APPLY + (CS_REDUCE_ONLY if group == "reduce" else ()):
            for tag, M in _m_values(C):
                for dt in ("f32", "bf16"):
                    v = _VARIANTS[k % len(_VARIANTS)]
                    k += 1
                    cases.append(Case("%s-C%d-%s-%s" % (group, C, tag, dt), M, C, dt, *v, "normal", None, tag))
        for kind, M, C in (("offset4", 3136, 64), ("offset30", 3136, 64), ("offset30", 50176, 8), ("const", 777, 32),
                           ("padzero", 3136, 128), ("padzero", 100, 256), ("const", 4097, 512)):
            for dt in ("f32", "bf16"):
                v = _VARIANTS[k % 4]            # the four affine variants
                k += 1
                cases.append(Case("%s-%s-M%d-C%d-%s" % (group, kind, M, C, dt), M, C, dt, *v, kind, None, kind))
    elif group == "rows":
        for rows in (1, 32, 512, 513, 5000, 50000):
            for C, M in ((64, 3136), (8, 600), (256, 1000)):
                for dt in ("f32", "bf16"):
                    v = _VARIANTS[k % len(_VARIANTS)]
                    k += 1
                    cases.append(Case("rows%d-C%d-%s" % (rows, C, dt), M, C, dt, v[0], False, False, v[3], "normal", rows,
                                      "rows%d" % rows))
    elif group == "lattice":
        for C, M, rows in ((8, 64, 1), (64, 4096, 32), (256, 1024, 513), (2048, 16, 5), (32, 65536, 1000)):
            for dt in ("f32", "bf16"):
                for v in _VARIANTS[:4]:
                    cases.append(Case("lattice-C%d-M%d-%s-a%dr%df%d" % (C, M, dt, v[0], v[1], v[2]), M, C, dt, *v,
                                      "lattice", rows, "lattice"))
    elif group == "big":     # many grid-stride trips: n8 = M * C / 8 against 768 x 256 threads
        for C, M in ((256, 256 * 14 * 14), (64, 64 * 112 * 112)):
            for dt in ("f32", "bf16"):
                v = _VARIANTS[k % 4]
                k += 1
                cases.append(Case("big-C%d-M%d-%s" % (C, M, dt), M, C, dt, *v, "normal", None, "big"))
    return cases


def draw(case, device="cpu"):
    """Seeded operands of a case, rounded to the storage type.  Returns a dict of tensors on `device`."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    M, C, dt = case.M, case.C, DT[case.dtype]

    def rn(*s):
        return torch.randn(*s, generator=g)
    d = {}
    if case.kind == "lattice":
        def ri(lo, hi, *s):
            return torch.randint(lo, hi + 1, s, generator=g).float()
        d["x"], d["res"], d["dy"] = ri(-3, 3, M, C), ri(-2, 2, M, C), 4.0 * ri(-2, 2, M, C)
        d["add"], d["nx"] = ri(-2, 2, M, C), ri(-3, 3, M, C)
        d["scale"] = torch.tensor([1.0, 2.0, -1.0, 0.5])[torch.arange(C) % 4].clone()
        d["scale"][C // 2:] *= 2.0
        d["shift"] = ri(-2, 2, C) * 2.0           # x * scale + shift: multiples of 0.5, zero on a known share of elements
        d["alpha"] = torch.tensor([0.25, 0.0, -0.5])[torch.arange(C) % 3].clone()
        d["mean"], d["invstd"] = ri(-1, 1, C), torch.tensor([0.5, 1.0])[torch.arange(C) % 2].clone()
        d["nmean"], d["ninvstd"] = ri(-1, 1, C), torch.tensor([1.0, 0.5])[torch.arange(C) % 2].clone()
        d["k1"], d["k2"] = ri(-2, 2, C), ri(-1, 1, C) * 0.5       # sum g / n, sum g xhat / n: given through the rows
        d["k3"] = ri(-3, 3, C)
    else:
        x = rn(M, C)
        sign = 1.0 - 2.0 * (torch.arange(C) % 2)
        if case.kind == "offset4":
            x = x + 4.0 * sign
        elif case.kind == "offset30":
            x = x + 30.0 * sign
        elif case.kind == "const":
            x[:, 0], x[:, 1], x[:, 2] = 1.5, 1.1, -300.0          # exact sums / inexact sums / large m^2 (var clamps at 0)
        d["x"], d["res"], d["dy"], d["add"], d["nx"] = x, rn(M, C), rn(M, C), rn(M, C), rn(M, C) + 0.5
        d["gamma"], d["beta"], d["alpha"] = 1.0 + 0.5 * rn(C), 0.5 * rn(C), 0.25 + 0.1 * rn(C)
        d["rmean0"], d["rvar0"] = 0.3 * rn(C), 1.0 + 0.5 * torch.rand(C, generator=g)
        d["nmean"], d["ninvstd"] = 0.5 + 0.1 * rn(C), 1.0 + 0.2 * torch.rand(C, generator=g)
        d["pre"] = rn(3, C)                                       # gradients already in the arena (accumulate = 1)
        if case.kind == "padzero":                                # pad channels of a map stored wider than the layer
            for k in ("x", "res", "dy", "add", "nx"):
                d[k][:, C - 8:] = 0.0
            for k in ("gamma", "beta", "alpha", "rmean0"):
                d[k][C - 8:] = 0.0
            d["rvar0"][C - 8:] = 1.0
    for k in ("x", "res", "dy", "add", "nx"):
        d[k] = d[k].to(dt)
    if not case.alpha:
        d["alpha"] = None
    if not case.residual:
        d["res"] = None
    if not case.affine and case.kind != "lattice":
        d["gamma"] = d["beta"] = None
    return {k: (v.to(device) if v is not None else None) for k, v in d.items()}


# -------------------------------------------------------------------------------------------------- f64 reference
def w(t):
    return None if t is None else t.double()


def autograd_reference(x, gamma, beta, alpha, res, res_first, dy, rmean0, rvar0, momentum, eps, training=True):
    """F.batch_norm + F.prelu + residual in f64 on [M][C] operands, backward by autograd.  Returns a dict."""
    x = w(x).clone().requires_grad_(True)
    leaves = {"dx": x}
    p = {}
    for n, t in (("dgamma", gamma), ("dbeta", beta), ("dalpha", alpha), ("dres", res)):
        p[n] = None if t is None else w(t).clone().requires_grad_(True)
        if t is not None:
            leaves[n] = p[n]
    rm, rv = w(rmean0).clone(), w(rvar0).clone()
    z = F.batch_norm(x, rm, rv, p["dgamma"], p["dbeta"], training, momentum, eps)
    if res is not None and res_first:
        z = z + p["dres"]
    if alpha is not None:
        z = F.prelu(z, p["dalpha"])
    if res is not None and not res_first:
        z = z + p["dres"]
    out = {"y": z.detach(), "rmean": rm, "rvar": rv}
    if dy is not None:
        grads = torch.autograd.grad(z, list(leaves.values()), w(dy))
        out.update(dict(zip(leaves, grads)))
    return out


def stats_reference(x, count=None):
    x = w(x)
    n = float(x.shape[0] if count is None else count)
    s, ss = x.sum(0), (x * x).sum(0)
    m = s / n
    var = (ss / n - m * m).clamp_min(0.0)
    return {"s": s, "ss": ss, "sabs": x.abs().sum(0), "m": m, "var": var, "n": n}


def coef_reference(st, gamma, beta, rmean0, rvar0, momentum, eps):
    """What msml_bn_finalize / msml_bn_fin_act_fwd derive from the sums, in f64."""
    C = st["m"].numel()
    g = w(gamma) if gamma is not None else torch.ones(C, dtype=torch.float64, device=st["m"].device)
    b = w(beta) if beta is not None else torch.zeros(C, dtype=torch.float64, device=st["m"].device)
    inv = 1.0 / torch.sqrt(st["var"] + eps)
    n = st["n"]
    unb = st["var"] * (n / (n - 1.0)) if n > 1 else st["var"]     # count == 1 keeps the biased one, as k_bn_finalize
    out = {"mean": st["m"], "invstd": inv, "scale": g * inv, "shift": b - st["m"] * g * inv, "g": g, "b": b, "unb": unb}
    if rmean0 is not None:
        out["rmean"] = (1.0 - momentum) * w(rmean0) + momentum * st["m"]
        out["rvar"] = (1.0 - momentum) * w(rvar0) + momentum * unb
    return out


def coef_budget(st, cf, chain, momentum, eps, rmean0=None, rvar0=None, ds=None, dss=None):
    """Budgets of (mean, invstd, scale, shift, rmean, rvar).  ds / dss: bounds on the sums (default: one slab launch)."""
    n = st["n"]
    ds = chain * U32 * st["sabs"] if ds is None else ds                  # q += x: chain adds
    dss = (chain + 1) * U32 * st["ss"] if dss is None else dss           # q += x * x: one product more
    dm, de2 = ds / n, dss / n
    dvar = de2 + 2.0 * st["m"].abs() * dm + dm * dm                      # E[x^2] - m^2, both in f64 on the device
    inv = cf["invstd"]
    lo = 1.0 / torch.sqrt(st["var"] + dvar + eps)
    hi = 1.0 / torch.sqrt((st["var"] - dvar).clamp_min(0.0) + eps)       # the kernel clamps var < 0 to 0
    dmean = dm + U32 * st["m"].abs()                                     # (float)m
    dinv = torch.maximum(hi - inv, inv - lo) + U32 * inv                 # (float)(1 / sqrt(var + eps))
    g, b = cf["g"].abs(), cf["b"].abs()
    out = {"mean": dmean, "invstd": dinv, "var": dvar,
           "scale": g * dinv + U32 * cf["scale"].abs(),                  # g * invstd: 1 op
           # b - mean * g * invstd: 3 ops on |b| + |mean g invstd|
           "shift": g * (dmean * (inv + dinv) + st["m"].abs() * dinv) + 3 * U32 * (b + (st["m"] * cf["scale"]).abs())}
    if rmean0 is not None:
        f = n / (n - 1.0) if n > 1 else 1.0
        a = abs(1.0 - momentum)
        # (1 - mom) * r + mom * v: 4 ops (1 - mom, two products, the sum) on |(1 - mom) r| + |mom v|; (float)unbiased: 1 op
        out["rmean"] = momentum * dmean + 4 * U32 * (a * w(rmean0).abs() + momentum * st["m"].abs())
        out["rvar"] = momentum * f * (dvar + U32 * st["var"]) + 4 * U32 * (a * w(rvar0).abs() + momentum * cf["unb"])
    return out


def _bc(v, like, dflt):
    if v is None:
        return torch.full((like.shape[1],), dflt, dtype=torch.float64, device=like.device)
    return w(v)


def fwd_reference(x, scale, shift, alpha, res, res_first, dtype, dscale=None, dshift=None):
    """y = prelu(x * scale + shift [+ r]) [+ r] in f64 and its budget.  dscale / dshift: bounds on the coefficients the
    kernel derived itself (None: they are inputs, exact)."""
    x, sc, sh = w(x), w(scale), w(shift)
    r = w(res) if res is not None else None
    z = x * sc + sh
    mag = (x * sc).abs() + sh.abs()
    k = 2                                                                # z = x * sc + sh: 2 ops
    if r is not None and res_first:
        z = z + r
        mag = mag + r.abs()
        k += 1                                                           # + r
    ez = k * U32 * mag
    if dscale is not None:
        ez = ez + x.abs() * dscale + dshift
    y, ey = z, ez
    if alpha is not None:
        a = w(alpha)
        y = torch.where(z > 0, z, z * a)
        # a sign flip of z within ez moves y by at most max(1, |a|) ez; z * a: 1 op
        ey = ez * a.abs().clamp_min(1.0) + U32 * y.abs()
    if r is not None and not res_first:
        y = y + r
        ey = ey + U32 * y.abs()                                          # + r: 1 op
    return {"y": y, "y_budget": ey + u_store(dtype) * y.abs(), "z": z if alpha is not None else None, "ez": ez}


def bwd_reference(dy, x, scale, shift, alpha, mean, invstd, res_first_res, dtype, chain, sums=None, dsums=None,
                  add=None, pre=None, dcoef=None):
    """The backward formulas in f64 and their budgets.  sums = (s0, s1, s2) given by the caller through partial rows /
    accumulators (then dsums bounds what the fold may add), else the reduce pass of the entry point computes them.
    dcoef = {scale, shift, mean, invstd}: bounds on coefficients the implementation derived itself (first order)."""
    dy, x, sc, mu, inv = w(dy), w(x), w(scale), w(mean), w(invstd)
    n = float(x.shape[0])
    gg, egg, ez, zneg = dy, torch.zeros_like(dy), None, None
    amb = 0
    if alpha is not None:
        f = fwd_reference(x, scale, shift, None, res_first_res, True, dtype, *((dcoef["scale"], dcoef["shift"]) if dcoef else ()))
        z, ez, a = f["y"], f["ez"], w(alpha)
        neg = z <= 0
        ambig = (z != 0) & (z.abs() <= SAFETY * ez)                      # may take either PReLU branch, see the module text
        amb = int(ambig.sum())
        gg = torch.where(neg, dy * a, dy)
        egg = U32 * gg.abs() * neg + ambig * (dy * (1.0 - a)).abs()      # dy * a: 1 op
        zneg = torch.where(neg, z, torch.zeros_like(z))
    xh = (x - mu) * inv
    exh = 2 * U32 * xh.abs()                                             # (x - mu) * is: 2 ops
    if dcoef:
        exh = exh + dcoef["mean"] * inv.abs() + (x - mu).abs() * dcoef["invstd"]
    out = {"dres": gg, "dres_budget": egg + u_store(dtype) * gg.abs(), "ambiguous": amb}
    if sums is None:
        s0, s1 = gg.sum(0), (gg * xh).sum(0)
        d0 = chain * U32 * gg.abs().sum(0) + egg.sum(0)                  # q0 += gg
        d1 = (chain + 1) * U32 * (gg * xh).abs().sum(0) + (egg * xh.abs() + gg.abs() * exh).sum(0)   # q1 += gg * xh
        if alpha is not None:
            s2 = (dy * zneg).sum(0)                                      # q2 += gg * z where z <= 0
            d2 = (chain + 1) * U32 * (dy * zneg).abs().sum(0) + (dy.abs() * ez * (neg | ambig)).sum(0)
        else:
            s2, d2 = torch.zeros_like(s0), torch.zeros_like(s0)
    else:
        (s0, s1, s2), (d0, d1, d2) = sums, dsums
    k1, k2 = s0 / n, s1 / n
    dk1, dk2 = d0 / n + U32 * k1.abs(), d1 / n + U32 * k2.abs()          # (float)(s / count)
    inner = gg - k1 - xh * k2
    # gg - k1 - xh * k2: 3 ops on |gg| + |k1| + |xh k2|
    e_in = egg + dk1 + exh * k2.abs() + xh.abs() * dk2 + 3 * U32 * (gg.abs() + k1.abs() + (xh * k2).abs())
    dx = sc * inner
    edx = sc.abs() * e_in + U32 * dx.abs()                               # sc * (...): 1 op
    if dcoef:
        edx = edx + dcoef["scale"] * (inner.abs() + e_in)
    if add is not None:
        dx = dx + w(add)
        edx = edx + U32 * dx.abs()                                       # + add: 1 op
    out.update(dx=dx, dx_budget=edx + u_store(dtype) * dx.abs())
    for i, (nm, s, d) in enumerate((("dbeta", s0, d0), ("dgamma", s1, d1), ("dalpha", s2, d2))):
        p = w(pre[i]) if pre is not None else 0.0
        out[nm] = s + p
        out[nm + "_budget"] = d + U32 * s.abs() + (U32 * (s + p).abs() if pre is not None else 0.0)   # (float)s, prev + s
    return out


def emitted_reference(stored, M, C, g, nx=None, nmean=None, ninvstd=None, acc=False):
    """The sums STATS / NEXT must emit, in f64 from the tensor the DEVICE STORED (they are defined on the rounded values)."""
    t = w(stored)
    chain = grid_chain(M, C, g)
    fold = (g * U64) if acc else 0.0                                     # f64 adds of g partials
    if nx is None:
        q0, q1 = t, t * t
        k1 = 1                                                           # v * v: 1 op
    else:
        q0, q1 = t, t * ((w(nx) - w(nmean)) * w(ninvstd))
        k1 = 3                                                           # o * ((xn - nmu) * nis): 3 ops
    return {"q0": q0.sum(0), "q1": q1.sum(0), "q0_budget": (chain * U32 + fold) * q0.abs().sum(0),
            "q1_budget": ((chain + k1) * U32 + fold) * q1.abs().sum(0)}


def scatter_s2(compact, N, H, W):
    """Dense [N*H*W][C] gradient of a 1x1 / stride-2 / pad-0 conv from the compact [N][ceil(H/2)][ceil(W/2)][C]."""
    C = compact.shape[-1]
    dense = torch.zeros(N, H, W, C, dtype=compact.dtype, device=compact.device)
    dense[:, ::2, ::2] = compact.view(N, (H + 1) // 2, (W + 1) // 2, C)
    return dense.view(N * H * W, C)


def split_rows(total, rows, gen, lattice=False):
    """`rows` random f32 pieces [rows][C] and their f64 total (the known sum a caller of msml_bn_act_bwd_apply holds).
    lattice: integer pieces that sum to `total` exactly."""
    if lattice:
        p = torch.randint(-4, 5, (rows, total.numel()), generator=gen).double()
        p[0] += total.cpu().double() - p.sum(0)
        return p.float(), p.sum(0)
    t = total.cpu().double()
    p = ((t / rows) * (1.0 + 0.5 * torch.randn(rows, t.numel(), generator=gen, dtype=torch.float64))).float()
    return p, p.double().sum(0)


def rows_fold_budget(pieces):
    """What the f64 fold of given partial rows may lose: rows > 512 go through 32 f32 folded rows (k_fold_rows)."""
    a = pieces.double().abs().sum(0)
    rows = pieces.shape[0]
    return ((U32 if rows > FOLD_MIN_ROWS else 0.0) + (rows + 40) * U64) * a


# ---------------------------------------------------------------------------------------------------- comparison
class Report:
    """Worst error / budget per (entry point, dtype); every check asserts error <= SAFETY * budget."""

    def __init__(self):
        self.worst = {}
        self.failures = []
        self.ambiguous = 0
        self.offset = {}          # (data kind, dtype, quantity) -> (worst error / budget, worst relative error): offset cases

    def check(self, key, what, got, ref, budget, case):
        got = got.double()
        assert got.shape == ref.shape, (key, what, got.shape, ref.shape)
        if not bool(torch.isfinite(got).all()):
            self.failures.append((key, what, case.name, float("inf")))
            return float("inf")
        err = (got - ref).abs()
        b = SAFETY * (budget if torch.is_tensor(budget) else torch.full_like(err, budget))
        b = b.expand_as(err)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(b).all()), ("reference or budget not finite", key, what, case.name)
        ratio = torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
        r = float(ratio.max()) if ratio.numel() else 0.0
        k = (key, case.dtype)
        n, old, oc = self.worst.get(k, (0, 0.0, ""))
        self.worst[k] = (n + 1, max(old, r), case.name + ":" + what if r >= old else oc)
        if r > 1.0:
            self.failures.append((key, what, case.name, r))
        if case.kind.startswith("offset") and what in ("invstd", "mean", "rvar", "y", "dx acc=0"):
            rel = float((err / ref.abs().clamp_min(1e-300)).max()) if what in ("invstd", "rvar") else float("nan")
            ko = (case.kind, case.dtype, key + ":" + what)
            o = self.offset.get(ko, (0.0, 0.0))
            self.offset[ko] = (max(o[0], r), max(o[1], rel) if rel == rel else rel)
        return r

    def exact(self, key, what, got, ref, case):
        ok = torch.equal(got.double(), ref.double())
        k = (key, case.dtype)
        n, old, oc = self.worst.get(k, (0, 0.0, ""))
        self.worst[k] = (n + 1, old, oc)
        if not ok:
            self.failures.append((key, what + " (exact)", case.name, float("inf")))
        return ok

    def table(self):
        lines = ["%-28s %-5s %6s  %-10s %s" % ("entry point", "dtype", "cases", "worst e/b", "at")]
        for (key, dt), (n, r, at) in sorted(self.worst.items()):
            lines.append("%-28s %-5s %6d  %-10.3g %s" % (key, dt, n, r, at))
        for (kind, dt, q), (r, rel) in sorted(self.offset.items()):
            lines.append("offset case %-9s %-5s %-38s e/b %-9.3g relative error %.3g" % (kind, dt, q, r, rel))
        return "\n".join(lines)


# ------------------------------------------------------------------------- torch restatement of the kernels' arithmetic
MUTANTS = ("count_plus_1", "biased_running_var", "z_lt_0", "res_first_ignored_bwd", "k2_no_count", "xhat_with_scale",
           "coef_next_chunk_2nd_trip", "stats_unrounded", "add_on_odd_pixels", "accumulate_ignored", "dalpha_over_pos")


def _two_level(v, idx):
    """f32 sums in the kernels' order: idx [blocks][trips][lanes] pixel numbers (M = nothing); a thread chains its trips,
    the workgroup chains its lanes.  -> rows [blocks][C]."""
    ve = torch.cat([v, torch.zeros(1, v.shape[1], dtype=v.dtype)])
    acc = torch.zeros(idx.shape[0], idx.shape[2], v.shape[1])
    for k in range(idx.shape[1]):
        acc = acc + ve[idx[:, k]]
    s = torch.zeros(idx.shape[0], v.shape[1])
    for y in range(idx.shape[2]):
        s = s + acc[:, y]
    return s


def _slab_idx(M, C, rows):
    PY, per = py_of(C), -(-M // rows)
    K = -(-per // PY)
    off = torch.arange(K).view(1, K, 1) * PY + torch.arange(PY).view(1, 1, PY)
    pix = torch.arange(rows).view(rows, 1, 1) * per + off
    return torch.where((off < per) & (pix < M), pix, torch.full_like(pix, M))


def _grid_idx(M, C, g):
    lpb = 256 // (C // 8)
    K = -(-M // (g * lpb))
    pix = (torch.arange(g).view(g, 1, 1) * lpb + torch.arange(lpb).view(1, 1, lpb)) + torch.arange(K).view(1, K, 1) * (g * lpb)
    return torch.where(pix < M, pix, torch.full_like(pix, M))


class Restatement:
    """The entry points of bn.hip in torch: f32 operations in the kernels' order, f64 where they use it, storage rounding
    where they store.  `mutant` plants one fault (MUTANTS).  CPU tensors."""
    name = "restatement"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mut = mutant

    # msml_bn_stats [+ msml_bn_finalize] / msml_bn_stats_acc: f64 totals of the f32 partial rows
    def stats(self, x, proto="rows"):
        M, C = x.shape
        v = x.float()
        idx = _slab_idx(M, C, stats_rows(M, C))
        return _two_level(v, idx).double().sum(0), _two_level(v * v, idx).double().sum(0)

    def _finalize(self, s, ss, count, gamma, beta, rmean, rvar, momentum, eps):
        if self.mut == "count_plus_1":
            count = count + 1.0
        m = s / count
        var = (ss / count - m * m).clamp_min(0.0)
        mean, inv = m.float(), (1.0 / torch.sqrt(var + eps)).float()
        if rmean is not None:
            unb = var * count / (count - 1.0) if count > 1.0 and self.mut != "biased_running_var" else var
            mom = torch.tensor(momentum, dtype=torch.float32)
            rmean.copy_((1.0 - mom) * rmean + mom * mean)
            rvar.copy_((1.0 - mom) * rvar + mom * unb.float())
        g = gamma if gamma is not None else torch.ones_like(mean)
        b = beta if beta is not None else torch.zeros_like(mean)
        return g * inv, b - mean * g * inv, mean, inv

    def bn_train(self, x, gamma, beta, rmean, rvar, momentum, eps, proto="rows"):
        s, ss = self.stats(x)
        return self._finalize(s, ss, float(x.shape[0]), gamma, beta, rmean, rvar, momentum, eps)

    def finalize_eval(self, gamma, beta, rmean, rvar, eps):
        inv = 1.0 / torch.sqrt(rvar + torch.tensor(eps, dtype=torch.float32))
        g = gamma if gamma is not None else torch.ones_like(inv)
        b = beta if beta is not None else torch.zeros_like(inv)
        return g * inv, b - rmean * g * inv

    def _second_trip(self, M, C, t):
        """Coefficients a thread would hold for chunk (tid + 1) % C8 from its second grid-stride trip on."""
        if self.mut != "coef_next_chunk_2nd_trip":
            return None
        g = ew_rows(M, C)
        first = g * 256 // (C // 8)                   # pixels of the first trip
        return first if first < M else None

    def _apply_coef(self, M, C, coefs):
        first = self._second_trip(M, C, None)
        out = []
        for c in coefs:
            if c is None:
                out.append(None)
                continue
            full = c.view(1, C).expand(M, C)
            if first is not None:
                full = torch.cat([full[:first], torch.roll(c, -8).view(1, C).expand(M - first, C)])
            out.append(full)
        return out

    # msml_bn_act_fwd[_stats] (proto 'rows') / the apply half of msml_bn_fin_act_fwd (proto 'acc')
    def act_fwd(self, x, scale, shift, alpha, res, res_first, emit=False, proto="rows"):
        M, C = x.shape
        sc, sh, al = self._apply_coef(M, C, (scale, shift, alpha))
        z = x.float() * sc + sh
        if res is not None and res_first:
            z = z + res.float()
        if alpha is not None:
            z = torch.where(z > 0, z, z * al)
        if res is not None and not res_first:
            z = z + res.float()
        y = z.to(x.dtype)
        if not emit:
            return y, None
        v = z if self.mut == "stats_unrounded" else y.float()
        idx = _grid_idx(M, C, ew_rows(M, C))
        return y, (_two_level(v, idx).double().sum(0), _two_level(v * v, idx).double().sum(0))

    # msml_bn_stats_acc + msml_bn_fin_act_fwd
    def fin_act_fwd(self, x, gamma, beta, rmean, rvar, momentum, eps, alpha, res, res_first, emit):
        coef = self.bn_train(x, gamma, beta, rmean, rvar, momentum, eps)
        y, em = self.act_fwd(x, coef[0], coef[1], alpha, res, res_first, emit)
        return coef, y, em

    def _bwd_terms(self, dy, x, sc, sh, al, mu, inv, res, for_apply):
        gg = dy.float()
        q2 = torch.zeros_like(gg)
        if al is not None:
            z = x.float() * sc + sh
            if res is not None and not (for_apply and self.mut == "res_first_ignored_bwd"):
                z = z + res.float()
            neg = (z < 0) if self.mut == "z_lt_0" else (z <= 0)
            q2 = torch.where((z > 0) if self.mut == "dalpha_over_pos" else neg, gg * z, q2)
            gg = torch.where(neg, gg * al, gg)
        xh = (x.float() - mu) * (sc if self.mut == "xhat_with_scale" else inv)
        return gg, xh, q2

    def _bwd_finish(self, s, count, grads, accumulate, dy, x, scale, shift, alpha, mean, invstd, res, add, nxt):
        M, C = x.shape
        acc = accumulate and self.mut != "accumulate_ignored"
        for i, gr in enumerate(grads):
            if gr is not None:
                gr.copy_((gr if acc else torch.zeros_like(gr)) + s[i].float())
        k1 = (s[0] / count).float()
        k2 = (s[1] if self.mut == "k2_no_count" else s[1] / count).float()
        sc, sh, al, mu, inv, k1, k2 = self._apply_coef(M, C, (scale, shift, alpha, mean, invstd, k1, k2))
        gg, xh, _ = self._bwd_terms(dy, x, sc, sh, al, mu, inv, res, True)
        v = sc * (gg - k1 - xh * k2)
        if add is not None:
            v = v + add.float()
        dx, dres = v.to(x.dtype), (gg.to(x.dtype) if res is not None else None)
        em = None
        if nxt is not None:
            nx, nm, ni = nxt
            o = dx.float()
            idx = _grid_idx(M, C, ew_rows(M, C))
            em = (_two_level(o, idx).double().sum(0), _two_level(o * ((nx.float() - nm) * ni), idx).double().sum(0))
        return dx, dres, em

    # msml_bn_act_bwd (proto 'rows') / msml_bn_act_bwd_acc (proto 'acc'); grads = [dbeta, dgamma, dalpha] updated in place
    def act_bwd(self, dy, x, scale, shift, alpha, mean, invstd, res, grads, accumulate, proto="rows", add=None):
        M, C = x.shape
        gg, xh, q2 = self._bwd_terms(dy, x, scale, shift, alpha, mean, invstd, res, False)
        idx = _slab_idx(M, C, stats_rows(M, C))
        s = [_two_level(t, idx).double().sum(0) for t in (gg, gg * xh, q2)]
        dx, dres, _ = self._bwd_finish(s, float(M), grads, accumulate, dy, x, scale, shift, alpha, mean, invstd, res, add, None)
        return dx, dres

    # msml_bn_act_bwd_apply[_next][_s2] (proto 'rows': pieces [rows][3][C] f32) / msml_bn_fin_bwd_apply (proto 'acc')
    def bwd_apply(self, dy, x, scale, shift, alpha, mean, invstd, pieces, grads, accumulate, add=None, add_hw=None,
                  nxt=None, proto="rows", res=None):
        M, C = x.shape
        rows = pieces.shape[0]
        if proto == "rows" and rows > FOLD_MIN_ROWS:
            chunk = -(-rows // FOLD_ROWS)
            pieces = torch.stack([pieces[b * chunk:(b + 1) * chunk].double().sum(0).float() for b in range(FOLD_ROWS)])
        s = list(pieces.double().sum(0))
        if add_hw is not None:
            H, W = add_hw
            if self.mut == "add_on_odd_pixels":
                dense = torch.zeros(M // (H * W), H, W, C, dtype=add.dtype)
                dense[:, 1::2, 1::2] = add.view(M // (H * W), (H + 1) // 2, (W + 1) // 2, C)[:, :H // 2, :W // 2]
                add = dense.view(M, C)
            else:
                add = scatter_s2(add, M // (H * W), H, W)
        dx, dres, em = self._bwd_finish(s, float(M), grads, accumulate, dy, x, scale, shift, alpha, mean, invstd, res, add, nxt)
        return dx, dres, em

    def bias_grad(self, dy, creal, db, accumulate):
        s, _ = self.stats(dy)
        db.copy_((db if accumulate else torch.zeros_like(db)) + s[:creal].float())

    def add(self, a, b):
        return (a.float() + b.float()).to(a.dtype)


# ------------------------------------------------------------------------------------- the checks, for any backend
MOMENTA = (0.1, 1.0)


def check_reduce_case(be, case, rep, device="cpu"):
    """msml_bn_stats + msml_bn_finalize (train, eval), msml_bn_stats_acc + msml_bn_fin_act_fwd's coefficients,
    msml_bias_grad."""
    d = draw(case, device)
    x, M, C = d["x"], case.M, case.C
    eps = f32(EPS)
    st = stats_reference(x)
    chain = slab_chain(M, C, stats_rows(M, C))
    for proto in ("rows", "acc"):
        if proto == "acc" and 256 % (C // 8):
            continue                                   # msml_bn_fin_act_fwd refuses these C (checked by the refusal test)
        mom = f32(MOMENTA[(zlib.crc32(case.name.encode()) + (proto == "acc")) % 2])
        cf = coef_reference(st, d["gamma"], d["beta"], d["rmean0"], d["rvar0"], mom, eps)
        bud = coef_budget(st, cf, chain, mom, eps, d["rmean0"], d["rvar0"])
        rm, rv = d["rmean0"].clone(), d["rvar0"].clone()
        sc, sh, mean, inv = be.bn_train(x, d["gamma"], d["beta"], rm, rv, mom, eps, proto=proto)
        key = "bn_stats+finalize" if proto == "rows" else "bn_stats_acc+fin_act_fwd"
        for nm, got in (("scale", sc), ("shift", sh), ("mean", mean), ("invstd", inv), ("rmean", rm), ("rvar", rv)):
            rep.check(key, nm, got, cf[nm], bud[nm], case)
        if case.kind == "const":                       # sums of 1.5 are exact in f32: var == 0 exactly, no budget needed
            rep.exact(key, "const mean", mean[0], torch.tensor(1.5, device=mean.device), case)
            rep.exact(key, "const invstd", inv[0], torch.tensor(1.0 / math.sqrt(eps), device=mean.device).float(), case)
    # eval mode (rows == 0): coefficients from the running statistics, all f32: g * (1 / sqrt(rv + eps)): 4 ops;
    # b - rm * g * invstd: 2 more on |b| + |rm scale|
    g = _bc(d["gamma"], x, 1.0)
    b = _bc(d["beta"], x, 0.0)
    inv = 1.0 / torch.sqrt(w(d["rvar0"]) + eps)
    sc, sh = be.finalize_eval(d["gamma"], d["beta"], d["rmean0"], d["rvar0"], eps)
    rep.check("bn_finalize(eval)", "scale", sc, g * inv, 4 * U32 * (g * inv).abs(), case)
    rep.check("bn_finalize(eval)", "shift", sh, b - w(d["rmean0"]) * g * inv,
              6 * U32 * (b.abs() + (w(d["rmean0"]) * g * inv).abs()), case)
    # msml_bias_grad: column sums of the first Creal channels, accumulate
    creal = C - 3 if C > 8 else C
    for accumulate in (0, 1):
        db = d["pre"][0, :creal].clone()
        be.bias_grad(d["dy"], creal, db, accumulate)
        dyw = w(d["dy"])[:, :creal]
        ref = dyw.sum(0) + (w(d["pre"][0, :creal]) if accumulate else 0.0)
        rep.check("bias_grad", "db acc=%d" % accumulate, db, ref,
                  chain * U32 * dyw.abs().sum(0) + U32 * dyw.sum(0).abs() + U32 * ref.abs(), case)


def check_apply_case(be, case, rep, device="cpu", protos=("rows", "acc")):
    """Forward and backward entry points with an apply loop, coefficients from the backend's own finalize (so they are
    the f32 values a training step would hand over), each compared with f64 of exactly those inputs."""
    d = draw(case, device)
    x, M, C, dt = d["x"], case.M, case.C, DT[case.dtype]
    eps, mom = f32(EPS), f32(0.1)
    res, rf, alpha = d["res"], int(case.res_first and case.residual), d["alpha"]
    st = stats_reference(x)
    cf = coef_reference(st, d["gamma"], d["beta"], d["rmean0"], d["rvar0"], mom, eps)
    sc, sh, mean, inv = be.bn_train(x, d["gamma"], d["beta"], d["rmean0"].clone(), d["rvar0"].clone(), mom, eps)
    g_ew = ew_rows(M, C)
    pad = slice(C - 8, C) if case.kind == "padzero" else None
    # ---- forward, coefficients given
    ref = fwd_reference(x, sc, sh, alpha, res, rf, dt)
    for emit in (False, True):
        key = "bn_act_fwd_stats" if emit else "bn_act_fwd"
        y, em = be.act_fwd(x, sc, sh, alpha, res, rf, emit=emit, proto="rows")
        rep.check(key, "y", y, ref["y"], ref["y_budget"], case)
        if pad is not None:
            rep.exact(key, "pad channels of y", y[:, pad], torch.zeros(M, 8, device=y.device), case)
        if emit:
            er = emitted_reference(y, M, C, g_ew)
            rep.check(key, "sum", em[0], er["q0"], er["q0_budget"], case)
            rep.check(key, "sumsq", em[1], er["q1"], er["q1_budget"], case)
    # ---- forward, one launch from the accumulator: against the FULL f64 BatchNorm, coefficient budgets included
    if "acc" in protos:
        bud = coef_budget(st, cf, slab_chain(M, C, stats_rows(M, C)), mom, eps, d["rmean0"], d["rvar0"])
        full = fwd_reference(x, cf["scale"], cf["shift"], alpha, res, rf, dt, bud["scale"], bud["shift"])
        rm, rv = d["rmean0"].clone(), d["rvar0"].clone()
        for emit in (False, True):
            coef2, y, em = be.fin_act_fwd(x, d["gamma"], d["beta"], rm if not emit else rm.clone(),
                                          rv if not emit else rv.clone(), mom, eps, alpha, res, rf, emit)
            rep.check("bn_fin_act_fwd", "y", y, full["y"], full["y_budget"], case)
            rep.check("bn_fin_act_fwd", "scale", coef2[0], cf["scale"], bud["scale"], case)
            rep.check("bn_fin_act_fwd", "shift", coef2[1], cf["shift"], bud["shift"], case)
            if emit:
                er = emitted_reference(y, M, C, g_ew, acc=True)
                rep.check("bn_fin_act_fwd", "acc_out sum", em[0], er["q0"], er["q0_budget"], case)
                rep.check("bn_fin_act_fwd", "acc_out sumsq", em[1], er["q1"], er["q1_budget"], case)
        rep.check("bn_fin_act_fwd", "rmean", rm, cf["rmean"], bud["rmean"], case)
        rep.check("bn_fin_act_fwd", "rvar", rv, cf["rvar"], bud["rvar"], case)
    # ---- backward with its own reduce pass
    resb = res if rf else None
    chain = slab_chain(M, C, stats_rows(M, C))
    for proto in protos:
        key = "bn_act_bwd" if proto == "rows" else "bn_act_bwd_acc"
        for accumulate, with_dalpha in ((0, True), (1, True), (0, False)):
            pre = d["pre"] if accumulate else None
            br = bwd_reference(d["dy"], x, sc, sh, alpha, mean, inv, resb, dt, chain, pre=pre)
            rep.ambiguous += br["ambiguous"]
            grads = [d["pre"][0].clone(), d["pre"][1].clone(), d["pre"][2].clone() if with_dalpha else None]
            dx, dres = be.act_bwd(d["dy"], x, sc, sh, alpha, mean, inv, resb, grads, accumulate, proto=proto)
            tag = " acc=%d" % accumulate
            rep.check(key, "dx" + tag, dx, br["dx"], br["dx_budget"], case)
            if resb is not None:
                rep.check(key, "dres" + tag, dres, br["dres"], br["dres_budget"], case)
            for i, nm in enumerate(("dbeta", "dgamma", "dalpha")):
                if grads[i] is not None:
                    rep.check(key, nm + tag, grads[i], br[nm], br[nm + "_budget"], case)
            if pad is not None:
                rep.exact(key, "pad channels of dx", dx[:, pad], torch.zeros(M, 8, device=dx.device), case)
        if proto == "acc":            # msml_bn_act_bwd_acc also takes `add`, the other gradient path joining at the input
            br = bwd_reference(d["dy"], x, sc, sh, alpha, mean, inv, resb, dt, chain, add=d["add"])
            grads = [torch.zeros(C, device=x.device) for _ in range(3)]
            dx, dres = be.act_bwd(d["dy"], x, sc, sh, alpha, mean, inv, resb, grads, 0, proto=proto, add=d["add"])
            rep.check(key, "dx with add", dx, br["dx"], br["dx_budget"], case)
            rep.check(key, "dbeta with add", grads[0], br["dbeta"], br["dbeta_budget"], case)


def _hw_of(M):
    """An odd-sided (H, W) with M % (H * W) == 0 when there is one (the compact `add` then has ceil() sides)."""
    for H, W in ((7, 7), (5, 3), (3, 1), (14, 14), (2, 3), (4, 4), (2, 2), (1, 1)):
        if M % (H * W) == 0:
            return H, W


def check_rows_case(be, case, rep, device="cpu", protos=("rows", "acc")):
    """msml_bn_act_bwd_apply / _next / _s2 / _next_s2 (given partial rows) and msml_bn_fin_bwd_apply (given accumulator) in
    the four NEXT x S2 forms.  Lattice cases compare with torch.equal."""
    d = draw(case, device)
    x, M, C, dt = d["x"], case.M, case.C, DT[case.dtype]
    lat = case.kind == "lattice"
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) + 1)
    alpha = d["alpha"]
    resb = d["res"] if (case.res_first and case.residual) else None
    if lat:
        sc, sh, mean, inv = d["scale"], d["shift"], d["mean"], d["invstd"]
        totals = [d["k1"].double() * M, d["k2"].double() * M, d["k3"].double()]
    else:
        eps, mom = f32(EPS), f32(0.1)
        sc, sh, mean, inv = be.bn_train(x, d["gamma"], d["beta"], d["rmean0"].clone(), d["rvar0"].clone(), mom, eps)
        free = bwd_reference(d["dy"], x, sc, sh, alpha, mean, inv, resb, dt, 1)
        totals = [free["dbeta"], free["dgamma"], free["dalpha"]]
    H, W = _hw_of(M)
    N = M // (H * W)
    compact = d["add"][:N * ((H + 1) // 2) * ((W + 1) // 2)].contiguous()
    g_ew = ew_rows(M, C)
    for proto in protos:
        rows = case.rows if proto == "rows" else ACC_ROWS
        ps = [split_rows(t, rows, gen, lat) for t in totals]
        pieces = torch.stack([p[0] for p in ps], 1).to(x.device)                   # [rows][3][C]
        sums = [p[1].to(x.device) for p in ps]
        dsums = [rows_fold_budget(p[0]).to(x.device) if proto == "rows" else (rows + 40) * U64 * p[0].double().abs().sum(0).to(x.device)
                 for p in ps]
        for nxt_on in (False, True):
            for addkind in ("none", "dense", "s2"):
                res_arg = None if proto == "rows" else resb         # the row entry points take no residual_first
                accumulate = int(nxt_on) ^ int(addkind == "dense")
                key = ("bn_act_bwd_apply" if proto == "rows" else "bn_fin_bwd_apply") + ("_next" if nxt_on else "") + \
                      ("_s2" if addkind == "s2" else "")
                add = {"none": None, "dense": d["add"], "s2": compact}[addkind]
                dense = {"none": None, "dense": d["add"], "s2": scatter_s2(compact, N, H, W)}[addkind]
                pre = None if lat else (d["pre"] if accumulate else None)
                br = bwd_reference(d["dy"], x, sc, sh, alpha, mean, inv, res_arg, dt, 1, sums=sums, dsums=dsums,
                                   add=dense, pre=pre)
                rep.ambiguous += br["ambiguous"]
                if lat:
                    grads, accumulate = [torch.zeros(C, device=x.device) for _ in range(3)], 0
                else:
                    grads = [d["pre"][i].clone() for i in range(3)]
                if alpha is None and proto == "rows":
                    grads[2] = None
                nxt = (d["nx"], d["nmean"], d["ninvstd"]) if nxt_on else None
                dx, dres, em = be.bwd_apply(d["dy"], x, sc, sh, alpha, mean, inv, pieces, grads, accumulate, add=add,
                                            add_hw=(H, W) if addkind == "s2" else None, nxt=nxt, proto=proto,
                                            res=res_arg)
                if lat:
                    rep.exact(key, "dx", dx, br["dx"], case)
                    for i, nm in enumerate(("dbeta", "dgamma", "dalpha")):
                        if grads[i] is not None:
                            rep.exact(key, nm, grads[i], br[nm], case)
                    if res_arg is not None:
                        rep.exact(key, "dres", dres, br["dres"], case)
                else:
                    rep.check(key, "dx", dx, br["dx"], br["dx_budget"], case)
                    for i, nm in enumerate(("dbeta", "dgamma", "dalpha")):
                        if grads[i] is not None:
                            rep.check(key, nm, grads[i], br[nm], br[nm + "_budget"], case)
                    if res_arg is not None:
                        rep.check(key, "dres", dres, br["dres"], br["dres_budget"], case)
                if nxt_on:
                    er = emitted_reference(dx, M, C, g_ew, d["nx"], d["nmean"], d["ninvstd"], acc=proto == "acc")
                    if lat:
                        rep.exact(key, "next sum", em[0], er["q0"], case)
                        rep.exact(key, "next sum*xhat", em[1], er["q1"], case)
                    else:
                        rep.check(key, "next sum", em[0], er["q0"], er["q0_budget"], case)
                        rep.check(key, "next sum*xhat", em[1], er["q1"], er["q1_budget"], case)


def check_lattice_fwd(be, case, rep, device="cpu"):
    """msml_bn_act_fwd[_stats] on operands whose every intermediate is exact in f32 and bf16: torch.equal."""
    d = draw(case, device)
    x, M, C, dt = d["x"], case.M, case.C, DT[case.dtype]
    rf = int(case.res_first and case.residual)
    ref = fwd_reference(x, d["scale"], d["shift"], d["alpha"], d["res"], rf, dt)
    zero = float((ref["z"] == 0).double().mean()) if ref["z"] is not None else None
    y, em = be.act_fwd(x, d["scale"], d["shift"], d["alpha"], d["res"], rf, emit=True, proto="rows")
    rep.exact("bn_act_fwd_stats", "lattice y", y, ref["y"], case)
    rep.exact("bn_act_fwd_stats", "lattice sum", em[0], ref["y"].sum(0), case)
    rep.exact("bn_act_fwd_stats", "lattice sumsq", em[1], (ref["y"] * ref["y"]).sum(0), case)
    return zero


# ------------------------------------------------------------------------------------------ stride-2 pixel decode
S2_MOST_FIXUPS = (2, 3)      # what s2_decode_scan finds over S2_SHAPES (asserted by tests/test_bn_cpu.py); the GPU test uses it
S2_SHAPES = ((1, 1), (2, 3), (7, 7), (14, 14), (113, 113), (1831, 1831), (3, 5592405))


def s2_decode_scan(H, W, limit=1 << 24):
    """The float-reciprocal + one-fix-up decode of k_bn_bwd_apply<ADD_S2> (pix -> n, y, x) in numpy float32 for every
    pix < limit.  Returns (decode equals integer divmod everywhere, number of fix-ups taken)."""
    import numpy as np
    pix = np.arange(limit, dtype=np.int64)
    rcpW, rcpH = np.float32(1.0) / np.float32(W), np.float32(1.0) / np.float32(H)
    row = (pix.astype(np.float32) * rcpW).astype(np.int64)            # (int): truncation, operands >= 0
    xx = pix - row * W
    lo, hi = xx < 0, xx >= W
    row = row - lo + hi
    xx = xx + lo * W - hi * W
    nn = (row.astype(np.float32) * rcpH).astype(np.int64)
    yy = row - nn * H
    lo2, hi2 = yy < 0, yy >= H
    nn = nn - lo2 + hi2
    yy = yy + lo2 * H - hi2 * H
    r_ref, x_ref = np.divmod(pix, W)
    n_ref, y_ref = np.divmod(r_ref, H)
    ok = bool((xx == x_ref).all() and (yy == y_ref).all() and (nn == n_ref).all())
    return ok, int(lo.sum() + hi.sum() + lo2.sum() + hi2.sum())
