"""Shared by tests/test_bn_eval_cpu.py and tests/test_gpu_bn_eval_bwd.py: the case table of msml_bn_eval_act_bwd (the
backward through an eval-mode / frozen BatchNorm, msml_amd/csrc/bn.hip), its float64 reference with derived error budgets,
a torch restatement of the kernel's f32 arithmetic with single-fault mutants, and the check that compares ANY
implementation -- the restatement on the CPU, the library on the GPU -- with the reference.

Reference (eval mode: scale = gamma * invstd and shift = beta - running_mean * scale are CONSTANTS of the graph):
  z = x * scale + shift [+ r],  g = dy * (z <= 0 ? alpha : 1)   (g = dy without PReLU)
  dx = scale * g,  dres = g,  dbeta = sum g,  dgamma = sum g * (x - running_mean) * invstd,  dalpha = sum dy * min(z, 0)
tests/test_bn_eval_cpu.py shows that these formulas equal torch autograd of F.batch_norm(training=False) + F.prelu +
residual in f64 (bn_cases.autograd_reference) before anything is compared with them.

Budgets, derived as bn_cases.bwd_reference derives them (never fitted to an output): k * u32 * (magnitudes of the terms)
with k counted from the expression next to it, u_store(dtype) * |ref| for a stored tensor, chain * u32 * sum |term| for a
sum, chain = grid-stride trips of a thread + the 256 / (C/8) lanes of the LDS fold (bn_cases.grid_chain with the library's
own row count), the f64 fold of the rows at (rows + 40) * u64, SAFETY = 2 on everything (bn_cases.Report.check).  An element
whose |z| is within the budget of z but not exactly 0 may take either PReLU branch; z == 0 exactly is never excused.
"""
import torch

from tests import bn_cases as B
from tests.bn_cases import SAFETY, U32, U64, u_store, w

MS = (1, 2, 255, 257, 4099)
CS = (8, 64, 512, 2048)
SUMS = ("none", "all", "beta")                  # which of (dbeta, dgamma, dalpha) the caller asks for
MUTANTS = ("training_formula", "z_lt_0", "res_first_ignored", "xhat_batch_mean", "dgamma_no_invstd", "accumulate_overwrites")


def eval_rows(M, C):
    """msml_bn_eval_act_bwd_rows (asked from the library: the grid rule under test is the library's, not a copy)."""
    from msml_amd import _lib
    return _lib.value("msml_bn_eval_act_bwd_rows", M, C)


def case_table(group="normal", Cs=CS, dtypes=("f32", "bf16"), Ms=MS, variants="all"):
    """variants: 'all' = every variant of bn_cases._VARIANTS at every (C, M, dtype) (the GPU test); 'cycle' = one variant
    per (C, M, dtype), stepping through them so that each dtype and each C meets all eight (the CPU restatement, whose
    torch loops over lanes and trips cost seconds per case at the large shapes)."""
    cases = []
    if group == "normal":
        k = 0
        for C in CS:
            for M in MS:
                for i, dt in enumerate(("f32", "bf16")):
                    pick = B._VARIANTS if variants == "all" else [B._VARIANTS[(k + 3 * i) % len(B._VARIANTS)]]
                    k += 1 if i else 0
                    if C not in Cs or M not in Ms or dt not in dtypes:
                        continue
                    for v in pick:
                        cases.append(B.Case("eval-C%d-M%d-%s-a%dr%df%dg%d" % (C, M, dt, *map(int, v)), M, C, dt, *v, "normal",
                                            None, "eval"))
    elif group == "lattice":
        for C, M in ((8, 64), (64, 4099), (256, 1025), (2048, 16)):
            if C not in Cs:
                continue
            for dt in dtypes:
                for v in B._VARIANTS[:4]:
                    cases.append(B.Case("eval-lattice-C%d-M%d-%s-a%dr%df%d" % (C, M, dt, *map(int, v[:3])), M, C, dt, *v,
                                        "lattice", None, "lattice"))
    return cases


def eval_coefficients(d):
    """(scale, shift, mean, invstd) in f32 as msml_bn_finalize's eval branch hands them over: inputs of the backward."""
    if "scale" in d:                               # lattice draw: given
        return d["scale"], d["shift"], d["mean"], d["invstd"]
    rm, rv = d["rmean0"], d["rvar0"]
    inv = (1.0 / torch.sqrt(rv.double() + B.f32(B.EPS))).float()
    g = d["gamma"] if d["gamma"] is not None else torch.ones_like(inv)
    b = d["beta"] if d["beta"] is not None else torch.zeros_like(inv)
    return g * inv, b - rm * g * inv, rm, inv


# -------------------------------------------------------------------------------------------------- f64 reference
def eval_reference(dy, x, scale, shift, alpha, mean, invstd, res_first_res, dtype, chain=1, rows=1, pre=None):
    """The eval-mode backward in f64 on exactly these operands, and its budgets."""
    dy, x, sc, mu, inv = w(dy), w(x), w(scale), w(mean), w(invstd)
    gg, egg = dy, torch.zeros_like(dy)
    amb = 0
    neg = ambig = None
    if alpha is not None:
        f = B.fwd_reference(x, scale, shift, None, res_first_res, True, dtype)
        z, ez, a = f["y"], f["ez"], w(alpha)
        neg = z <= 0
        ambig = (z != 0) & (z.abs() <= SAFETY * ez)                      # may take either PReLU branch
        amb = int(ambig.sum())
        gg = torch.where(neg, dy * a, dy)
        egg = U32 * gg.abs() * neg + ambig * (dy * (1.0 - a)).abs()      # dy * a: 1 op
        zneg = torch.where(neg, z, torch.zeros_like(z))
    dx = sc * gg
    edx = sc.abs() * egg + U32 * dx.abs()                                # sc * g: 1 op
    out = {"dx": dx, "dx_budget": edx + u_store(dtype) * dx.abs(), "dres": gg,
           "dres_budget": egg + u_store(dtype) * gg.abs(), "ambiguous": amb}
    xh = (x - mu) * inv
    exh = 2 * U32 * xh.abs()                                             # (x - mu) * is: 2 ops
    fold = (rows + 40) * U64                                             # f64 fold of the partial rows
    s0, s1 = gg.sum(0), (gg * xh).sum(0)
    d0 = (chain * U32 + fold) * gg.abs().sum(0) + egg.sum(0)             # q0 += g
    d1 = ((chain + 1) * U32 + fold) * (gg * xh).abs().sum(0) + (egg * xh.abs() + gg.abs() * exh).sum(0)   # q1 += g * xh
    if alpha is not None:
        s2 = (dy * zneg).sum(0)                                          # q2 += dy * z where z <= 0
        d2 = ((chain + 1) * U32 + fold) * (dy * zneg).abs().sum(0) + (dy.abs() * ez * (neg | ambig)).sum(0)
    else:
        s2, d2 = torch.zeros_like(s0), torch.zeros_like(s0)
    for i, (nm, s, d) in enumerate((("dbeta", s0, d0), ("dgamma", s1, d1), ("dalpha", s2, d2))):
        p = w(pre[i]) if pre is not None else 0.0
        out[nm] = s + p
        out[nm + "_budget"] = d + U32 * s.abs() + (U32 * (s + p).abs() if pre is not None else 0.0)   # (float)s, prev + s
    return out


# ------------------------------------------------------------------------- torch restatement of the kernel's arithmetic
class Restatement:
    """msml_bn_eval_act_bwd in torch: f32 operations in the kernel's order (grid-stride trips of a thread, LDS fold over
    the lanes of a workgroup, f64 fold of the rows), storage rounding where it stores.  `mutant` plants one fault."""
    name = "restatement"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mut = mutant

    # grads = [dbeta, dgamma, dalpha] (None: not asked for), updated in place
    def eval_bwd(self, dy, x, scale, shift, alpha, mean, invstd, res, grads, accumulate):
        M, C = x.shape
        gg = dy.float()
        q2 = torch.zeros_like(gg)
        if alpha is not None:
            z = x.float() * scale + shift
            if res is not None and self.mut != "res_first_ignored":
                z = z + res.float()
            neg = (z < 0) if self.mut == "z_lt_0" else (z <= 0)
            q2 = torch.where(neg, gg * z, q2)
            gg = torch.where(neg, gg * alpha, gg)
        mu = x.float().mean(0) if self.mut == "xhat_batch_mean" else mean
        xh = (x.float() - mu) if self.mut == "dgamma_no_invstd" else (x.float() - mu) * invstd
        v = scale * gg
        if self.mut == "training_formula":
            v = scale * (gg - gg.mean(0) - xh * (gg * xh).mean(0))
        dx, dres = v.to(x.dtype), (gg.to(x.dtype) if res is not None else None)
        if any(g is not None for g in grads):
            idx = B._grid_idx(M, C, eval_rows(M, C))
            acc = accumulate and self.mut != "accumulate_overwrites"
            for gr, t in zip(grads, (gg, gg * xh, q2)):
                if gr is not None:
                    s = B._two_level(t, idx).double().sum(0)
                    gr.copy_((gr if acc else torch.zeros_like(gr)) + s.float())
        return dx, dres


# ------------------------------------------------------------------------------------- the check, for any backend
def _ask(sums, pre, has_alpha):
    """[dbeta, dgamma, dalpha] buffers holding `pre` for the outputs `sums` asks for (dalpha only with a PReLU)."""
    if sums == "none":
        return [None, None, None]
    if sums == "beta":
        return [pre[0].clone(), None, None]
    return [pre[0].clone(), pre[1].clone(), pre[2].clone() if has_alpha else None]


def check_eval_case(be, case, rep, device="cpu", sums_modes=SUMS, key="bn_eval_act_bwd"):
    d = B.draw(case, device)
    x, M, C, dt = d["x"], case.M, case.C, B.DT[case.dtype]
    sc, sh, mean, inv = eval_coefficients(d)
    alpha = d["alpha"]
    resb = d["res"] if (case.res_first and case.residual) else None
    lattice = case.kind == "lattice"
    if lattice:
        g = torch.Generator().manual_seed(C * 131 + M)
        pre_t = torch.randint(-4, 5, (3, C), generator=g).float().to(device)
    else:
        pre_t = d["pre"]
    rows = eval_rows(M, C)
    chain = B.grid_chain(M, C, rows)
    refs = {acc: eval_reference(d["dy"], x, sc, sh, alpha, mean, inv, resb, dt, chain, rows, pre=pre_t if acc else None)
            for acc in (0, 1)}
    rep.ambiguous += refs[0]["ambiguous"]
    pad = slice(C - 8, C) if case.kind == "padzero" else None
    for sums in sums_modes:
        for accumulate in (0, 1):
            br = refs[accumulate]
            grads = _ask(sums, pre_t, alpha is not None)
            dx, dres = be.eval_bwd(d["dy"], x, sc, sh, alpha, mean, inv, resb, grads, accumulate)
            tag = " sums=%s acc=%d" % (sums, accumulate)
            if lattice:
                rep.exact(key, "dx" + tag, dx, br["dx"].to(dt), case)
                if resb is not None:
                    rep.exact(key, "dres" + tag, dres, br["dres"].to(dt), case)
            else:
                rep.check(key, "dx" + tag, dx, br["dx"], br["dx_budget"], case)
                if resb is not None:
                    rep.check(key, "dres" + tag, dres, br["dres"], br["dres_budget"], case)
            if resb is None:
                assert dres is None
            for i, nm in enumerate(("dbeta", "dgamma", "dalpha")):
                if grads[i] is None:
                    continue
                if lattice:
                    rep.exact(key, nm + tag, grads[i], br[nm].float(), case)
                else:
                    rep.check(key, nm + tag, grads[i], br[nm], br[nm + "_budget"], case)
            if pad is not None:
                rep.exact(key, "pad channels of dx", dx[:, pad], torch.zeros(M, 8, device=dx.device), case)
