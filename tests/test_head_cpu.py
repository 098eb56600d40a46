"""CPU side of the head / PartialFC / optimizer kernel tests (tests/head_cases.py): the f64 references are checked against
torch's own functions and against the module-level goldens of g5_heads.npz before anything is checked against them, the
torch restatement of the kernels' arithmetic passes every derived budget (the budgets are satisfiable), and every
single-fault mutant of it fails the check named for it (the budgets have power)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.inputs import head_inputs
from tests import head_cases as H
from tests.helpers import load, rel_err

CPU_CAP = 1 << 20            # N * ld of the margin / PartialFC cases the restatement runs on the CPU
CPU_CAP_GEMM = 1 << 22       # M * K


def _close(a, b, what):
    """f64 against f64, other operation order: 2^-53 x (terms of the longest sum, < 2^12 here) x 8, relative to the
    largest magnitude of the tensor."""
    tol = 8 * 4096 * H.U64 * max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)


def test_libm_constants_cover_this_machine():
    got = H.measure_libm()
    print()
    for fn in sorted(got):
        print("%-5s measured %.3f u32, recorded %.3f, budget %.3f" % (fn, got[fn], H.LIBM_MEASURED[fn], H.L(fn)))
        assert got[fn] <= H.L(fn), fn


def test_rownorm_reference_equals_torch():
    torch.manual_seed(1)
    w = (0.3 * torch.randn(7, 40, dtype=torch.float64)).requires_grad_(True)
    dy = torch.randn(7, 40, dtype=torch.float64)
    y = F.normalize(w)
    y.backward(dy)
    ry, _, bwd = H.rownorm_reference_for_autograd(w.detach())
    _close(ry, y.detach(), "y")
    _close(bwd(dy), w.grad, "dw")


def test_margin_reference_equals_g5_heads():
    """The margin expression + autograd in f64, through normalize / linear, against the module-level outputs and
    gradients the golden file pins (arc0, arc1, cos0, cos1)."""
    g = load("g5_heads.npz")
    emb, w, label = head_inputs()
    for name, kind, prm in (("arc0", H.ARC, (64.0, 0.48, 0.0, 0.0)), ("arc1", H.ARC, (64.0, 0.5, 1.2, 0.1)),
                            ("cos0", H.COS, (64.0, 0.4, 0.0, 0.0)), ("cos1", H.COS, (64.0, 0.4, 1.2, 0.1))):
        e = emb.double().requires_grad_(True)
        ww = w.double().requires_grad_(True)
        cos = F.linear(F.normalize(e), F.normalize(ww))
        r = H.margin_reference(cos.detach(), label, 8, kind, *prm)
        assert rel_err(r["logits"].numpy(), g[name + "_out"]) < 1e-5, name
        # the backward factor: dcos = dlogit * d, then through cos by autograd
        dout = torch.linspace(-1, 1, cos.numel()).reshape(cos.shape).double()
        cos.backward(dout * r["d"])
        assert rel_err(e.grad.numpy(), g[name + "_demb"]) < 1e-5, name
        assert rel_err(ww.grad.numpy(), g[name + "_dw"]) < 1e-5, name
        # and the same factor from the expression differentiated as a whole matrix
        c2 = cos.detach().clone().requires_grad_(True)
        lg = 64.0 * c2
        rows = (label >= 0).nonzero().flatten()
        lg = lg.index_put((rows, label[rows]), H.margin_expr(c2[rows, label[rows]], kind, *prm))
        lg.backward(dout)
        _close(c2.grad, dout * r["d"], name + " factor")


def test_sgd_reference_equals_torch_optim():
    torch.manual_seed(2)
    for mu, wd in ((0.9, 5e-4), (0.0, 5e-4), (0.9, 0.0)):
        p = torch.nn.Parameter(torch.randn(50, dtype=torch.float64))
        opt = torch.optim.SGD([p], lr=0.1, momentum=mu, weight_decay=wd)
        wt, buf = p.detach().clone(), torch.zeros(50, dtype=torch.float64)
        for step in range(3):
            grad = torch.randn(50, dtype=torch.float64)
            p.grad = grad.clone()
            opt.step()
            wt, buf = H.sgd_reference(wt, grad, buf, 0.1, mu, wd, step == 0, 1.0)
            _close(wt, p.detach(), "w after step %d" % step)


def test_norm_reference_equals_clip_grad_norm():
    torch.manual_seed(3)
    for max_norm in (0.5, 50.0):
        p = torch.nn.Parameter(torch.zeros(300, dtype=torch.float64))
        p.grad = torch.randn(300, dtype=torch.float64)
        g0 = p.grad.clone()
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        norm, coef = H.norm_reference(g0, max_norm, 1.0)
        _close(norm, total, "norm")
        _close(g0 * coef, p.grad, "clipped gradient")
        # a sum over W ranks scaled by 1 / W is the same gradient
        n4, c4 = H.norm_reference(g0 * 4.0, max_norm, 0.25)
        _close(n4, total, "scaled norm")
        _close(g0 * 4.0 * c4, p.grad, "scaled clipped gradient")


def test_pfc_reference_equals_softmax_cross_entropy():
    """p = exp(l - max) / sum is softmax, and (p - y) / n is the gradient of the label-smoothed cross entropy the PartialFC
    head documents (0.9 at the target, 0.1 / (C - 1) elsewhere)."""
    torch.manual_seed(4)
    N, C = 5, 11
    cos = (torch.rand(N, C, dtype=torch.float64) * 1.6 - 0.8)
    lab = torch.randint(0, C, (N,))
    s, m, a, k = H.margin_params(H.ARC, H.AKS[1])
    r = H.pfc_reference(cos, lab, C, H.ARC, s, m, a, k)
    lg = r["logits"].clone().requires_grad_(True)
    y = torch.full((N, C), 0.1 / (C - 1), dtype=torch.float64)
    y[torch.arange(N), lab] = 0.9
    loss = -(y * torch.log_softmax(lg, 1)).sum() / N
    loss.backward()
    p = torch.exp(r["logits"] - r["max"][:, None]) / r["sum"][:, None]
    _close((p - y) / N, lg.grad, "dlogit")
    _close(r["lse"], torch.logsumexp(r["logits"], 1), "lse")


def _run_all(make, rep, cap=True):
    planted = excused = 0
    count = {"target_is_max": 0, "target_not_max": 0}
    for c in H.rownorm_cases():
        H.check_rownorm_case(make(), c, rep)
    for c in H.margin_cases():
        if c.N * c.ld > CPU_CAP:
            continue
        p, e = H.check_margin_case(make(), c, rep)
        planted, excused = planted + p, excused + e
        if c.C > 1:
            p, e = H.check_pfc_grad_case(make(), c, rep)
            planted, excused = planted + p, excused + e
    for c in H.rowstats_cases():
        if c.N * c.ld <= CPU_CAP:
            H.check_rowstats_case(make(), c, rep, count=count)
    for R, C in H.TRANSPOSE_SHAPES:
        for dt in ("f32", "bf16"):
            for ld_d in sorted({R, H.kpad(R)}):
                if R * C <= CPU_CAP:
                    H.check_transpose(make(), R, C, C + 3, ld_d, dt, rep)
    for M, K in H.GEMM_SHAPES:
        if M * K <= CPU_CAP_GEMM:
            H.check_gemm(make(), M, K, rep)
    for n in H.SGD_NS:
        for v in H.SGD_VARIANTS:
            H.check_sgd(make(), n, v, rep)
    for n in H.NORM_NS:
        for above in (False, True):
            for scale in (1.0, 0.25):
                H.check_norm_clip(make(), n, above, scale, rep)
    return planted, excused, count


def test_restatement_passes_every_budget():
    rep = H.Report()
    planted, excused, count = _run_all(H.Restatement, rep)
    print("\n" + rep.table())
    print("planted targets with |c| == 1: %d, backward elements excused: %d; rows whose target is / is not the row max: %d / %d"
          % (planted, excused, count["target_is_max"], count["target_not_max"]))
    assert planted > 0 and excused == planted
    assert count["target_is_max"] > 0 and count["target_not_max"] > 0
    assert not rep.failures, rep.failures[:10]


def _power_runs(mutant):
    """Calls that can tell a mutant from the kernel, cheapest first: (function, arguments after the backend)."""
    mc = [c for c in H.margin_cases() if c.N == 9 and c.C in (2, 257) and c.p.get("labels") is None]
    if mutant in ("smooth_denominator_C", "smooth_on_label_minus_1", "ptarget_unwritten_minus_1"):
        return [(H.check_pfc_grad_case, (c,)) for c in mc]
    if mutant == "rescale_dropped":
        return [(H.check_rowstats_case, (c,)) for c in H.rowstats_cases() if c.C == 16385 and c.spread == "wide"]
    if mutant == "pad_in_rowstats":
        return [(H.check_rowstats_case, (c,)) for c in H.rowstats_cases() if c.C == 257 and c.ld == H.kpad(257)]
    if mutant == "ldo_not_zeroed":
        return [(H.check_margin_case, (c,)) for c in mc if c.ldo > c.C]
    if mutant == "minus_1_hits_last_column":
        return [(H.check_margin_case, (c,)) for c in mc]
    if mutant == "k_sign_flipped":
        return [(H.check_margin_case, (c,)) for c in mc if c.kind_ == H.ARC and c.ak == H.AKS[1]]
    if mutant == "sgd_first_ignored":
        return [(H.check_sgd, (1023, H.SGD_VARIANTS[0]))]
    if mutant == "sgd_tail_skipped":
        return [(H.check_sgd, (5, H.SGD_VARIANTS[1]))]
    if mutant == "sumsq_tail_skipped":
        return [(H.check_norm_clip, (5, True, 1.0))]
    if mutant == "clip_not_capped":
        return [(H.check_norm_clip, (1024, False, 1.0))]
    if mutant == "scale_not_on_coef":
        return [(H.check_norm_clip, (1024, True, 0.25))]
    raise KeyError(mutant)


def test_every_mutant_fails_the_check_named_for_it():
    print()
    bad = []
    for mutant, (key, what) in H.MUTANTS.items():
        caught = None
        for fn, args in _power_runs(mutant):
            rep = H.Report()
            fn(H.Restatement(mutant), *args, rep)
            if rep.failures:
                k, w, name, r = rep.failures[0]
                caught = (k, w, "%s: %s %s at %.3g x budget" % (name, k, w, r))
                break
        print("mutant %-28s caught by %s" % (mutant, caught and caught[2]))
        if caught is None or not (caught[0].startswith(key) and caught[1].startswith(what)):
            bad.append((mutant, caught))
    assert len(H.MUTANTS) >= 12 and not bad, bad


def test_case_tables_bracket_the_grid_caps():
    """The shapes the tables promise: below, at and above the 64 x 256 and 128 x 256 column caps, one and two trips of the
    1024-thread row kernel, the capped SGD and sum-of-squares grids."""
    cs = {c.C for c in H.margin_cases()}
    for cap in (64 * 256, 128 * 256):
        assert cap in cs and cap + 1 in cs
    assert {4096, 4097, 3, 4, 5} <= {c.C for c in H.rowstats_cases()} and any(c.C < 64 for c in H.rowstats_cases())
    assert H.sgd_grid(max(H.SGD_NS)) == 4096 and max(H.SGD_NS) // 4 > 2 * 4096 * 256 and max(H.SGD_NS) % 4
    assert 1024 * 4096 + 3 in H.SGD_NS and H.sgd_grid(1024 * 4096 + 3) == 4096
    assert H.sumsq_rows(262144 - 1) == 1024 and H.sumsq_rows(1024) == 4
    n = max(H.NORM_NS)
    assert n // 4 > 4 * 1024 * 256 and (n // 4) % (1024 * 256) and n % 4       # unrolled trips + remainder loop + tail
    assert H.rownorm_v8(512, 512) and H.rownorm_v8(1024, 1024) and not H.rownorm_v8(1536, 1536) and not H.rownorm_v8(512, 512, False)
    assert np.isclose(np.sqrt(1023.0 / 1025.0), 0.99902391) and H.CMAX <= np.sqrt(1023.0 / 1025.0)
