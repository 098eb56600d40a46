"""CPU side of the BatchNorm kernel-family tests (tests/bn_cases.py): the f64 reference is checked against torch's own
modules before anything is checked against it, the torch restatement of the kernels' arithmetic passes every derived
budget (the budgets are satisfiable), eleven single-fault mutants of it each fail one (the budgets have power), and the
float-reciprocal pixel decode of the stride-2 scatter equals integer divmod below 2^24 pixels."""
import torch

from tests import bn_cases as B

CPU_CAP = 1 << 24            # M * C of the cases the restatement runs on the CPU
CPU_CAP_REDUCE = 1 << 26     # reduction-only entry points: with 16 pixels per thread the 1024-row cap starts at 2^25


def _close(a, b, what):
    """f64 against f64, other summation order: 2^-53 x (terms of the longest sum, < 2^12 here) x 8, relative to the
    largest magnitude of the tensor."""
    tol = 8 * 4096 * B.U64 * max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)


def test_reference_equals_torch_modules():
    torch.manual_seed(3)
    N, C, H, W = 3, 16, 5, 7
    for with_alpha, with_res, res_first, affine in B._VARIANTS:
        bn = torch.nn.BatchNorm2d(C, eps=B.f32(B.EPS), momentum=0.1, affine=affine).double()
        pr = torch.nn.PReLU(C).double()
        with torch.no_grad():
            if affine:
                bn.weight.copy_(1.0 + 0.5 * torch.randn(C))
                bn.bias.copy_(0.5 * torch.randn(C))
            pr.weight.copy_(0.25 + 0.2 * torch.randn(C))
            bn.running_mean.copy_(torch.randn(C))
            bn.running_var.copy_(1.0 + torch.rand(C))
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
        for step in range(2):
            x = (torch.randn(N, C, H, W, dtype=torch.float64) * 2 + 1).requires_grad_(True)
            x.data[0, 0, 0, 0] = 0.0
            r = torch.randn(N, C, H, W, dtype=torch.float64).requires_grad_(True)
            dy = torch.randn(N, C, H, W, dtype=torch.float64)
            z = bn(x)
            if with_res and res_first:
                z = z + r
            if with_alpha:
                z = pr(z)
            if with_res and not res_first:
                z = z + r
            for p in list(bn.parameters()) + list(pr.parameters()):
                p.grad = None
            z.backward(dy)
            gamma, beta = (bn.weight.detach(), bn.bias.detach()) if affine else (None, None)
            alpha = pr.weight.detach() if with_alpha else None
            ref = B.autograd_reference(flat(x.detach()), gamma, beta, alpha, flat(r.detach()) if with_res else None, res_first,
                                       flat(dy), rm0, rv0, 0.1, B.f32(B.EPS))
            _close(ref["y"], flat(z.detach()), "y")
            _close(ref["dx"], flat(x.grad), "dx")
            _close(ref["rmean"], bn.running_mean, "running_mean after step %d" % step)
            _close(ref["rvar"], bn.running_var, "running_var after step %d" % step)
            if with_res:
                _close(ref["dres"], flat(r.grad), "dres")
            if affine:
                _close(ref["dgamma"], bn.weight.grad, "dgamma")
                _close(ref["dbeta"], bn.bias.grad, "dbeta")
            if with_alpha:
                _close(ref["dalpha"], pr.weight.grad, "dalpha")
            # the formulas the entry points are compared with, fed the exact f64 coefficients, equal autograd
            st = B.stats_reference(flat(x.detach()))
            cf = B.coef_reference(st, gamma, beta, rm0, rv0, 0.1, B.f32(B.EPS))
            _close(cf["rmean"], ref["rmean"], "formula rmean")
            _close(cf["rvar"], ref["rvar"], "formula rvar")
            fr = B.fwd_reference(flat(x.detach()), cf["scale"], cf["shift"], alpha, flat(r.detach()) if with_res else None,
                                 int(res_first), torch.float32)
            _close(fr["y"], ref["y"], "formula y")
            br = B.bwd_reference(flat(dy), flat(x.detach()), cf["scale"], cf["shift"], alpha, cf["mean"], cf["invstd"],
                                 flat(r.detach()) if (with_res and res_first and with_alpha) else None, torch.float32, 1)
            _close(br["dx"], ref["dx"], "formula dx")
            if affine:
                _close(br["dgamma"], ref["dgamma"], "formula dgamma")
                _close(br["dbeta"], ref["dbeta"], "formula dbeta")
            if with_alpha:
                _close(br["dalpha"], ref["dalpha"], "formula dalpha")
            if with_res:
                _close(br["dres"] if res_first and with_alpha else flat(dy), ref["dres"], "formula dres")
            rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    # count == 1: the biased variance goes into running_var (k_bn_finalize); torch refuses a single value per channel
    st = B.stats_reference(torch.tensor([[2.0, -1.0]], dtype=torch.float64))
    cf = B.coef_reference(st, None, None, torch.zeros(2), torch.ones(2), 0.1, 1e-5)
    assert torch.equal(cf["rvar"], torch.full((2,), 0.9, dtype=torch.float64))


def _run(be, case, rep):
    if case.kind == "lattice":
        zero = B.check_lattice_fwd(be, case, rep)
        B.check_rows_case(be, case, rep)
        return zero
    if case.name.startswith("reduce"):
        B.check_reduce_case(be, case, rep)
    elif case.rows is not None:
        B.check_rows_case(be, case, rep)
    else:
        B.check_apply_case(be, case, rep)


def _cpu_cases():
    run, skipped = [], []
    for group in ("reduce", "apply", "rows", "lattice", "big"):
        for c in B.case_table(group):
            cap = CPU_CAP_REDUCE if group == "reduce" else CPU_CAP
            (run if c.M * c.C <= cap else skipped).append(c)
    return run, skipped


def test_restatement_passes_every_budget():
    run, skipped = _cpu_cases()
    print("\nskipped on the CPU (M * C above the cap):", ", ".join(c.name for c in skipped))
    # a category is a row of the case table's M / data-kind list; the slab boundaries above 512 rows fit under the cap
    # only through the reduction-only entry points (same slab_reduce)
    tags_run = {c.tag for c in run}
    for c in skipped:
        assert c.tag in tags_run, "a whole category is skipped on the CPU: %s" % (c.tag,)
    for c in run + skipped:
        assert B.slab_geometry_ok(c), "the case no longer sits on the boundary its tag names: %s" % (c.name,)
    rep = B.Report()
    zeros = []
    for c in run:
        z = _run(B.Restatement(), c, rep)
        if z is not None:
            zeros.append(z)
    print(rep.table())
    print("elements within their own z budget of the PReLU kink (either branch accepted):", rep.ambiguous)
    print("lattice: share of elements with z == 0: %.3f .. %.3f" % (min(zeros), max(zeros)))
    assert min(zeros) > 0.02, "the lattice does not visit z == 0"
    assert not rep.failures, rep.failures[:10]


def _power_cases(mutant):
    """Where a mutant can differ, cheapest first."""
    ap = [c for c in B.case_table("apply") if c.M * c.C <= 1 << 20]
    if mutant in ("count_plus_1", "biased_running_var"):
        return [c for c in B.case_table("reduce") if c.M <= 7 and c.M > 1]
    if mutant == "z_lt_0":
        return [c for c in B.case_table("lattice") if c.alpha and c.M <= 4096]
    if mutant == "coef_next_chunk_2nd_trip":
        return [c for c in B.case_table("big") if c.M * c.C <= CPU_CAP]
    if mutant == "add_on_odd_pixels":
        return [c for c in B.case_table("rows") if c.rows == 32]
    if mutant == "stats_unrounded":
        return [c for c in ap if c.dtype == "bf16" and c.C == 2048]
    if mutant == "res_first_ignored_bwd":
        return [c for c in ap if c.res_first and c.alpha and c.M > 7]
    if mutant == "xhat_with_scale":
        return [c for c in ap if c.affine and c.M > 7]
    return [c for c in ap if c.alpha and c.M > 7]


def test_every_mutant_fails_a_budget():
    print()
    missed = []
    for mutant in B.MUTANTS:
        caught = None
        for c in _power_cases(mutant):
            rep = B.Report()
            _run(B.Restatement(mutant), c, rep)
            if rep.failures:
                key, what, name, r = rep.failures[0]
                caught = "%s: %s %s at %.3g x budget" % (name, key, what, r)
                break
        print("mutant %-26s caught by %s" % (mutant, caught))
        if caught is None:
            missed.append(mutant)
    assert len(B.MUTANTS) == 11 and not missed, missed


def test_stride2_pixel_decode_equals_divmod_below_2_24():
    print()
    best = None
    for H, W in B.S2_SHAPES:
        ok, fix = B.s2_decode_scan(H, W)
        print("H=%d W=%d: decode == divmod for every pix < 2^24: %s, fix-ups taken %d" % (H, W, ok, fix))
        assert ok, (H, W)
        if best is None or fix > best[0]:
            best = (fix, H, W)
    print("most fix-ups at (H, W) =", best[1:])
    assert best[1:] == B.S2_MOST_FIXUPS
