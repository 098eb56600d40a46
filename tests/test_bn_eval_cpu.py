"""tests/bn_eval_cases.py checked without a GPU: the eval-mode backward formulas equal torch autograd in f64, the torch
restatement of msml_bn_eval_act_bwd stays inside the derived budgets over the whole case table (and is exact on the
lattice), and every planted fault (bn_eval_cases.MUTANTS) is rejected by those same checks."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_cases as B
from tests import bn_eval_cases as E


def test_formulas_equal_autograd_f64():
    """eval_reference on f64 coefficients == autograd of F.batch_norm(training=False) + F.prelu + residual in f64."""
    eps, mom = B.f32(B.EPS), B.f32(0.1)
    n = 0
    for case in E.case_table("normal", Cs=(8, 64), dtypes=("f32",)):
        if not case.affine:
            continue
        d = B.draw(case)
        ag = B.autograd_reference(d["x"], d["gamma"], d["beta"], d["alpha"], d["res"], case.res_first, d["dy"], d["rmean0"],
                                  d["rvar0"], mom, eps, training=False)
        assert torch.equal(ag["rmean"], d["rmean0"].double()) and torch.equal(ag["rvar"], d["rvar0"].double())
        inv = 1.0 / torch.sqrt(d["rvar0"].double() + eps)
        sc = d["gamma"].double() * inv
        sh = d["beta"].double() - d["rmean0"].double() * sc
        resb = d["res"] if (case.res_first and case.residual) else None
        ref = E.eval_reference(d["dy"], d["x"], sc, sh, d["alpha"], d["rmean0"], inv, resb, torch.float32)

        def close(a, b):
            return bool(((a - b).abs() <= 1e-12 * (1.0 + b.abs())).all())
        assert close(ref["dx"], ag["dx"]) and close(ref["dbeta"], ag["dbeta"]), case.name
        # (sums over M pixels: relative to the sum of magnitudes)
        assert bool(((ref["dgamma"] - ag["dgamma"]).abs() <= 1e-11 * (1.0 + d["dy"].double().abs().sum(0) * 10)).all()), case.name
        if d["alpha"] is not None:
            assert close(ref["dalpha"], ag["dalpha"]), case.name
        if d["res"] is not None:
            assert close(ref["dres"] if resb is not None else d["dy"].double(), ag["dres"]), case.name
        n += 1
    assert n >= 40


def test_z_equal_zero_takes_alpha_as_autograd():
    """The z <= 0 convention on exact zeros: the lattice has them, and F.prelu's autograd takes alpha there."""
    zeros = 0
    for case in E.case_table("lattice", Cs=(8, 256), dtypes=("f32",)):
        if not case.alpha:
            continue
        d = B.draw(case)
        sc, sh, mean, inv = E.eval_coefficients(d)
        resb = d["res"] if (case.res_first and case.residual) else None
        x = d["x"].double().requires_grad_(True)
        z = x * sc.double() + sh.double()
        if resb is not None:
            z = z + resb.double()
        zeros += int((z == 0).sum())
        (dx,) = torch.autograd.grad(F.prelu(z, d["alpha"].double()), x, d["dy"].double())
        ref = E.eval_reference(d["dy"], d["x"], sc, sh, d["alpha"], mean, inv, resb, torch.float32)
        assert torch.equal(ref["dx"], dx), case.name
    assert zeros > 100


@pytest.mark.parametrize("C", E.CS)
def test_restatement_within_budgets(C):
    rep = B.Report()
    for case in E.case_table("normal", Cs=(C,), variants="cycle"):
        E.check_eval_case(E.Restatement(), case, rep)
    assert not rep.failures, rep.failures[:10]
    print(rep.table())


def test_restatement_exact_on_lattice():
    rep = B.Report()
    for case in E.case_table("lattice"):
        E.check_eval_case(E.Restatement(), case, rep)
    assert not rep.failures, rep.failures[:10]


def _mutant_cases():
    """A small set on which every planted fault shows: exact zeros of z (lattice), residual_first, few and many pixels."""
    return E.case_table("lattice", Cs=(8,)) + E.case_table("normal", Cs=(8,), dtypes=("f32",), Ms=(2, 257))


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_mutants_are_rejected(mutant):
    rep = B.Report()
    for case in _mutant_cases():
        E.check_eval_case(E.Restatement(mutant), case, rep)
    assert rep.failures, "the checks accept the planted fault %r" % mutant


def test_clean_restatement_passes_the_mutant_cases():
    rep = B.Report()
    for case in _mutant_cases():
        E.check_eval_case(E.Restatement(), case, rep)
    assert not rep.failures, rep.failures[:10]
