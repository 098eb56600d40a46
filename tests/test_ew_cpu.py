"""CPU side of the FM / KD / segmentation-loss / LightCNN / split-bf16 kernel tests (tests/ew_cases.py): the f64 references
are checked against torch's own functions and the oracle before anything is checked against them, the torch restatement
of the kernels' arithmetic passes every derived budget on every case of every table (the budgets are satisfiable, no case
excluded), and every single-fault mutant of it fails the check named for it (the budgets have power)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as O
from tests import ew_cases as E
from tests import head_cases as H


def _close(a, b, what, scale=1.0):
    """f64 against f64, other operation order: 2^-53 x (terms of the longest sum, < 2^16 here) x 8, relative to the largest
    magnitude of the tensor."""
    tol = 8 * 65536 * H.U64 * max(1.0, float(b.abs().max())) * scale
    assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)


# ------------------------------------------------------------------------------------------------- the references
def test_libm_constants_cover_tanh_and_log():
    got = H.measure_libm()
    for fn in ("tanh", "log", "exp"):
        print("%-5s measured %.3f u32, recorded %.3f, budget %.3f" % (fn, got[fn], H.LIBM_MEASURED[fn], H.L(fn)))
        assert got[fn] <= H.L(fn), fn


def test_fuse_reference_equals_torch_autograd():
    torch.manual_seed(1)
    for act, fn in ((E.TANH, torch.tanh), (E.SIGMOID, torch.sigmoid)):
        for arith in (E.ADD, E.SUB, E.MUL, E.DIV):
            x = (torch.rand(500, dtype=torch.float64) * 8.0 + 0.05).requires_grad_(True)
            y = torch.randn(500, dtype=torch.float64, requires_grad=True)
            d = torch.randn(500, dtype=torch.float64)
            m = fn(x)
            z = (y + m, y - m, y * m, y / m)[arith] + y
            gx, gy = torch.autograd.grad(z, (x, y), d)
            (rz, _), (rx, _), (ry, _) = E.fuse_reference(x.detach(), y.detach(), d, act, arith, 0.0)
            _close(rz, z.detach(), "z")
            _close(rx, gx, "dx", 500.0)
            _close(ry, gy, "dyf", 500.0)
            mm, _, g, _ = E.act_terms(x.detach(), act)
            (gm,) = torch.autograd.grad(fn(x), x, torch.ones_like(x))
            _close(mm, fn(x).detach(), "m")
            _close(g, gm, "dm/dx")


def test_mse_reference_equals_nn_mseloss():
    torch.manual_seed(2)
    a = torch.randn(40, 8, dtype=torch.float64)
    b = torch.randn(40, 8, dtype=torch.float64)
    a[:, 5:], b[:, 5:] = 0.0, 0.0
    ar = a[:, :5].clone().requires_grad_(True)
    loss = torch.nn.MSELoss()(ar, b[:, :5])
    loss.backward()
    _close(E.mse_reference(a, b, 200.0), loss.detach(), "mse")
    _close((2.0 / 200.0) * (a - b)[:, :5], ar.grad, "d mse / da")


def test_dropout_hash_restatement():
    """The integer restatement against Python's own arbitrary-precision integers; the planted seeds hit the threshold; the
    keep rate at the grid-stride size lies within 4 binomial sigma of 1 - p."""
    def py_hash(seed, i):
        z = ((seed & E._M64) + i * E._GOLD) & E._M64
        z = ((z ^ (z >> 30)) * E._C1) & E._M64
        z = ((z ^ (z >> 27)) * E._C2) & E._M64
        return (z ^ (z >> 31)) >> 32
    for seed in E.DROP_SEEDS:
        idx = np.array([0, 1, 7, 2 ** 22 + 3, E.FM_NS[-1] - 1], dtype=np.uint64)
        assert [int(v) for v in E.drop_hash(seed, idx)] == [py_hash(seed, int(i)) for i in idx]
    assert int(E.drop_thr(0.5)) == 1 << 31 and int(E.drop_thr(0.0)) == 0
    assert int(E.drop_thr(0.4)) == int(float(np.float32(0.4)) * 2.0 ** 32)
    for n, p, i in E.PLANTED_DROPS:
        seed = E.planted_seed(i, E.drop_thr(p))
        assert -(1 << 63) <= seed < (1 << 63) and py_hash(seed, i) == int(E.drop_thr(p))
        assert bool(E.keep_mask(seed, n, p)[i]) and not bool(E.keep_mask(seed, n, p, strict=True)[i])
    n = E.FM_NS[-1]
    for p, seed in zip(E.DROP_PS, E.DROP_SEEDS):
        q = 1.0 - float(np.float32(p))
        rate = float(E.keep_mask(seed, n, p).double().mean())
        assert abs(rate - q) <= 4.0 * (q * (1.0 - q) / n) ** 0.5 + 2.0 ** -32, (p, seed, rate)


def test_dap_reference_equals_oracle_dap():
    torch.manual_seed(3)
    x = torch.randn(2, 5, 7, 24, dtype=torch.float64)
    xc = x[..., :18].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    seg = O.dap(xc)
    dseg = torch.randn(2, 2, 5, 7, dtype=torch.float64)
    seg.backward(dseg)
    be = E.Restatement()
    s32, mask = be.dap_fwd(x.float(), True)
    assert float((s32.double() - O.dap(x.float().double()[..., :18].permute(0, 3, 1, 2))).abs().max()) < 1e-6
    assert torch.equal(mask.bool(), s32[:, 1] > s32[:, 0])
    dx = be.dap_bwd(dseg.float(), 24, torch.float32)
    assert float((dx[..., :18].double() - xc.grad.permute(0, 2, 3, 1)).abs().max()) < 1e-6
    assert not bool(dx[..., 18:].any())


def test_consensus_expr_equals_oracle():
    """ew_cases.consensus_expr (which supplies the gradient elements the oracle's autograd leaves NaN) has the oracle's value
    on every case and the oracle's gradient wherever that is finite; NaN appears only under reduce_pixel = 'all' in images
    that lack a blob other images have."""
    nan_cases = 0
    for c in E.seg_cases():
        logit, msk = E.draw_seg(c)
        l1, d1, l2, d2 = E.seg_reference(logit, msk, c.ab[0], c.ab[1], c.mean_all, c.kl_all, parts=True)
        assert bool(torch.isfinite(l1)) and bool(torch.isfinite(d2).all()), c.name
        _close(l2, l1, c.name + " loss")
        bad = torch.isnan(d1)
        if bool(bad.any()):
            nan_cases += 1
            assert c.mean_all, c.name
            lacks = torch.stack([(msk.view(c.N, -1) == s).sum(1) == 0 for s in (0, 1)], 1).any(1)        # [N]
            assert torch.equal(bad.view(c.N, -1).any(1), lacks), c.name
        _close(torch.where(bad, d1.new_zeros(()), d2), torch.where(bad, d1.new_zeros(()), d1), c.name + " dlogit")
    print("cases with NaN in the oracle's autograd gradient:", nan_cases)


def test_seg_domain_edge():
    """Outside the domain the kernel's 2 * sup and the reference's count of non-zero entries part.  At |l0 - l1| = 120 the
    smaller f32 probability is 0: the oracle, run in f32 as the original is, counts 3 non-zero entries where 2 * sup is 4
    and drops that entry's log from its sum, and its loss leaves the kernel arithmetic's (the restatement) far behind.
    At |l0 - l1| = 30, the edge the cases draw, the two still agree to f32 rounding."""
    msk = torch.zeros(1, 1, 2, dtype=torch.int64)                              # N = 1, H = 1, W = 2, one blob
    for d, inside in ((30.0, True), (120.0, False)):
        logit = torch.tensor([[[[d / 2, 0.3]], [[-d / 2, -0.2]]]])
        nz = int((torch.softmax(logit, 1) != 0).sum())
        assert nz == (4 if inside else 3) and 2 * int((msk == 0).sum()) == 4
        ref = float(O.consensus_loss(logit, msk, 0.0, 1.0))
        got = float(E.Restatement().seg_loss(logit, msk, 0.0, 1.0, 0, 0, False)[0])
        assert (abs(got - ref) <= 1e-5 * abs(ref)) == inside, (d, ref, got)
    assert float(torch.softmax(torch.tensor([0.0, -E.MAX_DIFF]), 0).min()) >= 9e-14


def test_pool_reference_and_mfm_rule_equal_torch():
    # torch's CPU max_pool2d on the planted windows: ties keep the first maximum, a NaN wins (what lightcnn.hip restates)
    for win in E.POOL_WINDOWS:
        v = torch.tensor(win, dtype=torch.float64)
        want = 0
        for k in range(1, 4):
            if v[k] > v[want] or v[k] != v[k]:
                want = k
        _, idx = F.max_pool2d(v.view(1, 1, 2, 2), 2, return_indices=True)
        assert int(idx) == want, win
    assert len(E.POOL_WINDOWS) == 1 + 4 + 6 + 2 + 4
    # torch.max of two tensors: a tie splits the gradient, a NaN passes all of it to both
    a = torch.tensor([1.0, 2.0, 3.0, float("nan"), 5.0, float("nan")], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([1.0, 3.0, 2.0, 4.0, float("nan"), float("nan")], dtype=torch.float64, requires_grad=True)
    d = torch.tensor([2.0, 4.0, 6.0, 8.0, 10.0, 12.0], dtype=torch.float64)
    torch.max(a, b).backward(d)
    sel = torch.tensor([[0, 2, 1, 3, 3, 3]], dtype=torch.uint8)
    ref = E.mfm_reference(d[None], sel, 6, 16)
    assert torch.equal(ref[0, :6], a.grad) and torch.equal(ref[0, 6:12], b.grad) and not bool(ref[0, 12:].any())


def test_x3_split_carries_16_bits():
    torch.manual_seed(5)
    v = torch.randn(4096, 8) * torch.exp(4.0 * torch.randn(4096, 8))
    t = E.x3_split(v)
    worst = float(((E.x3_value(t, 8) - v.double()).abs() / v.double().abs()).max())
    print("worst relative error of hi + lo: 2^%.2f" % np.log2(worst))
    assert E.U_SPLIT < worst <= E.SAFETY * E.U_SPLIT            # the budget of the split store, with SAFETY, is the measured maximum
    worst = float(((v.bfloat16().double() - v.double()).abs() / v.double().abs()).max())
    assert E.UBF < worst <= E.SAFETY * E.UBF                     # and that of a bf16 store the half ulp an RNE store reaches
    assert len({v for c in E.x3_cases() if c.M * c.C <= E.FM_CAP for v in E.x3_bn_variants(c)}) == 24 == len(E._BN_VARIANTS)
    assert torch.equal(t[:, :8], t[:, 16:])
    # +-FLT_MAX, 0x7F7F8000 and +-inf read back as the infinity, 0x7F7F7FFF as itself to 16 bits
    sp = torch.tensor(E.X3_SPECIAL_BITS[:6], dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert bool(torch.isfinite(E.Restatement().x3_to_f32(E.x3_split(sp[3:4].view(1, 1)), 1)).all())
    sp = sp[[0, 1, 2, 4, 5]].view(1, 5)
    back = E.Restatement().x3_to_f32(E.x3_split(sp), 5)
    assert bool(torch.isinf(back).all()) and torch.equal(torch.sign(back), torch.sign(sp))


# ------------------------------------------------------------------------- the restatement is inside every budget
@pytest.mark.parametrize("family", sorted(E.CHECKS))
def test_restatement_within_budget(family):
    check, table = E.CHECKS[family]
    rep = E.Report()
    cases = table()
    for c in cases:
        check(E.Restatement(), c, rep)
    print("\n%d cases\n%s" % (len(cases), rep.table()))
    assert not rep.failures, rep.failures[:10]


# ----------------------------------------------------------------------------------------- every mutant is caught
def _mutant_cases(name, family):
    cases = E.CHECKS[family][1]()
    if family == "fm":
        if name == "grid_tail_dropped":
            return [c for c in cases if c.n > E.FM_CAP][:2]
        return [c for c in cases if c.n == 2056]
    if family == "dropout":
        return [c for c in cases if c.planted is not None]
    if family == "dap":
        return [c for c in cases if c.N * c.H * c.W < 1 << 16]
    if family == "x3":
        return [c for c in cases if c.M <= 257]
    if family == "seg":
        return [c for c in cases if c.N * c.H * c.W < 1 << 20]
    return cases


@pytest.mark.parametrize("mutant", sorted(E.MUTANTS))
def test_mutant_is_caught(mutant):
    family, key, what = E.MUTANTS[mutant]
    rep = E.Report()
    for c in _mutant_cases(mutant, family):
        E.CHECKS[family][0](E.Restatement(mutant), c, rep)
    hits = [f for f in rep.failures if f[0] == key and f[1].startswith(what)]
    assert hits, (mutant, rep.failures[:5])


# --------------------------------------------------------------------------------- refusals need no GPU: none launches
@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU tests/test_gpu_ew.py::test_refusals runs the table on device "
                    "tensors: a host check that regressed would launch on this test's host buffer")
def test_refusals_without_gpu():
    import ctypes
    from msml_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 2048)()
    table = E.refusal_table(ctypes.addressof(buf))
    assert len(table) > 150
    for name, args, want in table:
        assert getattr(lib, name)(*args, None) == want, (name, args, want, lib.msml_last_error())
