"""The weight-gradient kernels on the MI355X through the C ABI (msml_conv_wgrad, msml_conv_wgrad_group,
msml_conv_wgrad_bnin) against the float64 restatement and the derived budget of tests/wgrad_cases.py (the checks
tests/test_wgrad_cpu.py runs the mutants against): bit equality on integer data for every case and both `accumulate`
settings, the budget and equal bits of two calls on random data, the BatchNorm-in-LDS entry point against
msml_bn_act_fwd + msml_conv_wgrad bit for bit.  Memory hygiene as in tests/abi_harness.py: dW and the workspace lie
between guard bands, the workspace is pre-filled with NaN and may be written only where the plan says, inputs are
compared after the call.

The pixel-decode case runs at N = 3064 (4.19 M pixels, 342 splits of 12 288), not at N = 12 000: its float64 reference
and the host copies already take about 3 s at that size.

Figures of the run this file was written against (MI355X, 131 tests in 12 s): every exact case bit-equal; worst error /
budget on random data: halo128 0.0018, halo64 0.0028, pair7 0.0038, bnin 0.0008, im2col 0.0093, im2col_decode < 0.0001,
generic 0.0145, n32 0.0043, line 0.0010, fc 0.0293 (docs/KERNELS.md, "Weight-gradient kernel tests")."""
import contextlib
import ctypes

import pytest
import torch

from msml_amd import _lib
from tests import wgrad_cases as C
from tests.abi_harness import GuardedDevice

pytestmark = pytest.mark.gpu
CASES = C.cases()
PATHS = sorted({c.path for c in CASES})
NAN_BITS = torch.full((1,), float("nan")).view(torch.int32).item()
_DEVICE = {}


def device_layers(case, kind):
    """[(u, v, (scale, shift, alpha) or None)] on the device, one per layer of the call; uploaded once per (case, kind)."""
    key = (case.name, kind)
    if key not in _DEVICE:
        out = []
        for i in range(case.group):
            u, v, coef = C.reference(case, kind, i)[:3]
            if coef is not None:
                coef = tuple(None if t is None else t.cuda() for t in coef)
            out.append((u.cuda(), v.cuda(), coef))
        _DEVICE[key] = out
    return _DEVICE[key]


def launch(case, layers, accumulate, entry=None):
    """One call of the case's entry point (entry="one": msml_conv_wgrad on the same tensors); returns dW of every layer."""
    c, entry = case, entry or case.entry
    with _lib.option(c.switch, 1) if c.switch else contextlib.nullcontext():
        pl, rc = C.plan(c._replace(switch=None, entry=entry))
        assert rc == 0, (c.name, rc)
        if entry == "group":
            need = pl["slab"]
        else:
            need = _lib.value("msml_conv_wgrad_workspace", c.up, c.vp, c.N, c.P, c.Q, c.R, c.S)
        assert need % 4 == 0 and pl["slab"] <= need
        dev = GuardedDevice()
        ws = dev.out((max(need // 4, 1),), torch.float32)                    # NaN between two guard bands
        dws = [dev.out((c.A, c.Btot, c.R, c.S), torch.float32, init=C.init_dw(c, accumulate, i).cuda())
               for i in range(len(layers))]
        tail = (c.N, c.H, c.W, c.P, c.Q, c.R, c.S, c.stride, c.ph, c.pw, int(accumulate), ws, need)
        u0, v0, coef = layers[0]
        if entry == "one":
            dev.call("msml_conv_wgrad", u0, c.up, v0, c.vp, dws[0], c.A, c.Breal, c.Btot, c.boff, *tail, c.dtype)
        elif entry == "bnin":
            dev.call("msml_conv_wgrad_bnin", u0, c.up, v0, c.vp, coef[0], coef[1], coef[2], dws[0], c.A, c.Breal, c.Btot,
                     c.boff, *tail)
        else:
            arr = ctypes.c_void_p * len(layers)
            before = [(t, t.clone()) for lay in layers for t in lay[:2]]
            dev.call("msml_conv_wgrad_group", arr(*[l[0].data_ptr() for l in layers]), arr(*[l[1].data_ptr() for l in layers]),
                     arr(*[d.data_ptr() for d in dws]), len(layers), c.up, c.vp, c.A, c.Breal, c.Btot, c.boff, *tail, c.dtype)
            assert all(torch.equal(t.view(torch.int16), k.view(torch.int16)) for t, k in before), "the call modified an input"
    torch.cuda.synchronize()
    filled = ws.view(torch.int32) == NAN_BITS            # (a finite partial sum is never the pre-fill)
    written = pl["slab"] // 4
    assert not bool(filled[:written].any()), "%d of the %d announced slab dwords were not written" % (
        int(filled[:written].sum()), written)
    assert bool(filled[written:].all()), "the launch wrote past the slabs of its plan"
    return dws


def describe(got, want):
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    return "%d of %d elements differ, worst %.6g; first at %s: got %s, want %s" % (
        int(bad.sum()), bad.numel(), float((got - want).abs().nan_to_num(float("inf")).max()), idx[:4].tolist(),
        got[bad][:4].tolist(), want[bad][:4].tolist())


# ------------------------------------------------------------------------------------------- 1. integer data: equal bits
@pytest.mark.parametrize("accumulate", (0, 1), ids=("overwrite", "accumulate"))
@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_exact_data_is_bit_equal(case, accumulate):
    """Every summation order gives these integers exactly; the sentinel columns outside the window are part of `want`."""
    layers = device_layers(case, "exact")
    dws = launch(case, layers, accumulate)
    for i, dw in enumerate(dws):
        want = C.expected(case, C.reference(case, "exact", i)[3], C.init_dw(case, accumulate, i), accumulate)
        got = dw.cpu().double()
        assert torch.equal(got, want), "%s layer %d: %s" % (case.name, i, describe(got, want))


# ------------------------------------------------------------------------------------------- 2. random data: the budget
def random_reference(case, layers, i):
    """(dW, sum |u v|) in float64 of layer i; behind the BatchNorm the v operand is what msml_bn_act_fwd stores."""
    if case.entry != "bnin":
        return C.reference(case, "random", i)[3:]
    return C.reference(case, "random", i, v_operand=bn_act(case, layers[i]).cpu())[3:]


def bn_act(case, layer):
    _, v, coef = layer
    act = torch.empty_like(v)
    _lib.call("msml_bn_act_fwd", v, coef[0], coef[1], coef[2], None, 0, act, case.N * case.H * case.W, case.vp, _lib.BF16)
    torch.cuda.synchronize()
    return act


@pytest.mark.parametrize("path", PATHS)
def test_random_data_within_budget_and_deterministic(path):
    worst = 0.0
    for case in (c for c in CASES if c.path == path):
        pl, _ = C.plan(case)
        layers = device_layers(case, "random")
        for accumulate in (0, 1):
            dws, again = launch(case, layers, accumulate), launch(case, layers, accumulate)
            for i, dw in enumerate(dws):
                assert torch.equal(dw.view(torch.int32), again[i].view(torch.int32)), (case.name, i, "two calls differ")
                ref, mag = random_reference(case, layers, i)
                init = C.init_dw(case, accumulate, i)
                ratio = C.worst_ratio(dw.cpu(), C.expected(case, ref, init, accumulate),
                                      C.budget(case, pl, mag, init, accumulate))
                print("   %-34s layer %d accumulate %d  k %5d  worst |err| / budget %.4f" % (
                    case.name, i, accumulate, C.kfactor(case, pl, accumulate), ratio))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (case.name, i, accumulate, ratio)
    print("wgrad %s: worst error / budget %.4f" % (path, worst))


# ------------------------------------------------------------------------------------------- 3. BatchNorm in LDS
@pytest.mark.parametrize("kind", ("exact", "random"))
@pytest.mark.parametrize("case", [c for c in CASES if c.entry == "bnin"], ids=C.case_id)
def test_bnin_equals_bn_act_fwd_then_wgrad(case, kind):
    layers = device_layers(case, kind)
    u, v, coef = layers[0]
    act = bn_act(case, layers[0])
    if kind == "exact":                                  # the coefficients are powers of two: no rounding anywhere
        assert torch.equal(act.cpu(), C.bn_apply(v.cpu(), *[None if t is None else t.cpu() for t in coef]))
    for accumulate in (0, 1):
        fused = launch(case, layers, accumulate)[0]
        plain = launch(case, [(u, act, None)], accumulate, entry="one")[0]
        assert torch.equal(fused.view(torch.int32), plain.view(torch.int32)), describe(fused.cpu(), plain.cpu())


def test_bnin_refusal_leaves_dw_alone():
    c = C.REFUSED
    u, v = (t.cuda() for t in C.make_data(c, "exact"))
    scale, shift, _ = (None if t is None else t.cuda() for t in C.bn_coefficients(c, "exact"))
    dev = GuardedDevice()
    need = _lib.value("msml_conv_wgrad_workspace", c.up, c.vp, c.N, c.P, c.Q, c.R, c.S)
    ws = dev.out((max(need // 4, 1),), torch.float32)
    dw = dev.out((c.A, c.Btot, c.R, c.S), torch.float32, init=7.0)
    rc = _lib.call_status("msml_conv_wgrad_bnin", u, c.up, v, c.vp, scale, shift, None, dw, c.A, c.Breal, c.Btot, c.boff, c.N,
                          c.H, c.W, c.P, c.Q, c.R, c.S, c.stride, c.ph, c.pw, 0, ws, need)
    torch.cuda.synchronize()
    assert rc == _lib.UNSUPPORTED
    assert bool((dw == 7.0).all()) and bool((ws.view(torch.int32) == NAN_BITS).all())
