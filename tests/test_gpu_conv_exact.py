"""The conv forward and backward-data kernels on the MI355X through the C ABI (msml_conv2d, msml_conv2d_acc,
msml_conv2d_fused, msml_conv2d_bnbwd[_acc], msml_conv2d_bnin[_acc], msml_deconv4_bwd_data) against the float64 restatement
and the derived budget of tests/conv_cases.py (the checks tests/test_conv_cpu.py runs the mutants against): bit equality of
the output, the statistics and the fused BatchNorm-backward sums on integer data for every case, the budget and equal bits
of two calls on random data, the BatchNorm-in-LDS entry points against msml_bn_act_fwd + msml_conv2d and
msml_bn_fin_act_fwd + msml_conv2d_acc bit for bit, and the refusals.  Memory hygiene as in tests/abi_harness.py: every
output lies between guard bands and is pre-filled with NaN (statistics rows and bnbwd rows included: every row the header
sizes must be written, no row beyond *rows_used may be), inputs are compared after the call.

Figures of the run this file was written against (MI355X, 308 tests in 33 s, the slowest 2.4 s): every exact case bit-equal;
worst error / allowance on random data (out / statistics / bnbwd sums): ws 0.936 / 0.0001 / 0.0003, s2r 0.973 / 0 / 0,
r32 0.981 / 0.0002 / 0.0010, pw 0.998 / 0.0040 / 0.0034, halo 0.845 / 0.0001 / 0.0019, halo_p 0.950 / 0 / 0, halo2 0.926 / 0 /
0.0001, line 0.988, d4 0.946, fast 0.993 / 0 / 0.0004, igemm 0.995 / 0.0008.  A bf16 out sits just below 1 by construction:
a correctly rounded result may lie half an ulp from the f64 value and that half ulp is most of the allowance; the f32
outputs show the accumulation alone, 0.0017 to 0.0067 (docs/KERNELS.md, "Conv forward and backward-data kernel tests")."""
import ctypes

import pytest
import torch

from msml_amd import _lib
from tests import conv_cases as C
from tests.abi_harness import GuardedDevice

pytestmark = pytest.mark.gpu
CASES = C.cases()
_DEVICE = {}
WORST = {}


def kpad(k):
    return C.cdiv(k, 32) * 32


def pack(w, c1, c1p, c2, c2p, kop, r, s, dtype):
    """msml_pack_weight of w [A][c1 + c2][R][S] (transpose 0: ko = a), the destination pre-filled with NaN."""
    ktot = kpad(r * s * c1p) + (kpad(r * s * c2p) if c2 else 0)
    wp = torch.full((kop, ktot), float("nan"), dtype=_lib.TORCH_DTYPE[dtype], device="cuda")
    _lib.call("msml_pack_weight", w.cuda().contiguous(), wp, w.shape[0], w.shape[1], r, s, 0, c1, c1p, c2, c2p, kop, dtype)
    return wp


def device_data(c, kind):
    """The operands of the case on the device, uploaded and packed once per (case, kind)."""
    key = (c.name, kind)
    if key not in _DEVICE:
        _DEVICE.clear()                                   # (one case at a time: the large cases hold 30 MB tensors)
        d = C.reference(c, kind)[0]
        dd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items() if k != "w"}
        if c.entry == "deconv4_bwd_data":
            dd["wp0"] = pack(d["w"][:18], 18, 32, 0, 0, 32, 4, 4, _lib.BF16)
            dd["wp1"] = pack(d["w"][18:], 18, 32, 0, 0, 32, 4, 4, _lib.BF16)
        else:
            dd["wp"] = pack(d["w"], c.c0, c.c0p, c.c1, c.c1p, C.kop(c), c.R, c.S, c.dtype[0])
        if c.entry == "bnin_acc":
            acc, count, gamma, beta = C.bnin_acc_operands(c, d, kind)
            dd.update(acc_in=acc.cuda(), count=count, gamma=gamma.cuda(), beta=beta.cuda())
        _DEVICE[key] = dd
    return _DEVICE[key]


def launch(c, dd, entry=None, x0=None):
    """One call of the case's entry point; returns what it stored: out, stats / bnb as float64 column sums (and the raw
    buffers under "raw"), for bnin_acc also act and coef.  entry / x0: the unfused counterpart on another input tensor."""
    entry = entry or c.entry
    x0 = dd["x0"] if x0 is None else x0
    dev = GuardedDevice()
    shape = (c.N, c.H, c.W, c.P, c.Q, c.R, c.S, c.stride, c.ph, c.pw)
    got, raw = {}, {}
    with C.switched(c):
        if entry == "deconv4_bwd_data":
            dx0, dx1 = dev.out((c.N, c.P, c.Q, 32), torch.bfloat16), dev.out((c.N, c.P, c.Q, 32), torch.bfloat16)
            dev.call("msml_deconv4_bwd_data", x0, dd["wp0"], dd["wp1"], dx0, dx1, c.N, c.P)
            torch.cuda.synchronize()
            return dict(out=torch.cat([dx0, dx1], 3).cpu(), raw={})
        out = dev.out((c.N, c.P, c.Q, c.coutp), C.out_dtype(c))
        stats = None
        if c.stats == "rows" and entry in ("conv2d", "bnin"):
            stats = dev.out((C.cdiv(c.N * c.P * c.Q, C.tile_m(c.coutp)), 2, c.coutp), torch.float32)
        elif c.stats:
            stats = dev.out((8, 2, c.coutp), torch.float64, init=0.0)
        head = (x0, c.c0p, dd.get("x1"), c.c1p, dd["wp"], C.kop(c))
        if entry in ("conv2d", "conv2d_acc"):
            dev.call("msml_" + entry, *head, dd.get("bias"), out, c.coutp, stats, *shape, c.tr, c.dtype[0], c.dtype[1])
        elif entry == "fused":
            dev.call("msml_conv2d_fused", *head, dd.get("scale"), dd["bias"], dd.get("alpha"), dd.get("res"), c.res_first, out,
                     c.coutp, *shape, c.tr)
        elif entry in ("bnbwd", "bnbwd_acc"):
            bn = (dd["bn_x"], dd["bn_scale"], dd["bn_shift"], dd["bn_alpha"], dd["bn_mean"], dd["bn_invstd"])
            if entry == "bnbwd":
                cap = _lib.value("msml_conv2d_bnbwd_rows", c.coutp, c.N, c.P, c.Q)
                part = dev.out((cap, 3, c.coutp), torch.float32)
                used = ctypes.c_int(-1)
                dev.call("msml_conv2d_bnbwd", x0, c.c0p, dd["wp"], C.kop(c), out, c.coutp, *shape, c.tr, *bn, part, cap,
                         ctypes.byref(used))
                torch.cuda.synchronize()
                assert used.value == C.route(c)[1], (c.name, used.value, C.route(c))
                assert bool(torch.isfinite(part[:used.value]).all()), "a bnbwd row below *rows_used was not written"
                assert bool(torch.isnan(part[used.value:]).all()), "a bnbwd row beyond *rows_used was written"
                raw["bnb"], got["bnb"] = part[:used.value], part[:used.value].double().sum(0).cpu()
            else:
                acc = dev.out((8, 3, c.coutp), torch.float64, init=0.0)
                dev.call("msml_conv2d_bnbwd_acc", x0, c.c0p, dd["wp"], C.kop(c), out, c.coutp, *shape, c.tr, *bn, acc)
                raw["bnb"], got["bnb"] = acc, acc.sum(0).cpu()
        elif entry == "bnin":
            dev.call("msml_conv2d_bnin", x0, c.c0p, dd["in_scale"], dd["in_shift"], dd["in_alpha"], dd["wp"], C.kop(c), out,
                     c.coutp, stats, *shape)
        else:
            assert entry == "bnin_acc"
            coef, act = dev.out((4, c.c0p), torch.float32), dev.out((c.N, c.H, c.W, c.c0p), torch.bfloat16)
            rm, rv = dev.out((c.c0p,), torch.float32, init=0.0), dev.out((c.c0p,), torch.float32, init=1.0)
            dev.call("msml_conv2d_bnin_acc", x0, c.c0p, dd["acc_in"], dd["count"], dd["gamma"], dd["beta"], rm, rv, 0.1, C.EPS,
                     coef, dd["in_alpha"], act, dd["wp"], C.kop(c), out, c.coutp, stats, *shape)
            got.update(act=act, coef=coef, running=(rm, rv))
    torch.cuda.synchronize()
    got["out"] = out.cpu()
    if stats is not None:
        assert bool(torch.isfinite(stats).all()), "%d statistics elements were not written" % int((~torch.isfinite(stats)).sum())
        raw["stats"], got["stats"] = stats, stats.double().sum(0).cpu()
    got["raw"] = raw
    return got


def layout(c, want):
    """`want` in the layout the call stores: msml_deconv4_bwd_data writes its 36 channels as two 18-of-32 tensors."""
    if c.entry != "deconv4_bwd_data":
        return want
    w = dict(want)
    for k in ("out", "final", "allow"):
        w[k] = torch.cat(C.d4_split(c, want[k]), 3)
    return w


def bn_act(c, dd):
    """What msml_bn_act_fwd makes of in0 with the case's input BatchNorm."""
    act = torch.empty_like(dd["x0"])
    _lib.call("msml_bn_act_fwd", dd["x0"], dd["in_scale"], dd["in_shift"], dd["in_alpha"], None, 0, act, c.N * c.H * c.W, c.c0p,
              _lib.BF16)
    torch.cuda.synchronize()
    return act


def describe(c, want, got):
    g, w = got["out"].double(), want["out"].double()
    bad = (g != w) | torch.isnan(g)
    return "%s: %s; first at %s: got %s, want %s" % (c.name, "; ".join(C.exact_failures(c, want, got)), bad.nonzero()[:4].tolist(),
                                                     g[bad][:4].tolist(), w[bad][:4].tolist())


# ------------------------------------------------------------------------------------------- 1. integer data: equal bits
@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_exact_data_is_bit_equal(case):
    """Every summation order gives these integers exactly: out (pad channels 0, no element left NaN), the column sums of
    the statistics and the bnbwd sums are compared with torch.equal -- no element and no case is left out."""
    c = case
    dd = device_data(c, "exact")
    got = launch(c, dd)
    want = layout(c, C.expect(c, "exact"))
    assert C.exact_failures(c, want, got) == [], describe(c, want, got)
    if c.entry == "bnin_acc":                            # the coefficients are the constructed ones, the activation is exact
        d = want["d"]
        assert torch.equal(got["coef"][0, :c.c0].cpu(), d["in_scale"][:c.c0]) and torch.equal(got["coef"][1, :c.c0].cpu(), d["in_shift"][:c.c0])
        assert bool((got["coef"][3, :c.c0] == 2.0).all())
        assert torch.equal(got["act"][..., :c.c0].cpu(), C.bn_apply(d["x0"], d["in_scale"], d["in_shift"], d["in_alpha"])[..., :c.c0])
    C.forget()


# ------------------------------------------------------------------------------------------- 2. random data: the budget
@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_random_data_within_budget_and_deterministic(case):
    c = case
    dd = device_data(c, "random")
    got, again = launch(c, dd), launch(c, dd)
    assert torch.equal(got["out"].view(torch.int16 if got["out"].dtype == torch.bfloat16 else torch.int32),
                       again["out"].view(torch.int16 if got["out"].dtype == torch.bfloat16 else torch.int32)), "two calls differ: out"
    for k, buf in got["raw"].items():                    # statistics rows, accumulators (their totals do not depend on the
        other = again["raw"][k]                          # order of the adds: include/msml_hip.h), bnbwd rows
        bits = torch.int32 if buf.dtype == torch.float32 else torch.int64
        assert torch.equal(buf.view(bits), other.view(bits)), "two calls differ: %s" % k
    x_operand = None
    if c.entry == "bnin":                                # behind the BatchNorm the operand is what msml_bn_act_fwd stores
        x_operand = bn_act(c, dd).cpu()
    elif c.entry == "bnin_acc":                          # ... or what the call itself wrote (test 3 compares it with the chain)
        x_operand = got["act"].cpu()
    want = layout(c, C.expect(c, "random", x_operand))
    ratios = C.budget_ratios(c, want, got)
    WORST[c.family] = max(WORST.get(c.family, 0.0), max(ratios.values()))
    print("   %-36s k %5d  worst |err| / budget %s   (%s so far: %.4f)" % (
        c.name, C.kterms(c), {k: round(v, 4) for k, v in ratios.items()}, c.family, WORST[c.family]))
    assert max(ratios.values()) <= 1.0, (c.name, ratios)
    C.forget()


# ------------------------------------------------------------------------------------------- 3. BatchNorm in LDS
@pytest.mark.parametrize("kind", ("exact", "random"))
@pytest.mark.parametrize("case", [c for c in CASES if c.entry == "bnin"], ids=C.case_id)
def test_bnin_equals_bn_act_fwd_then_conv2d(case, kind):
    c = case
    dd = device_data(c, kind)
    act = bn_act(c, dd)
    if kind == "exact":                                  # the coefficients are powers of two: no rounding anywhere
        assert torch.equal(act.cpu(), C.bn_apply(dd["x0"].cpu(), *[None if dd[k] is None else dd[k].cpu() for k in ("in_scale", "in_shift", "in_alpha")]))
    fused = launch(c, dd)
    plain = launch(c, dd, entry="conv2d", x0=act)
    assert torch.equal(fused["out"].view(torch.int16), plain["out"].view(torch.int16))
    if c.stats:
        assert torch.equal(fused["raw"]["stats"].view(torch.int32), plain["raw"]["stats"].view(torch.int32))
    C.forget()


@pytest.mark.parametrize("kind", ("exact", "random"))
@pytest.mark.parametrize("case", [c for c in CASES if c.entry == "bnin_acc"], ids=C.case_id)
def test_bnin_acc_equals_bn_fin_act_fwd_then_conv2d_acc(case, kind):
    c = case
    dd = device_data(c, kind)
    fused = launch(c, dd)
    coef = torch.full((4, c.c0p), float("nan"), device="cuda")
    act = torch.full_like(dd["x0"], float("nan"))
    rm, rv = torch.zeros(c.c0p, device="cuda"), torch.ones(c.c0p, device="cuda")
    _lib.call("msml_bn_fin_act_fwd", dd["acc_in"], dd["count"], dd["gamma"], dd["beta"], rm, rv, 0.1, C.EPS, coef[0], coef[1],
              coef[2], coef[3], dd["x0"], dd["in_alpha"], None, 0, act, c.N * c.H * c.W, c.c0p, None, _lib.BF16)
    torch.cuda.synchronize()
    plain = launch(c, dd, entry="conv2d_acc", x0=act)
    assert torch.equal(fused["act"].view(torch.int16), act.view(torch.int16))
    assert torch.equal(fused["coef"].view(torch.int32), coef.view(torch.int32))
    assert torch.equal(fused["running"][0], rm) and torch.equal(fused["running"][1], rv)
    assert torch.equal(fused["out"].view(torch.int16), plain["out"].view(torch.int16))
    assert torch.equal(fused["stats"].view(torch.int64), plain["stats"].view(torch.int64))
    C.forget()


# ------------------------------------------------------------------------------------------- 4. the refusals
@pytest.mark.parametrize("case", C.REFUSED, ids=C.case_id)
def test_refusal_leaves_every_output_alone(case):
    """MSML_ERR_UNSUPPORTED before any launch (tests/test_conv_cpu.py reaches the same refusals with host pointers): out,
    the statistics / partial rows and *rows_used stay as pre-filled."""
    c = case
    dev = GuardedDevice()
    x = torch.zeros(4096, dtype=torch.bfloat16, device="cuda")
    f = torch.ones(4096, device="cuda")
    out, side = dev.out((4096,), torch.bfloat16, init=7.0), dev.out((4096,), torch.float32, init=7.0)
    shape = (c.N, c.H, c.W, c.P, c.Q, c.R, c.S, c.stride, c.ph, c.pw)
    used = ctypes.c_int(-7)
    if c.entry == "bnin":
        rc = _lib.call_status("msml_conv2d_bnin", x, c.c0p, f, f, None, x, C.kop(c), out, c.coutp, side if c.stats else None, *shape)
    elif c.entry == "bnin_acc":
        rc = _lib.call_status("msml_conv2d_bnin_acc", x, c.c0p, f, 1.0, f, f, None, None, 0.1, C.EPS, side, None, out, x, C.kop(c),
                              out, c.coutp, side, *shape)
    else:
        rc = _lib.call_status("msml_conv2d_bnbwd", x, c.c0p, x, C.kop(c), out, c.coutp, *shape, c.tr, x, f, f, None, f, f, side,
                              1 << 30, ctypes.byref(used))
    torch.cuda.synchronize()
    assert rc == _lib.UNSUPPORTED, (c.name, rc)
    assert used.value == -7 and bool((out == 7.0).all()) and bool((side == 7.0).all())
