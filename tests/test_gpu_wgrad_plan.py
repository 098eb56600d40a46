"""msml_conv_wgrad_plan against the launches it describes: for the smallest shape at which each weight-gradient family
and variant is still chosen, the launch writes exactly the split-K slabs the plan announces (workspace pre-filled with
NaN between guard bands, tests/abi_harness.py) and the gradient is inside the bound the family's own test uses against
f64 torch on bf16-rounded inputs (test_gpu_conv.py: 1.5e-2 x max|ref| for the strip / halo, im2col and generic bf16
kernels, 2e-3 for the narrow-operand, line and fc kernels, 1e-5 for f32)."""
import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from msml_amd import _lib, ops
from tests.abi_harness import GuardedDevice

pytestmark = pytest.mark.gpu

FC, N32, LINE, HALO, FAST, GENERIC = range(1, 7)
BF16, F32 = _lib.BF16, _lib.F32


def conv(n, cin, cout, h, r=3, s=3, stride=1, ph=1, pw=1):
    return ("conv", n, cin, cout, h, r, s, stride, ph, pw)


def deconv4(n, c, p):
    return ("deconv", n, c, c, p, 4, 4, 2, 1, 1)


# id: (layer, entry, dtype, group, switch, tolerance, expected plan words)
CASES = {
    "halo64": (conv(2, 64, 64, 14), "one", BF16, 1, None, 1.5e-2, dict(family=HALO, variant=64, splits=4)),
    "halo128": (conv(2, 64, 128, 14), "one", BF16, 1, None, 1.5e-2, dict(family=HALO, variant=128)),
    "halo_pair7": (conv(5, 64, 64, 7), "one", BF16, 1, None, 1.5e-2, dict(family=HALO, variant=7, splits=3)),
    "halo_group2": (conv(2, 64, 64, 14), "group", BF16, 2, None, 1.5e-2, dict(family=HALO, variant=64, splits=2, group_max=2)),
    "halo_bnin": (conv(2, 64, 64, 14), "bnin", BF16, 1, None, 1.5e-2, dict(family=HALO, variant=64, splits=4)),
    "fast_direct": (conv(8, 64, 64, 4), "one", BF16, 1, None, 1.5e-2, dict(family=FAST, splits=1, direct=1, slab=0)),
    "fast_slabs": (conv(64, 64, 64, 4), "one", BF16, 1, None, 1.5e-2, dict(family=FAST, ntw=3, direct=0)),
    "fast_group2": (conv(64, 64, 64, 4), "group", BF16, 2, None, 1.5e-2, dict(family=FAST, ntw=3, group_max=4)),
    "fast_128": (conv(64, 128, 128, 4), "one", BF16, 1, None, 1.5e-2, dict(family=FAST, ba=128, bb=128)),
    "fast_1x1": (conv(16, 64, 64, 8, 1, 1, 1, 0, 0), "one", BF16, 1, None, 1.5e-2, dict(family=FAST, ntw=1)),
    "generic_f32": (conv(3, 64, 64, 14), "one", F32, 1, None, 1e-5, dict(family=GENERIC, ntw=1)),
    "generic_bf16": (conv(64, 64, 64, 4), "one", BF16, 1, "MSML_NO_FAST_WGRAD", 1.5e-2, dict(family=GENERIC, ntw=3)),
    "n32_3x3": (conv(1, 32, 32, 14), "one", BF16, 1, None, 2e-3, dict(family=N32)),
    "n32_deconv": (deconv4(1, 32, 14), "one", BF16, 1, None, 2e-3, dict(family=N32)),
    "line_7x1": (conv(1, 32, 32, 28, 7, 1, 1, 3, 0), "one", BF16, 1, None, 2e-3, dict(family=LINE)),
    "line_1x7": (conv(1, 64, 32, 28, 1, 7, 1, 0, 3), "one", BF16, 1, None, 2e-3, dict(family=LINE)),
    "fc": (conv(16, 32, 32, 2, 2, 2, 1, 0, 0), "one", BF16, 1, None, 2e-3, dict(family=FC, direct=1, slab=0)),
}
WORDS = ("family", "variant", "ba", "bb", "ntw", "splits", "chunk", "direct")


@functools.lru_cache(maxsize=None)
def layers(layer, dtype, group, bnin):
    """`group` layers of one shape: (u, v) NHWC device tensors, the f64 weight gradients, the BatchNorm input and its
    coefficients for the bnin entry point -- computed once per case, shared by its two `accumulate` runs."""
    kind, n, cin, cout, h, r, s, stride, ph, pw = layer
    g = torch.Generator().manual_seed(sum(layer[1:]) + group)
    rnd = (lambda t: t.bfloat16().float()) if dtype == BF16 else (lambda t: t)
    out = []
    for _ in range(group):
        x = rnd(torch.randn(n, cin, h, h, generator=g))
        coef = alpha = raw = None
        if bnin:                 # the stored tensor is the BatchNorm input; the conv saw PReLU(x * scale + shift)
            coef = torch.stack([torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.5]).cuda()
            alpha = (torch.rand(cin, generator=g) * 0.3).cuda()
            raw = ops.to_nhwc(x.cuda(), BF16)
            act = torch.empty_like(raw)
            _lib.call("msml_bn_act_fwd", raw, coef[0], coef[1], alpha, None, 0, act, n * h * h, cin, BF16)
            x = act.cpu().permute(0, 3, 1, 2).float()
        if kind == "deconv":     # u = x on the p x p grid, v = dY on the 2p x 2p grid, dW[cin][cout][4][4]
            w = torch.zeros(cin, cout, r, s, dtype=torch.double, requires_grad=True)
            y = F.conv_transpose2d(x.double(), w, None, stride, ph)
        else:                    # u = dY, v = x, dW[cout][cin][r][s]
            w = torch.zeros(cout, cin, r, s, dtype=torch.double, requires_grad=True)
            y = F.conv2d(x.double(), w, None, stride, (ph, pw))
        dy = rnd(torch.randn(y.shape, generator=g))
        y.backward(dy.double())
        xd, dyd = (raw if bnin else ops.to_nhwc(x.cuda(), dtype)), ops.to_nhwc(dy.cuda(), dtype)
        out.append((xd, dyd, w.grad.float(), coef, alpha) if kind == "deconv" else (dyd, xd, w.grad.float(), coef, alpha))
    return out


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_writes_the_slabs_of_its_plan(case, accumulate):
    layer, entry, dtype, group, switch, tol, expect = CASES[case]
    lay = layers(layer, dtype, group, entry == "bnin")
    u0, v0, ref0 = lay[0][:3]
    (n, p, q, up), (_, h, w, vp) = u0.shape, v0.shape
    a, breal, r, s = ref0.shape
    stride, ph, pw = layer[7:]
    shape = (up, vp, a, breal, breal, 0, n, h, w, p, q, r, s, stride, ph, pw)
    with _lib.option(switch, 1) if switch else contextlib.nullcontext():
        words, slab = (ctypes.c_int * 8)(), ctypes.c_long()
        assert _lib.load().msml_conv_wgrad_plan(*shape, dtype, group, int(entry == "bnin"), words, ctypes.byref(slab)) == 0
        plan = dict(zip(WORDS, words), slab=slab.value)
        need = _lib.value("msml_conv_wgrad_workspace", up, vp, n, p, q, r, s)
        print(case, plan, "workspace", need)
        if "group_max" in expect:
            assert _lib.value("msml_conv_wgrad_group_max", *shape[:4], *shape[6:]) == expect["group_max"]
        assert {k: plan[k] for k in expect if k != "group_max"} == {k: v for k, v in expect.items() if k != "group_max"}
        assert plan["slab"] == (0 if plan["direct"] else group * plan["splits"] * up * r * s * vp * 4) and plan["slab"] <= need
        assert need % 4 == 0
        dev = GuardedDevice()
        ws = dev.out((need // 4,), torch.float32)                  # NaN between two guard bands
        dws = [dev.out(tuple(ref0.shape), torch.float32, init=2.0 + i) for i in range(group)]
        tail = (n, h, w, p, q, r, s, stride, ph, pw, int(accumulate), ws, need)
        if entry == "one":
            dev.call("msml_conv_wgrad", u0, up, v0, vp, dws[0], a, breal, breal, 0, *tail, dtype)
        elif entry == "bnin":
            coef, alpha = lay[0][3:]
            dev.call("msml_conv_wgrad_bnin", u0, up, v0, vp, coef[0], coef[1], alpha, dws[0], a, breal, breal, 0, *tail)
        else:
            arr = ctypes.c_void_p * group
            dev.call("msml_conv_wgrad_group", arr(*[l[0].data_ptr() for l in lay]), arr(*[l[1].data_ptr() for l in lay]),
                     arr(*[d.data_ptr() for d in dws]), group, up, vp, a, breal, breal, 0, *tail, dtype)
    bits = ws.view(torch.int32)
    filled = bits == torch.full((1,), float("nan")).view(torch.int32).item()      # (a finite partial sum is never the pre-fill)
    written = plan["slab"] // 4
    assert not bool(filled[:written].any()), "%d of the %d announced slab dwords were not written" % (int(filled[:written].sum()), written)
    assert bool(filled[written:].all()), "the launch wrote past the slabs of its plan"
    for i in range(group):
        ref = lay[i][2]
        want = ref + (2.0 + i if accumulate else 0.0)
        err = (dws[i].cpu() - want).abs().max().item()
        print("layer %d: max err %.3e of max|ref| %.3e" % (i, err, ref.abs().max().item()))
        assert err <= tol * ref.abs().max().item(), i

