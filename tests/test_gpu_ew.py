"""The element-wise and loss entry points of msml_amd/csrc/fm.hip, seg.hip, lightcnn.hip and x3.hip through the C ABI
(msml_amd._lib.call) against the float64 references and the derived budgets of tests/ew_cases.py (the same checks
tests/test_ew_cpu.py runs on the torch restatement), with the memory hygiene of tests/abi_harness.py: outputs between
sentinel guard bands and pre-filled with NaN (0xEE bytes for the DAP mask), pad channels of inputs NaN (0xFF for selector
bytes), every input cloned before the call and compared after it.  Nothing here provokes a fault: every shape is one the
entry point documents as supported or must refuse on the host.

Outcome on an MI355X (worst error / budget, budgets already x SAFETY = 2): the table test_zz_report prints; the figures of
the run this file was written against are in docs/KERNELS.md, "FM, KD, segmentation, LightCNN and split-bf16 kernel
tests"."""
import time

import pytest
import torch

from msml_amd import _lib
from msml_amd import functional as FN
from tests import ew_cases as E
from tests.abi_harness import DTC, GuardedDevice

pytestmark = pytest.mark.gpu
REP = E.Report()
T0 = time.time()
POOL_CAP = 65536 * 256              # lanes of the capped mfm_bwd / pool2 grids


class Device(GuardedDevice):
    """The entry points with the interface of ew_cases.Restatement."""

    # ---- fm.hip
    def fm_fuse_fwd(self, x, yf, act, arith):
        z = self.out(tuple(x.shape), x.dtype)
        self.call("msml_fm_fuse_fwd", x, yf, z, x.numel(), act, arith, DTC[x.dtype])
        return z

    def fm_fuse_bwd(self, dz, x, yf, act, arith):
        dx, dyf = self.out(tuple(x.shape), x.dtype), self.out(tuple(x.shape), x.dtype)
        self.call("msml_fm_fuse_bwd", dz, x, yf, dx, dyf, x.numel(), act, arith, DTC[x.dtype])
        return dx, dyf

    def fm_act_fwd(self, x, act):
        m = self.out(tuple(x.shape), x.dtype)
        self.call("msml_fm_act_fwd", x, m, x.numel(), act, DTC[x.dtype])
        return m

    def fm_act_bwd(self, dm, x, act):
        dx = self.out(tuple(x.shape), x.dtype)
        self.call("msml_fm_act_bwd", dm, x, dx, x.numel(), act, DTC[x.dtype])
        return dx

    def mul_fwd(self, a, b):
        o = self.out(tuple(a.shape), a.dtype)
        self.call("msml_mul_fwd", a, b, o, a.numel(), DTC[a.dtype])
        return o

    def mul_bwd(self, g, a, b, need_a, need_b):
        da = self.out(tuple(a.shape), a.dtype) if need_a else None
        db = self.out(tuple(a.shape), a.dtype) if need_b else None
        self.call("msml_mul_bwd", g, a, b, da, db, a.numel(), DTC[a.dtype])
        return da, db

    def axpb(self, x, a, b):
        y = self.out(tuple(x.shape), x.dtype)
        self.call("msml_axpb", x, y, x.numel(), a, b, DTC[x.dtype])
        return y

    def mse_fwd(self, a, b, count):
        nb = E.fm_grid(a.numel() // 8)
        ws, loss = self.out((nb,), torch.float64), self.out((1,), torch.float32)      # exactly the partials the grid writes
        self.call("msml_mse_fwd", a, b, a.numel(), count, loss, ws, nb, DTC[a.dtype])
        assert bool(torch.isfinite(ws).all())
        return loss

    def mse_bwd(self, a, b, g, count, need_a, need_b):
        da = self.out(tuple(a.shape), a.dtype) if need_a else None
        db = self.out(tuple(a.shape), a.dtype) if need_b else None
        self.call("msml_mse_bwd", a, b, g, count, da, db, a.numel(), DTC[a.dtype])
        return da, db

    def dropout(self, x, p, seed, dev=False):
        y = self.out(tuple(x.shape), x.dtype)
        if dev:
            self.call("msml_dropout_dev", x, y, x.numel(), p, torch.tensor([seed], dtype=torch.int64, device="cuda"), DTC[x.dtype])
        else:
            self.call("msml_dropout", x, y, x.numel(), p, seed, DTC[x.dtype])
        return y

    # ---- seg.hip
    def dap_fwd(self, x, with_mask):
        N, H, W, Cp = x.shape
        seg = self.out((N, 2, H, W), torch.float32)
        mask = None
        if with_mask:               # a byte view of a guarded f32 buffer, pre-filled with 0xEE (no mask value)
            npix = N * H * W
            mask = self.out(((npix + 3) // 4,), torch.float32).view(torch.uint8)
            mask.fill_(0xEE)
            self.call("msml_dap_fwd", x, seg, mask, N, H, W, Cp, DTC[x.dtype])
            assert bool((mask[npix:] == 0xEE).all())
            mask = mask[:npix].view(N, H, W)
        else:
            self.call("msml_dap_fwd", x, seg, None, N, H, W, Cp, DTC[x.dtype])
        return seg, mask

    def dap_bwd(self, dseg, Cp, dtype):
        N, _, H, W = dseg.shape
        dx = self.out((N, H, W, Cp), dtype)
        self.call("msml_dap_bwd", dseg, dx, N, H, W, Cp, DTC[dtype])
        return dx

    def seg_loss(self, logit, msk, alpha, beta, mean_all, kl_all, want_grad):
        N, _, H, W = logit.shape
        loss, ws = self.out((1,), torch.float32), self.out((20 * N,), torch.float32)
        d = self.out(tuple(logit.shape), torch.float32) if want_grad else None
        self.call("msml_seg_consensus_loss_r", logit, msk, N, H, W, alpha, beta, mean_all, kl_all, loss, d, ws, 20 * N)
        return loss, d, ws

    def seg_loss_plain(self, logit, msk, alpha, beta):
        N, _, H, W = logit.shape
        loss, ws = self.out((1,), torch.float32), self.out((20 * N,), torch.float32)
        d = self.out(tuple(logit.shape), torch.float32)
        self.call("msml_seg_consensus_loss", logit, msk, N, H, W, alpha, beta, loss, d, ws, 20 * N)
        return loss, d

    # ---- lightcnn.hip
    def pool2_fwd(self, x):
        N, H, W, cp = x.shape
        y = self.out((N, H // 2, W // 2, cp), x.dtype)
        self.call("msml_pool2_fwd", x, y, N, H, W, cp, DTC[x.dtype])
        return y

    def pool2_bwd(self, dy, x):
        N, H, W, cp = x.shape
        dx = self.out(tuple(x.shape), x.dtype)
        self.call("msml_pool2_bwd", dy, x, dx, N, H, W, cp, DTC[x.dtype])
        return dx

    def mfm_bwd(self, dy, sel, C, czp):
        dz = self.out((dy.shape[0], czp), dy.dtype)
        self.call("msml_mfm_bwd", dy, sel, dz, dy.shape[0], dy.shape[1], C, czp, DTC[dy.dtype])
        return dz

    # ---- x3.hip
    def x3_from_f32(self, src):
        M, C = src.shape
        dst = self.out((M, 3 * C), torch.bfloat16)
        self.call("msml_x3_from_f32", src, dst, M, C)
        return dst

    def x3_to_f32(self, t, C):
        dst = self.out((t.shape[0], C), torch.float32)
        self.call("msml_x3_to_f32", t, dst, t.shape[0], C)
        return dst

    def x3_add(self, a, b, C):
        o = self.out(tuple(a.shape), torch.bfloat16)
        self.call("msml_x3_add", a, b, o, a.shape[0], C)
        return o

    def x3_bn_act(self, x, scale, shift, alpha, res, res_first, C):
        y = self.out(tuple(x.shape), torch.bfloat16)
        self.call("msml_x3_bn_act_fwd", x, scale, shift, alpha, res, res_first, y, x.shape[0], C)
        return y

    def x3_fm_fuse(self, x, yf, act, arith, C):
        z = self.out(tuple(x.shape), torch.bfloat16)
        self.call("msml_x3_fm_fuse_fwd", x, yf, z, x.shape[0], C, act, arith)
        return z


def _finish(n0):
    new = REP.failures[n0:]
    assert not new, new[:10]


def _run(family, **kw):
    n0 = len(REP.failures)
    check, table = E.CHECKS[family]
    for c in table():
        check(Device(), c, REP, "cuda", **kw)
    _finish(n0)


def test_fm_fuse():
    _run("fm")


def test_fm_act_mul_axpb():
    _run("ew")


def test_mse():
    _run("mse")


def test_dropout():
    _run("dropout")


def test_dap():
    _run("dap")


def test_seg_consensus_loss():
    _run("seg")


def test_pool2():
    _run("pool")


def test_mfm_bwd():
    count = [0, 0, 0, 0]
    _run("mfm", count=count)
    print("\nselector values 0..3 drawn:", count)
    assert min(count) > 0


def test_x3():
    _run("x3")


def test_mfm_bwd_over_the_grid_cap():
    """One call over the 65 536-block cap == two calls on its halves, bit for bit; a slice across the cap against the rule."""
    n0 = len(REP.failures)
    M, C = POOL_CAP + 2 * 4099, 4
    g = torch.Generator(device="cuda").manual_seed(11)
    dy = torch.randn(M, 8, device="cuda", generator=g)
    dy[:, C:] = float("nan")
    sel = torch.randint(0, 4, (M, 8), device="cuda", dtype=torch.uint8, generator=g)
    sel[:, C:] = 0xFF
    assert M > POOL_CAP > M // 2
    full = Device().mfm_bwd(dy, sel, C, 8)
    for lo, hi in ((0, M // 2), (M // 2, M)):
        part = Device().mfm_bwd(dy[lo:hi], sel[lo:hi], C, 8)
        assert torch.equal(part.view(torch.int32), full[lo:hi].view(torch.int32)), "halves differ from the one call"
        del part
    c = E.Case("mfm-over-cap", dtype="f32")
    for lo in (0, POOL_CAP - 2048, M - 4096):
        REP.exact("mfm_bwd", "dz rows %d.." % lo, full[lo:lo + 4096], E.mfm_reference(dy[lo:lo + 4096], sel[lo:lo + 4096], C, 8), c)
    _finish(n0)


def test_pool2_over_the_grid_cap():
    n0 = len(REP.failures)
    N = POOL_CAP + 2 * 4099
    g = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(N, 2, 2, 8, device="cuda", dtype=torch.bfloat16, generator=g)
    v = torch.randn(N, 1, 1, 8, device="cuda", generator=g)
    dy = (torch.where(v < 0, -1.0, 1.0) * (0.25 + v.abs())).bfloat16()
    del v
    assert N > POOL_CAP > N // 2
    y = Device().pool2_fwd(x)
    dx = Device().pool2_bwd(dy, x)
    for lo, hi in ((0, N // 2), (N // 2, N)):
        part = Device().pool2_fwd(x[lo:hi])
        assert torch.equal(part.view(torch.int16), y[lo:hi].view(torch.int16)), "forward halves differ from the one call"
        part = Device().pool2_bwd(dy[lo:hi], x[lo:hi])
        assert torch.equal(part.view(torch.int16), dx[lo:hi].view(torch.int16)), "backward halves differ from the one call"
        del part
    c = E.Case("pool-over-cap", dtype="bf16")
    for lo in (POOL_CAP - 2048, N - 4096):
        s = slice(lo, lo + 4096)
        E.check_pool_outputs(y[s], dx[s], x[s], dy[s], c, REP, "cuda")
    _finish(n0)


def test_refusals():
    t = torch.zeros(1 << 12, device="cuda")
    tl = torch.zeros(1 << 11, dtype=torch.int64, device="cuda")
    table = E.refusal_table(t, tl)
    for name, args, want in table:
        assert _lib.call_status(name, *args) == want, (name, want)
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(tl.any()), "a refused call launched something"


# ------------------------------------------------------------------------ the autograd Functions of msml_amd.functional
def _leaf(t, grad=True):
    return t.detach().clone().requires_grad_(grad)


def test_functional_fm_family():
    n0 = len(REP.failures)
    c = E.Case("functional", dtype="f32")
    g = torch.Generator().manual_seed(21)
    shape = (2, 3, 4, 8)
    x, y, d = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    # _FmFuse: tanh, mul
    xa, ya = _leaf(x), _leaf(y)
    z = FN._FmFuse.apply(xa, ya, E.TANH, E.MUL)
    z.backward(d)
    (zr, bz), (dxr, bdx), (dyr, bdy) = E.fuse_reference(x.double(), y.double(), d.double(), E.TANH, E.MUL, E.U32)
    REP.check("functional._FmFuse", "z", z.detach(), zr, bz, c)
    REP.check("functional._FmFuse", "dx", xa.grad, dxr, bdx, c)
    REP.check("functional._FmFuse", "dyf", ya.grad, dyr, bdy, c)
    # _FmAct: sigmoid
    xa = _leaf(x)
    m = FN._FmAct.apply(xa, E.SIGMOID)
    m.backward(d)
    mr, dm, gp, dgp = E.act_terms(x.double(), E.SIGMOID)
    REP.check("functional._FmAct", "m", m.detach(), mr, dm + E.U32 * mr, c)
    REP.check("functional._FmAct", "dx", xa.grad, d.double() * gp, d.double().abs() * dgp + 2 * E.U32 * (d.double() * gp).abs(), c)
    # _Mul: the second operand needs no gradient (db == NULL)
    xa, yb = _leaf(x), _leaf(y, False)
    o = FN._Mul.apply(xa, yb)
    o.backward(d)
    REP.check("functional._Mul", "out", o.detach(), x.double() * y.double(), 2 * E.U32 * (x.double() * y.double()).abs() + E.FLT_MIN, c)
    REP.check("functional._Mul", "da", xa.grad, d.double() * y.double(), 2 * E.U32 * (d.double() * y.double()).abs() + E.FLT_MIN, c)
    assert yb.grad is None
    # _Axpb: 1 - x
    xa = _leaf(x)
    o = FN._Axpb.apply(xa, -1.0, 1.0)
    o.backward(d)
    REP.check("functional._Axpb", "y", o.detach(), 1.0 - x.double(), 3 * E.U32 * (1.0 + x.double().abs()), c)
    REP.exact("functional._Axpb", "dx", xa.grad, -d, c)
    # _Mse: pad channels zero, count the real elements, upstream gradient 0.37, the target needs no gradient (db == NULL)
    a, b = x.clone(), y.clone()
    a[..., 5:], b[..., 5:] = 0.0, 0.0
    aa, bb = _leaf(a), _leaf(b, False)
    count = 2 * 3 * 4 * 5
    loss = FN._Mse.apply(aa, bb, count)
    (loss * 0.37).backward()
    a64 = _leaf(a.double()[..., :5])
    lr = torch.nn.MSELoss()(a64, b.double()[..., :5])
    (lr * E.f32(0.37)).backward()
    REP.check("functional._Mse", "loss", loss.detach(), lr.detach(), 13 * E.U32 * lr.detach(), c)
    REP.check("functional._Mse", "da", aa.grad[..., :5], a64.grad, 6 * E.U32 * a64.grad.abs() + E.FLT_MIN, c)
    REP.exact("functional._Mse", "da pad channels", aa.grad[..., 5:], torch.zeros(2, 3, 4, 3).cuda(), c)
    assert bb.grad is None
    # _Dropout: forward and backward share the mask
    xa = _leaf(x)
    o = FN._Dropout.apply(xa, 0.4, 123)
    o.backward(d)
    keep = E.keep_mask(123, x.numel(), 0.4).view(shape).cuda()
    REP.exact("functional._Dropout", "keep mask", o.detach() != 0, keep & (x != 0), c)
    REP.exact("functional._Dropout", "dx", xa.grad, Device().dropout(d, 0.4, 123), c)
    sc = 1.0 / (1.0 - E.f32(0.4))
    REP.check("functional._Dropout", "y", o.detach(), torch.where(keep, x.double() * sc, torch.zeros(()).double().cuda()),
              4 * E.U32 * (x.double() * sc).abs(), c)
    _finish(n0)


def test_functional_dap_segloss_pool2():
    n0 = len(REP.failures)
    c = E.Case("functional", dtype="f32")
    g = torch.Generator().manual_seed(22)
    # _Dap
    x = torch.randn(2, 5, 7, 24, generator=g)
    x[..., 18:] = 0.0
    dseg = torch.randn(2, 2, 5, 7, generator=g)
    xa = _leaf(x.cuda())
    seg = FN._Dap.apply(xa)
    seg.backward(dseg.cuda())
    x64 = _leaf(x.double())
    from oracle.model import dap
    sr = dap(x64[..., :18].permute(0, 3, 1, 2))
    sr.backward(dseg.double())
    mag = dap(x.double().abs()[..., :18].permute(0, 3, 1, 2))
    REP.check("functional._Dap", "seg", seg.detach().cpu(), sr.detach(), 9 * E.U32 * mag, c)
    REP.check("functional._Dap", "dx", xa.grad.cpu(), x64.grad, 2 * E.U32 * x64.grad.abs() + E.FLT_MIN, c)
    # _SegLoss through seg_consensus_loss, upstream gradient 0.37
    sc = [s for s in E.seg_cases() if (s.N, s.H, s.W) == (3, 8, 8) and not s.mean_all and not s.kl_all][0]
    logit, msk = E.draw_seg(sc)
    la = _leaf(logit.cuda())
    loss = FN.seg_consensus_loss(la, msk.cuda(), sc.ab[0], sc.ab[1])
    (loss * 0.37).backward()
    ref, dref = E.seg_reference(logit, msk, E.f32(sc.ab[0]), E.f32(sc.ab[1]), 0, 0)
    dloss, dd, _ = E.seg_budget(logit, msk, E.f32(sc.ab[0]), E.f32(sc.ab[1]), 0, 0)
    k = E.f32(0.37)
    REP.check("functional._SegLoss", "loss", loss.detach().cpu(), ref, dloss + E.U32 * ref.abs(), c)
    REP.check("functional._SegLoss", "dlogit", la.grad.cpu(), k * dref, k * dd + E.U32 * (k * dref).abs(), c)     # dlogit * g: 1 op
    # _Pool2
    pc = [p for p in E.pool_cases() if (p.N, p.H, p.W, p.cp, p.dtype) == (3, 4, 4, 8, "f32")][0]
    x, dy = E.draw_pool(pc, "cuda")
    xa = _leaf(x)
    y = FN._Pool2.apply(xa)
    y.backward(dy)
    E.check_pool_outputs(y.detach(), xa.grad, x, dy, E.Case("functional._Pool2", dtype="f32"), REP, "cuda")
    _finish(n0)


def test_zz_report():
    print("\n" + REP.table())
    print("wall time of the file so far: %.0f s" % (time.time() - T0))
    assert not REP.failures, REP.failures[:10]
