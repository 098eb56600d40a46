"""The head, PartialFC and optimizer entry points (msml_amd/csrc/head.hip, msml_transpose, msml_gemm_splitk) through the C
ABI (msml_amd._lib.call) against the float64 references and the derived budgets of tests/head_cases.py (the same checks
tests/test_head_cpu.py runs on the torch restatement).  Memory hygiene without a sanitizer: every output lives between two
guard bands of a sentinel, outputs are pre-filled with NaN (an element the kernel does not write fails the comparison),
padded input columns hold NaN, every input is cloned before the call and compared after it.  Nothing here provokes a
fault: every shape is one the entry point documents as supported or must refuse on the host.

Outcome on an MI355X (worst error / budget, budgets already x SAFETY = 2): the table test_zz_report prints; the figures
of the run this file was written against are in docs/KERNELS.md, "Head, PartialFC and optimizer kernel tests"."""
import time

import pytest
import torch

from msml_amd import _lib
from tests import head_cases as H
from tests.abi_harness import DTC, GUARD, SENTINEL, GuardedDevice  # noqa: F401

pytestmark = pytest.mark.gpu
REP = H.Report()
T0 = time.time()
UNSUP, SHAPE, WORKSPACE = -4, -1, -5


def _offset_copy(t):
    """A copy of t whose base address is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


class Device(GuardedDevice):
    """The entry points with the interface of head_cases.Restatement."""

    def rownorm_fwd(self, wt, Rp, ld, dtype, misalign=False):
        R, E = wt.shape
        src = _offset_copy(wt) if misalign else wt
        dst, inv = self.out((Rp, ld), dtype), self.out((R,), torch.float32)
        self.call("msml_rownorm_fwd", src, R, Rp, E, dst, ld, inv, DTC[dtype])
        return dst, inv

    def rownorm_bwd(self, wt, inv, dy, E, accumulate, dw0):
        R = wt.shape[0]
        dw = self.out((R, E), torch.float32, dw0 if accumulate else None)
        self.call("msml_rownorm_bwd", wt, inv, dy, dy.shape[1], R, E, dw, accumulate)
        return dw

    def gather_target(self, cos, lab):
        o = self.out((cos.shape[0],), torch.float32)
        self.call("msml_gather_target", cos, cos.shape[1], lab, cos.shape[0], o)
        return o

    def margin_fwd(self, cos, lab, C, kind, s, m, a, k):
        o = self.out(tuple(cos.shape), torch.float32, cos)
        self.call("msml_margin_fwd", o, lab, cos.shape[0], C, cos.shape[1], kind, s, m, a, k)
        return o

    def margin_bwd(self, dlogit, lab, ct, C, ldo, kind, s, m, a, k, dtype):
        N = dlogit.shape[0]
        o = self.out((N, ldo), dtype)
        self.call("msml_margin_bwd", dlogit, dlogit.shape[1], lab, ct, N, C, o, ldo, kind, s, m, a, k, DTC[dtype])
        return o

    def pfc_rowstats(self, cos, C, lab, kind, s, m, a, k, misalign=False):
        N, ld = cos.shape
        src = _offset_copy(cos) if misalign else cos
        rm, rs = self.out((N,), torch.float32), self.out((N,), torch.float32)
        self.call("msml_pfc_rowstats", src, ld, N, C, lab, kind, s, m, a, k, rm, rs)
        return rm, rs

    def pfc_grad(self, cos, C, lab, kind, s, m, a, k, gmax, gsum, eps_ls, inv_n, ldo, dtype):
        N, ld = cos.shape
        o, pt = self.out((N, ldo), dtype), self.out((N,), torch.float32)
        self.call("msml_pfc_grad", cos, ld, N, C, lab, kind, s, m, a, k, gmax, gsum, eps_ls, inv_n, o, ldo, pt, DTC[dtype])
        return o, pt

    def transpose(self, src, C, ld_d, dtype):
        R, ld_s = src.shape
        full = self.out((2 * H.GUARD_ROWS + C, ld_d), dtype, 7.0)
        self.call("msml_transpose", src, R, C, ld_s, full[H.GUARD_ROWS:], ld_d, DTC[dtype])
        return full

    def gemm_splitk(self, a, wp):
        M, K = a.shape
        need = _lib.value("msml_gemm_splitk_workspace", M, wp.shape[0], K)
        ws = self.out((need // 4,), torch.float32)
        o = self.out((M, wp.shape[0]), torch.float32)
        self.call("msml_gemm_splitk", a, M, K, wp, wp.shape[0], o, wp.shape[0], ws, need, _lib.BF16)
        return o

    def sgd(self, wt, grad, buf, lr, mu, wd, first, coef, dev=False):
        n = wt.numel()
        w2 = self.out((n,), torch.float32, wt)
        b2 = self.out((n,), torch.float32, float("nan") if first else buf)      # a first step must not read the buffer
        if dev:
            assert not first
            self.call("msml_sgd_momentum_dev", w2, grad, b2, n, torch.tensor([lr], device="cuda"), mu, wd, coef)
        else:
            self.call("msml_sgd_momentum", w2, grad, b2, n, lr, mu, wd, first, coef)
        return w2, b2

    def grad_norm_clip(self, g, max_norm, scale):
        n = g.numel()
        rows = H.sumsq_rows(n)
        ws, o = self.out((rows,), torch.float32), self.out((2,), torch.float32)
        if scale == 1.0:
            self.call("msml_grad_norm_clip", g, n, max_norm, o, ws, rows)
        else:
            self.call("msml_grad_norm_clip_scaled", g, n, max_norm, scale, o, ws, rows)
        return o


def _finish(n0):
    new = REP.failures[n0:]
    assert not new, new[:10]


def _status(name, *args):
    rc, is_status = _lib._invoke(name, args)
    assert is_status
    return rc


def test_rownorm():
    n0 = len(REP.failures)
    for c in H.rownorm_cases():
        H.check_rownorm_case(Device(), c, REP, "cuda")
    _finish(n0)


def test_margin_gather_and_pfc_grad():
    n0 = len(REP.failures)
    planted = excused = 0
    for c in H.margin_cases():
        p, e = H.check_margin_case(Device(), c, REP, "cuda")
        planted, excused = planted + p, excused + e
        if c.C > 1:
            p, e = H.check_pfc_grad_case(Device(), c, REP, "cuda")
            planted, excused = planted + p, excused + e
        if c.N * c.ld > 1 << 20:
            torch.cuda.empty_cache()
    print("\nplanted targets with |c| == 1: %d, backward elements excused: %d" % (planted, excused))
    assert planted > 0 and excused == planted
    _finish(n0)


def test_pfc_rowstats():
    n0 = len(REP.failures)
    count = {"target_is_max": 0, "target_not_max": 0}
    for c in H.rowstats_cases():
        H.check_rowstats_case(Device(), c, REP, "cuda", count=count)
    print("\nrows whose target is / is not the row max:", count)
    assert count["target_is_max"] > 0 and count["target_not_max"] > 0
    _finish(n0)


def test_transpose():
    n0 = len(REP.failures)
    for R, C in H.TRANSPOSE_SHAPES:
        for dt in ("f32", "bf16"):
            for ld_d in sorted({R, H.kpad(R)}):
                H.check_transpose(Device(), R, C, C + 3, ld_d, dt, REP, "cuda")
    _finish(n0)


def test_gemm_splitk():
    n0 = len(REP.failures)
    for M, K in H.GEMM_SHAPES:
        H.check_gemm(Device(), M, K, REP, "cuda")
    _finish(n0)
    t = torch.zeros(1 << 16, device="cuda", dtype=torch.bfloat16)
    o = torch.zeros(32 * 512, device="cuda")
    need = _lib.value("msml_gemm_splitk_workspace", 32, 512, 2048)
    assert need > 0
    assert _status("msml_gemm_splitk", t, 32, 2048, t, 512, o, 512, o, need - 1, _lib.BF16) == WORKSPACE
    assert _status("msml_gemm_splitk", t, 32, 2048, t, 512, o, 512, o, need, _lib.F32) == UNSUP
    torch.cuda.synchronize()
    assert not bool(o.any()), "a refused call launched something"


def test_sgd_momentum():
    n0 = len(REP.failures)
    for n in H.SGD_NS:
        for v in H.SGD_VARIANTS:
            w2, b2 = H.check_sgd(Device(), n, v, REP, "cuda")
            if not v[0]:          # the device-lr entry on the same operands: the same bits
                c = H.Case("sgd-n%d-first%d-mu%g-wd%g-coef%s" % (n, v[0], v[1], v[2], v[3]))
                g = c.gen()
                wt, grad, buf = (torch.randn(n, generator=g).cuda() for _ in range(3))
                coef = None if v[3] is None else torch.tensor([v[3]], device="cuda")
                w3, b3 = Device().sgd(wt, grad, buf, H.f32(0.1), H.f32(v[1]), H.f32(v[2]), 0, coef, dev=True)
                assert torch.equal(w3, w2) and torch.equal(b3, b2), ("sgd_momentum_dev differs", n, v)
    _finish(n0)
    t = torch.zeros(64, device="cuda")
    keep = t.clone()
    for args in ((t[1:], t, t), (t, t[1:], t), (t, t, t[1:])):
        assert _status("msml_sgd_momentum", *args, 16, 0.1, 0.9, 0.0, 0, None) == SHAPE
        assert _status("msml_sgd_momentum_dev", *args, 16, t, 0.9, 0.0, None) == SHAPE
    torch.cuda.synchronize()
    assert torch.equal(t, keep)


def test_grad_norm_clip():
    n0 = len(REP.failures)
    for n in H.NORM_NS:
        for above in (False, True):
            for scale in (1.0, 0.25):
                a = H.check_norm_clip(Device(), n, above, scale, REP, "cuda")
                b = H.check_norm_clip(Device(), n, above, scale, H.Report(), "cuda")
                assert torch.equal(a, b), ("two runs differ", n, above, scale)
    _finish(n0)
    g = torch.ones(4096, device="cuda")
    o, ws = torch.zeros(2, device="cuda"), torch.zeros(16, device="cuda")
    assert _status("msml_grad_norm_clip", g, 4096, 1.0, o, ws, 15) == WORKSPACE
    assert _status("msml_grad_norm_clip_scaled", g, 4096, 1.0, 0.5, o, ws, 15) == WORKSPACE
    assert _status("msml_grad_norm_clip_scaled", g, 4096, 1.0, 0.0, o, ws, 16) == SHAPE
    assert _status("msml_grad_norm_clip_scaled", g, 4096, 1.0, -1.0, o, ws, 16) == SHAPE
    assert _status("msml_grad_norm_clip", g[1:], 4095, 1.0, o, ws, 16) == SHAPE
    torch.cuda.synchronize()
    assert not bool(o.any()) and not bool(ws.any()), "a refused call launched something"


def test_pfc_refusals():
    t = torch.zeros(1 << 12, device="cuda")
    lab = torch.zeros(8, dtype=torch.int64, device="cuda")
    keep = t.clone()
    tail = (lab, 0, 64.0, 0.5, 0.0, 0.0)
    for dt in (_lib.F32, _lib.BF16):
        assert _status("msml_pfc_grad", t, 32, 8, 1, *tail, t, t, 0.1, 0.125, t, 32, t, dt) == SHAPE          # C == 1
        assert _status("msml_pfc_grad", t, 31, 8, 32, *tail, t, t, 0.1, 0.125, t, 32, t, dt) == SHAPE         # ld < C
        assert _status("msml_pfc_grad", t, 32, 8, 32, *tail, t, t, 0.1, 0.125, t, 31, t, dt) == SHAPE         # ldo < C
        assert _status("msml_margin_bwd", t, 31, lab, t, 8, 32, t, 32, 0, 64.0, 0.5, 0.0, 0.0, dt) == SHAPE   # ldg < C
    assert _status("msml_margin_fwd", t, lab, 8, 32, 31, 0, 64.0, 0.5, 0.0, 0.0) == SHAPE
    assert _status("msml_margin_fwd", t, lab, 8, 32, 32, 2, 64.0, 0.5, 0.0, 0.0) == SHAPE                     # unknown kind
    assert _status("msml_pfc_rowstats", t, 31, 8, 32, *tail, t, t) == SHAPE
    assert _status("msml_rownorm_fwd", t, 4, 4, 64, t, 63, t, _lib.F32) == SHAPE
    assert _status("msml_transpose", t, 8, 8, 7, t, 8, _lib.F32) == SHAPE
    torch.cuda.synchronize()
    assert torch.equal(t, keep), "a refused call launched something"


def test_zz_report():
    print("\n" + REP.table())
    print("wall time of the file so far: %.0f s" % (time.time() - T0))
    assert not REP.failures, REP.failures[:10]
