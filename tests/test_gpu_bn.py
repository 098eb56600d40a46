"""Every entry point of msml_amd/csrc/bn.hip through the C ABI (msml_amd._lib.call), f32 and bf16, against the float64
reference and the derived budgets of tests/bn_cases.py (the same checks tests/test_bn_cpu.py runs on the torch restatement).
Memory hygiene without a sanitizer: every output lives between two guard bands of a sentinel, outputs are pre-filled with
NaN (an element the kernel does not write fails the comparison), every input is cloned before the call and compared
after it.  Nothing here provokes a fault: every shape is one the entry point documents as supported or must refuse on
the host.

Outcome on an MI355X (worst error / budget, budgets already x SAFETY = 2): see the table test_zz_report prints; the
figures of the run this file was written against are in DESIGN.md, "BatchNorm kernel tests"."""
import time

import pytest
import torch

from msml_amd import _lib
from tests import bn_cases as B
from tests.abi_harness import DTC, GUARD, SENTINEL, GuardedDevice  # noqa: F401

pytestmark = pytest.mark.gpu
REP = B.Report()          # one report for the whole file: test_zz_report (last in file order) prints its table
T0 = time.time()


class Device(GuardedDevice):
    """The entry points of bn.hip with the interface of bn_cases.Restatement."""

    def __init__(self):
        super().__init__()
        self.npart = None         # next_partial rows of the last bwd_apply (row protocol)

    # ---- statistics
    def stat_rows(self, x):
        M, C = x.shape
        part = self.out((B.stats_rows(M, C), 2, C), torch.float32)
        self.call("msml_bn_stats", x, M, C, part, DTC[x.dtype])
        return part

    def stat_acc(self, x):
        M, C = x.shape
        acc = self.out((B.ACC_ROWS, 2, C), torch.float64, 0.0)
        self.call("msml_bn_stats_acc", x, M, C, acc, DTC[x.dtype])
        return acc

    def bn_train(self, x, gamma, beta, rmean, rvar, momentum, eps, proto="rows"):
        M, C = x.shape
        src = self.stat_rows(x) if proto == "rows" else self.stat_acc(x)
        coef = self.out((4, C), torch.float32)
        rm, rv = self.out((C,), torch.float32, rmean), self.out((C,), torch.float32, rvar)
        if proto == "rows":
            part = src
            self.call("msml_bn_finalize", part, part.shape[0], C, float(M), gamma, beta, rm, rv, momentum, eps, coef[0], coef[1],
                      coef[2], coef[3])
        else:
            y = self.out(tuple(x.shape), x.dtype)
            self.call("msml_bn_fin_act_fwd", src, float(M), gamma, beta, rm, rv, momentum, eps, coef[0], coef[1], coef[2],
                      coef[3], x, None, None, 0, y, M, C, None, DTC[x.dtype])
        rmean.copy_(rm)
        rvar.copy_(rv)
        return coef[0], coef[1], coef[2], coef[3]

    def finalize_eval(self, gamma, beta, rmean, rvar, eps):
        C = rmean.numel()
        coef = self.out((2, C), torch.float32)
        self.call("msml_bn_finalize", None, 0, C, 0.0, gamma, beta, rmean, rvar, 0.1, eps, coef[0], coef[1], None, None)
        return coef[0], coef[1]

    # ---- forward
    def act_fwd(self, x, scale, shift, alpha, res, res_first, emit=False, proto="rows"):
        M, C = x.shape
        y = self.out(tuple(x.shape), x.dtype)
        if not emit:
            self.call("msml_bn_act_fwd", x, scale, shift, alpha, res, int(res_first), y, M, C, DTC[x.dtype])
            return y, None
        st = self.out((B.ew_rows(M, C), 2, C), torch.float32)
        self.call("msml_bn_act_fwd_stats", x, scale, shift, alpha, res, int(res_first), y, M, C, st, DTC[x.dtype])
        assert bool(torch.isfinite(st).all()), "msml_bn_act_fwd_stats left a partial row unwritten"
        t = st.double().sum(0)
        return y, (t[0], t[1])

    def fin_act_fwd(self, x, gamma, beta, rmean, rvar, momentum, eps, alpha, res, res_first, emit):
        M, C = x.shape
        acc = self.stat_acc(x)
        coef = self.out((4, C), torch.float32)
        rm, rv = self.out((C,), torch.float32, rmean), self.out((C,), torch.float32, rvar)
        y = self.out(tuple(x.shape), x.dtype)
        ao = self.out((B.ACC_ROWS, 2, C), torch.float64, 0.0) if emit else None
        self.call("msml_bn_fin_act_fwd", acc, float(M), gamma, beta, rm, rv, momentum, eps, coef[0], coef[1], coef[2], coef[3],
                  x, alpha, res, int(res_first), y, M, C, ao, DTC[x.dtype])
        rmean.copy_(rm)
        rvar.copy_(rv)
        t = ao.sum(0) if emit else None
        return (coef[0], coef[1], coef[2], coef[3]), y, ((t[0], t[1]) if emit else None)

    # ---- backward.  grads = [dbeta, dgamma, dalpha] (None: null pointer), updated in place
    def _grads(self, grads, C):
        return [None if g is None else self.out((C,), torch.float32, g) for g in grads]

    @staticmethod
    def _back(grads, gs):
        for g, o in zip(grads, gs):
            if g is not None:
                g.copy_(o)

    def act_bwd(self, dy, x, scale, shift, alpha, mean, invstd, res, grads, accumulate, proto="rows", add=None):
        M, C = x.shape
        dx = self.out(tuple(x.shape), x.dtype)
        dres = self.out(tuple(x.shape), x.dtype) if res is not None else None
        gs = self._grads(grads, C)
        if proto == "rows":
            need = B.stats_rows(M, C) * 3 * C + 2 * C
            ws = self.out((need,), torch.float32)
            self.call("msml_bn_act_bwd", dy, x, scale, shift, alpha, mean, invstd, res, dx, dres, gs[1], gs[0], gs[2],
                      accumulate, M, C, ws, need, DTC[x.dtype])
        else:
            acc = self.out((B.ACC_ROWS, 3, C), torch.float64, 0.0)
            self.call("msml_bn_act_bwd_acc", dy, x, scale, shift, alpha, mean, invstd, res, add, dx, dres, gs[1], gs[0],
                      gs[2], accumulate, M, C, acc, DTC[x.dtype])
        self._back(grads, gs)
        return dx, dres

    def bwd_apply(self, dy, x, scale, shift, alpha, mean, invstd, pieces, grads, accumulate, add=None, add_hw=None,
                  nxt=None, proto="rows", res=None):
        M, C = x.shape
        dt = DTC[x.dtype]
        dx = self.out(tuple(x.shape), x.dtype)
        gs = self._grads(grads, C)
        nx, nm, ni = nxt if nxt is not None else (None, None, None)
        H, W = add_hw if add_hw is not None else (0, 0)
        dres, em = None, None
        if proto == "rows":
            rows = pieces.shape[0]
            cws = self.out((98 * C,), torch.float32)
            npart = self.out((_lib.value("msml_bn_act_bwd_apply_rows", M, C), 3, C), torch.float32) if nxt is not None else None
            head = (dy, x, scale, shift, alpha, mean, invstd, pieces, rows, add)
            tail = (dx, gs[1], gs[0], gs[2], accumulate, M, C, cws)
            if nxt is None and add_hw is None:
                self.call("msml_bn_act_bwd_apply", *head, *tail, dt)
            elif nxt is None:
                self.call("msml_bn_act_bwd_apply_s2", *head, H, W, *tail, dt)
            elif add_hw is None:
                self.call("msml_bn_act_bwd_apply_next", *head, *tail, nx, nm, ni, npart, dt)
            else:
                self.call("msml_bn_act_bwd_apply_next_s2", *head, H, W, *tail, nx, nm, ni, npart, dt)
            if nxt is not None:
                assert bool(torch.isfinite(npart).all()) and bool((npart[:, 2] == 0).all()), "next_partial rows"
                self.npart = npart
                t = npart.double().sum(0)
                em = (t[0], t[1])
        else:
            acc = pieces.double().contiguous()
            dres = self.out(tuple(x.shape), x.dtype) if res is not None else None
            nacc = self.out((B.ACC_ROWS, 3, C), torch.float64, 0.0) if nxt is not None else None
            self.call("msml_bn_fin_bwd_apply", dy, x, scale, shift, alpha, mean, invstd, acc, res, add, H, W, dx, dres, gs[1],
                      gs[0], gs[2], accumulate, M, C, nx, nm, ni, nacc, dt)
            if nxt is not None:
                t = nacc.sum(0)
                em = (t[0], t[1])
        self._back(grads, gs)
        return dx, dres, em

    def bias_grad(self, dy, creal, db, accumulate):
        M, C = dy.shape
        need = B.stats_rows(M, C) * 2 * C
        ws = self.out((need,), torch.float32)
        o = self.out((creal,), torch.float32, db)
        self.call("msml_bias_grad", dy, M, C, creal, o, accumulate, ws, need, DTC[dy.dtype])
        db.copy_(o)

    def add(self, a, b, in_place=False):
        o = self.out(tuple(a.shape), a.dtype, a if in_place else None)
        self.call("msml_add", o if in_place else a, b, o, a.numel(), DTC[a.dtype])
        return o


def _finish(rep, n0):
    new = rep.failures[n0:]
    assert not new, new[:10]


def test_reduce_entry_points():
    n0 = len(REP.failures)
    for c in B.case_table("reduce"):
        assert B.slab_geometry_ok(c), c.name
        B.check_reduce_case(Device(), c, REP, "cuda")
    _finish(REP, n0)


def test_apply_entry_points():
    n0 = len(REP.failures)
    for c in B.case_table("apply") + B.case_table("big"):
        B.check_apply_case(Device(), c, REP, "cuda")
        torch.cuda.empty_cache()
    _finish(REP, n0)


def test_bwd_apply_family_given_rows():
    n0 = len(REP.failures)
    for c in B.case_table("rows"):
        B.check_rows_case(Device(), c, REP, "cuda")
    _finish(REP, n0)


def test_lattice_is_exact():
    n0 = len(REP.failures)
    zeros = []
    for c in B.case_table("lattice"):
        zeros.append(B.check_lattice_fwd(Device(), c, REP, "cuda"))
        B.check_rows_case(Device(), c, REP, "cuda")
    assert min(z for z in zeros if z is not None) > 0.02
    _finish(REP, n0)


@pytest.mark.parametrize("N,H,W", [(((1 << 24) - 1) // (B.S2_MOST_FIXUPS[0] * B.S2_MOST_FIXUPS[1]),) + B.S2_MOST_FIXUPS,
                                   (5, 1831, 1831)])
def test_stride2_add_just_under_2_24_pixels(N, H, W):
    """The float-reciprocal pixel decode at the largest M it is allowed: bn_cases.S2_MOST_FIXUPS is the (H, W) of
    bn_cases.S2_SHAPES with the most fix-ups taken (tests/test_bn_cpu.py runs the scan and asserts the choice),
    1831 x 1831 the largest odd square map."""
    M, C = N * H * W, 8
    assert M < 1 << 24 and M + H * W >= 1 << 24
    case = B.Case("s2-2^24-%dx%d" % (H, W), M, C, "bf16", False, False, False, True, "normal", 8, "s2big")
    g = torch.Generator(device="cuda").manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x, dy = rn(M, C).bfloat16(), rn(M, C).bfloat16()
    compact = rn(N * ((H + 1) // 2) * ((W + 1) // 2), C).bfloat16()
    sc, sh, mean, inv = 1.0 + 0.5 * rn(C), 0.5 * rn(C), 0.1 * rn(C), 1.0 + 0.1 * rn(C).abs()
    ref0 = B.bwd_reference(dy, x, sc, sh, None, mean, inv, None, torch.bfloat16, 1)
    gen = torch.Generator().manual_seed(6)
    ps = [B.split_rows(t, 8, gen) for t in (ref0["dbeta"], ref0["dgamma"], ref0["dalpha"])]
    pieces = torch.stack([p[0] for p in ps], 1).cuda()
    sums = [p[1].cuda() for p in ps]
    dsums = [B.rows_fold_budget(p[0]).cuda() for p in ps]
    del ref0
    br = B.bwd_reference(dy, x, sc, sh, None, mean, inv, None, torch.bfloat16, 1, sums=sums, dsums=dsums,
                         add=B.scatter_s2(compact, N, H, W))
    n0 = len(REP.failures)
    for proto in ("rows", "acc"):
        grads = [torch.zeros(C, device="cuda") for _ in range(3)]
        dx, _, _ = Device().bwd_apply(dy, x, sc, sh, None, mean, inv, pieces, grads, 0, add=compact, add_hw=(H, W), proto=proto)
        REP.check("bn_act_bwd_apply_s2" if proto == "rows" else "bn_fin_bwd_apply_s2", "dx", dx, br["dx"], br["dx_budget"], case)
    _finish(REP, n0)


def test_add():
    n0 = len(REP.failures)
    for dt in ("f32", "bf16"):
        for n in (8, 8 * 255, 8 * (768 * 256 + 5), 8 * (3 * 768 * 256 - 1)):      # n / 8 not a multiple of the grid
            case = B.Case("add-n%d-%s" % (n, dt), n // 8, 8, dt, False, False, False, False, "normal", None, "add")
            d = B.draw(case, "cuda")
            ref = d["x"].double() + d["dy"].double()
            for in_place in (False, True):        # the residual joins of the backward add into their first operand
                o = Device().add(d["x"], d["dy"], in_place)
                REP.check("add", "out" + " in place" * in_place, o, ref, B.U32 * ref.abs() + B.u_store(B.DT[dt]) * ref.abs(),
                          case)                   # a + b: 1 op
    _finish(REP, n0)


def test_two_runs_bit_identical_and_protocols_agree():
    """Row-protocol entry points are deterministic; the accumulator protocol's f64 totals equal the fixed-order f64 total
    of the row protocol exactly (docs/KERNELS.md: an f64 sum of f32 partials is exact, hence order-free).  From equal
    totals the two protocols run the same device functions (bn_coef, bn_fwd_stream, bn_bwd_stream: csrc/bn.hip,
    csrc/common.h), so coefficients, running statistics, y, dx and dres are the same bits too."""
    for c in [c for c in B.case_table("apply") if c.tag in ("row+1", "rows512", "rows513", "capped", "offset30")] + \
            B.case_table("big")[:2]:
        d = B.draw(c, "cuda")
        x, M, C = d["x"], c.M, c.C
        be = Device()
        p1, p2 = be.stat_rows(x), be.stat_rows(x)
        assert torch.equal(p1, p2), c.name
        acc = be.stat_acc(x)
        assert torch.equal(acc.sum(0), p1.double().sum(0)), "bn_stats_acc total != row total: %s" % c.name
        eps, mom = B.f32(B.EPS), B.f32(0.1)
        rm1, rv1 = d["rmean0"].clone(), d["rvar0"].clone()
        sc, sh, mean, inv = be.bn_train(x, d["gamma"], d["beta"], rm1, rv1, mom, eps)
        rf = int(c.res_first and c.residual)
        (y1, e1), (y2, e2) = (be.act_fwd(x, sc, sh, d["alpha"], d["res"], rf, emit=True) for _ in range(2))
        assert torch.equal(y1.view(torch.uint8), y2.view(torch.uint8)) and torch.equal(e1[0], e2[0]) and torch.equal(e1[1], e2[1])
        rm2, rv2 = d["rmean0"].clone(), d["rvar0"].clone()
        coef2, ya, ea = be.fin_act_fwd(x, d["gamma"], d["beta"], rm2, rv2, mom, eps, d["alpha"], d["res"], rf, True)
        # one coefficient rule (bn_coef / bn_running_update, common.h) on the same exact f64 totals, one forward loop
        for nm, a, b in zip(("scale", "shift", "mean", "invstd", "running_mean", "running_var"),
                            (sc, sh, mean, inv, rm1, rv1), tuple(coef2) + (rm2, rv2)):
            assert _same(a, b), "msml_bn_finalize and msml_bn_fin_act_fwd differ in %s: %s" % (nm, c.name)
        assert _same(y1, ya), "msml_bn_act_fwd and msml_bn_fin_act_fwd differ in y: %s" % c.name
        outs = []
        for proto in ("rows", "rows", "acc"):
            grads = [torch.zeros(C, device="cuda") for _ in range(3)]
            dx, dres = be.act_bwd(d["dy"], x, sc, sh, d["alpha"], mean, inv, d["res"] if rf else None, grads, 0, proto=proto)
            outs.append((dx, grads, dres))
        assert torch.equal(outs[0][0].view(torch.uint8), outs[1][0].view(torch.uint8))
        # one backward apply loop, k1 / k2 from the same exact totals
        assert _same(outs[0][0], outs[2][0]), "msml_bn_act_bwd and msml_bn_act_bwd_acc differ in dx: %s" % c.name
        assert _same(outs[0][2], outs[2][2]), "msml_bn_act_bwd and msml_bn_act_bwd_acc differ in dres: %s" % c.name
        for a, b in zip(outs[0][1], outs[1][1]):
            assert torch.equal(a, b)
        # same reduce kernel, exact f64 totals: the parameter gradients of the two protocols are the same f32 numbers
        for a, b in zip(outs[0][1], outs[2][1]):
            assert torch.equal(a, b), "accumulator protocol differs from the row protocol: %s" % c.name


def _bits(t):
    return None if t is None else t.contiguous().view(torch.uint8)


def _same(a, b):
    return (a is None and b is None) or torch.equal(_bits(a), _bits(b))


def test_every_row_protocol_entry_point_twice():
    """msml_bn_finalize, msml_bn_act_fwd, msml_bias_grad and msml_bn_act_bwd_apply / _next / _s2 / _next_s2 (below and above
    the k_fold_rows threshold) run twice on the same operands give the same bits: dx, the three gradients, next_partial."""
    import zlib
    for c in [c for c in B.case_table("rows") if c.rows in (32, 513, 5000) and c.C in (64, 256)]:
        d = B.draw(c, "cuda")
        x, M, C = d["x"], c.M, c.C
        eps, mom = B.f32(B.EPS), B.f32(0.1)
        runs = []
        for _ in range(2):
            be = Device()
            rm, rv = d["rmean0"].clone(), d["rvar0"].clone()
            coef = be.bn_train(x, d["gamma"], d["beta"], rm, rv, mom, eps)
            y, _ = be.act_fwd(x, coef[0], coef[1], d["alpha"], d["res"], 0)
            db = torch.zeros(C, device="cuda")
            be.bias_grad(d["dy"], C, db, 0)
            runs.append(list(coef) + [rm, rv, y, db])
        sc, sh, mean, inv = runs[0][:4]
        for a, b in zip(*runs):
            assert _same(a, b), c.name
        gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + 2)
        pieces = torch.randn(c.rows, 3, C, generator=gen).cuda()
        H, W = B._hw_of(M)
        compact = d["add"][:(M // (H * W)) * ((H + 1) // 2) * ((W + 1) // 2)].contiguous()
        for nxt_on in (False, True):
            for addkind in ("none", "dense", "s2"):
                outs = []
                for _ in range(2):
                    be = Device()
                    grads = [torch.zeros(C, device="cuda") for _ in range(3)]
                    dx, _, _ = be.bwd_apply(d["dy"], x, sc, sh, d["alpha"], mean, inv, pieces, grads, 0,
                                            add={"none": None, "dense": d["add"], "s2": compact}[addkind],
                                            add_hw=(H, W) if addkind == "s2" else None,
                                            nxt=(d["nx"], d["nmean"], d["ninvstd"]) if nxt_on else None)
                    outs.append([dx, be.npart] + grads)
                for a, b in zip(*outs):
                    assert _same(a, b), (c.name, nxt_on, addkind)


UNSUP, SHAPE, WORKSPACE = -4, -1, -5


def _status(name, *args):
    rc, is_status = _lib._invoke(name, args)
    assert is_status
    return rc


def refusal_calls(t, C, M=64, dt=_lib.F32):
    """(name, args) of every entry point with an apply loop; t: any tensor large enough (a refusing call never touches it)."""
    co = (t, t, t, t, t)            # scale, shift, alpha, mean, invstd
    return [
        ("msml_bn_act_fwd", (t, t, t, t, None, 0, t, M, C, dt)),
        ("msml_bn_act_fwd_stats", (t, t, t, t, None, 0, t, M, C, t, dt)),
        ("msml_bn_fin_act_fwd", (t, float(M), t, t, t, t, 0.1, 1e-5, t, t, t, t, t, t, None, 0, t, M, C, None, dt)),
        ("msml_bn_act_bwd", (t, t, *co, None, t, None, t, t, t, 0, M, C, t, 1 << 40, dt)),
        ("msml_bn_act_bwd_acc", (t, t, *co, None, None, t, None, t, t, t, 0, M, C, t, dt)),
        ("msml_bn_act_bwd_apply", (t, t, *co, t, 4, None, t, t, t, t, 0, M, C, t, dt)),
        ("msml_bn_act_bwd_apply_s2", (t, t, *co, t, 4, t, 2, 2, t, t, t, t, 0, M, C, t, dt)),
        ("msml_bn_act_bwd_apply_next", (t, t, *co, t, 4, None, t, t, t, t, 0, M, C, t, t, t, t, t, dt)),
        ("msml_bn_act_bwd_apply_next_s2", (t, t, *co, t, 4, t, 2, 2, t, t, t, t, 0, M, C, t, t, t, t, t, dt)),
        ("msml_bn_fin_bwd_apply", (t, t, *co, t, None, None, 0, 0, t, None, t, t, t, 0, M, C, None, None, None, None, dt)),
    ]


def test_refusals():
    t = torch.zeros(1 << 16, device="cuda")
    keep = t.clone()
    for C in B.CS_REDUCE_ONLY:
        for name, args in refusal_calls(t, C):
            assert _status(name, *args) == UNSUP, (name, C)
    M, C, dt = 64, 64, _lib.F32
    co = (t, t, t, t, t)
    for name, args, want in [
        # (M >= 2^24 with a stride-2 add is refused too: probed on host pointers only, tests/test_abi.py, where a
        # regression cannot launch over buffers this small)
        ("msml_bn_act_bwd_apply_s2", (t, t, *co, t, 4, t, 3, 3, t, t, t, t, 0, M, C, t, dt), SHAPE),               # M % (H W) != 0
        ("msml_bn_fin_bwd_apply", (t, t, *co, t, None, t, 3, 3, t, None, t, t, t, 0, M, C, None, None, None, None, dt), SHAPE),
        ("msml_bn_act_bwd", (t, t, *co, None, t, None, t, t, t, 0, M, C, t, 3 * C + 2 * C - 1, dt), WORKSPACE),
        ("msml_bias_grad", (t, M, C, C, t, 0, t, 2 * C - 1, dt), WORKSPACE),
        ("msml_bn_stats", (None, M, C, t, dt), SHAPE),
        ("msml_bn_stats_acc", (t, M, C, None, dt), SHAPE),
        ("msml_bn_finalize", (None, 4, C, 64.0, None, None, None, None, 0.1, 1e-5, t, t, None, None), SHAPE),
        ("msml_bn_finalize", (None, 0, C, 0.0, None, None, None, None, 0.1, 1e-5, t, t, None, None), SHAPE),
        ("msml_bn_act_fwd", (None, t, t, None, None, 0, t, M, C, dt), SHAPE),
        ("msml_bn_act_bwd", (t, t, *co, None, None, None, t, t, t, 0, M, C, t, 1 << 40, dt), SHAPE),                # null dx
        ("msml_bn_act_bwd_apply_next", (t, t, *co, t, 4, None, t, t, t, t, 0, M, C, t, t, t, t, None, dt), SHAPE),
        ("msml_bn_fin_bwd_apply", (t, t, *co, t, None, None, 0, 0, t, None, t, t, t, 0, M, C, None, t, t, t, dt), SHAPE),
        ("msml_add", (t, t, None, 64, dt), SHAPE),
        ("msml_add", (t, t, t, 63, dt), SHAPE),
    ]:
        assert _status(name, *args) == want, (name, want)
    torch.cuda.synchronize()
    assert torch.equal(t, keep), "a refused call launched something"


def _module_case(C, cr, dtype, acc_stats):
    from msml_amd import functional as Fn, ops
    old = ops.ACC_STATS
    ops.ACC_STATS = acc_stats
    try:
        torch.manual_seed(11)
        N, H, W = 4, 14, 14
        M = N * H * W
        bn = torch.nn.BatchNorm2d(cr).cuda()
        pr = torch.nn.PReLU(cr).cuda()
        with torch.no_grad():
            bn.weight.copy_(1.0 + 0.5 * torch.randn(cr))
            bn.bias.copy_(0.5 * torch.randn(cr))
            pr.weight.copy_(0.25 + 0.1 * torch.randn(cr))
            bn.running_mean.copy_(0.3 * torch.randn(cr))
            bn.running_var.copy_(1.0 + torch.rand(cr))
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        x = torch.randn(N, H, W, C, device="cuda").to(dtype)
        r = torch.randn(N, H, W, C, device="cuda").to(dtype)
        dy = torch.randn(N, H, W, C, device="cuda").to(dtype)
        for t in (x, r, dy):
            t[..., cr:] = 0
        x.requires_grad_(True)
        r.requires_grad_(True)
        y = Fn.bn_act(x, None, bn, pr, r, True)
        y.backward(dy)
        case = B.Case("bn_act-C%d/%d-%s-acc%d" % (cr, C, dtype, acc_stats), M, C, "bf16" if dtype == torch.bfloat16 else "f32",
                      True, True, True, True, "normal", None, "module")
        f2 = lambda t: t.detach().reshape(M, C)[:, :cr]
        eps, mom = B.f32(bn.eps), B.f32(bn.momentum)
        ref = B.autograd_reference(f2(x), bn.weight.detach(), bn.bias.detach(), pr.weight.detach(), f2(r), True, f2(dy), rm0,
                                   rv0, mom, eps)
        st = B.stats_reference(f2(x))
        cf = B.coef_reference(st, bn.weight.detach(), bn.bias.detach(), rm0, rv0, mom, eps)
        chain = B.slab_chain(M, C, B.stats_rows(M, C))
        bud = B.coef_budget(st, cf, chain, mom, eps, rm0, rv0)
        fr = B.fwd_reference(f2(x), cf["scale"], cf["shift"], pr.weight.detach(), f2(r), 1, dtype, bud["scale"], bud["shift"])
        br = B.bwd_reference(f2(dy), f2(x), cf["scale"], cf["shift"], pr.weight.detach(), cf["mean"], cf["invstd"], f2(r), dtype,
                             chain, dcoef=bud)
        key = "functional.bn_act" if C == cr else "functional._bn_act_padded"
        n0 = len(REP.failures)
        REP.check(key, "y", f2(y), ref["y"], fr["y_budget"], case)
        REP.check(key, "running_mean", bn.running_mean, ref["rmean"], bud["rmean"], case)
        REP.check(key, "running_var", bn.running_var, ref["rvar"], bud["rvar"], case)
        REP.check(key, "dx", f2(x.grad), ref["dx"], br["dx_budget"], case)
        REP.check(key, "dres", f2(r.grad), ref["dres"], br["dres_budget"], case)
        REP.check(key, "dgamma", bn.weight.grad, ref["dgamma"], br["dgamma_budget"], case)
        REP.check(key, "dbeta", bn.bias.grad, ref["dbeta"], br["dbeta_budget"], case)
        REP.check(key, "dalpha", pr.weight.grad, ref["dalpha"], br["dalpha_budget"], case)
        if cr < C:
            assert not bool(y.detach()[..., cr:].any()) and not bool(x.grad[..., cr:].any()), "pad channels must stay exactly zero"
        _finish(REP, n0)
    finally:
        ops.ACC_STATS = old


# accumulator-mode statistics serve bf16 only (ops.acc_applies): f32 has one protocol
MODULE_CASES = [(torch.bfloat16, True), (torch.bfloat16, False), (torch.float32, False)]


@pytest.mark.parametrize("dtype,acc_stats", MODULE_CASES)
def test_functional_bn_act(dtype, acc_stats):
    _module_case(64, 64, dtype, acc_stats)


@pytest.mark.parametrize("dtype,acc_stats", MODULE_CASES)
def test_functional_bn_act_padded(dtype, acc_stats):
    _module_case(32, 24, dtype, acc_stats)


def test_zz_report():
    print("\n" + REP.table())
    print("elements within their own z budget of the PReLU kink (either branch accepted):", REP.ambiguous)
    print("wall time of the file so far: %.0f s" % (time.time() - T0))
    assert not REP.failures, REP.failures[:10]
