"""Input-image gradients on the MI355X: msml_stem_bwd_data through the C ABI against the float64 restatement and the
derived budget of tests/stem_bwd_cases.py (the checks tests/test_stem_bwd_cpu.py runs the mutants against), its refusals
and determinism, and x.grad of whole MSML steps against the reference's golden (tests/golden/g21_input_grad.npz, recorded
by tools/make_golden_input_grad.py): f32 within the bounds of the parameter gradients of tests/test_gpu_bn_eval_bwd.py,
bf16 stem by stem from the dy each stem's backward received, LightCNN, use_osb=False, pair_saliency, and no launch when the
image does not ask.  Memory hygiene as in tests/abi_harness.py.

Figures of the run this file was written against (MI355X): worst error / budget of the random-data cases 0.004 (bf16 dy)
and 0.004 (f32 dy), of the stems inside a bf16 step 0.002; f32 x.grad against the golden, norm-wise / worst element over
the picks: eval 2.9e-6 / 8.3e-6, train 4.1e-4 / 1.8e-3; bf16 x.grad against the f32 golden, norm-wise over the picks: eval
0.058, train 0.249 (bound: the frb_early bound of the same step's parameter gradients)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msml_amd import _lib, ops, synthetic, verification
from msml_amd.backbones import MSML
from msml_amd.tricks.consensus_loss import StructureConsensuLossFunction
from oracle.bf16_emul import param_group
from oracle.fill import fill_module
from oracle.inputs import eval_inputs
from tests import stem_bwd_cases as S
from tests.abi_harness import DTC, SENTINEL, GuardedDevice
from tests.helpers import assert_cs, bf16_tolerances, elem_err, load, pick, rel_err

pytestmark = pytest.mark.gpu
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
CASES = S.cases()
DTYPES = (torch.bfloat16, torch.float32)
NPICK = 4096
_REF = {}


def reference(case, dt, kind):
    """(dy, w on the host, dx and its magnitude in float64): computed once per (case, dtype, data kind), never changed."""
    key = (case, dt, kind)
    if key not in _REF:
        dy, w = (S.exact_data if kind == "exact" else S.random_data)(case, dt)
        d64, w64 = S.operands(dy, w)
        _REF[key] = (dy, w, S.adjoint_f64(d64, w64, case), S.adjoint_f64(d64, w64, case, absolute=True))
    return _REF[key]


def launch(dev, case, dy, w):
    p, q = S.out_size(case.H, case.R, case.stride), S.out_size(case.W, case.R, case.stride)
    dx = dev.out((case.N, case.C, case.H, case.W), torch.float32)           # NaN: an element not written fails
    dev.call("msml_stem_bwd_data", dy, w, dx, case.N, case.C, case.H, case.W, p, q, case.Cout, case.ldy, case.R, case.R,
             case.stride, case.R // 2, DTC[dy.dtype])
    return dx


# ------------------------------------------------------------------------------------------- 1. the kernel, C ABI
@pytest.mark.parametrize("dt", DTYPES, ids=("bf16", "f32"))
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_exact_arithmetic(case, dt):
    dy, w, want, _ = reference(case, dt, "exact")
    got = launch(GuardedDevice(), case, dy.cuda(), w.cuda()).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, want), (float(np.abs(got - want).max()), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("dt", DTYPES, ids=("bf16", "f32"))
def test_random_data_against_f64(dt):
    worst = 0.0
    for case in CASES:
        dy, w, want, mag = reference(case, dt, "random")
        got = launch(GuardedDevice(), case, dy.cuda(), w.cuda()).cpu().numpy()
        ratio = S.worst_ratio(got, want, mag, case)
        print("   %-34s worst |err| / budget %.3f" % (S.case_id(case), ratio))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (case, ratio)
    print("stem_bwd_data %s dy: worst error / budget over %d cases %.3f" % (dt, len(CASES), worst))


def test_refusals_before_any_launch():
    dev = GuardedDevice()
    buf = torch.ones(1 << 16, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(1 << 14, device="cuda")

    def status(N=1, C=3, H=8, W=8, Cout=32, R=3, stride=1, null=None):
        dx = dev.out((4096,), torch.float32, 7.0)
        pad = R // 2
        p, q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        a = {"dy": buf, "w": w, "dx": dx}
        if null:
            a[null] = None
        rc = _lib.call_status("msml_stem_bwd_data", a["dy"], a["w"], a["dx"], N, C, H, W, p, q, Cout, Cout, R, R, stride, pad,
                              _lib.BF16)
        torch.cuda.synchronize()
        assert bool((dx == 7.0).all())
        for b, n in dev.bufs:
            assert bool((b[:64] == SENTINEL).all()) and bool((b[64 + n:] == SENTINEL).all())
        return rc

    assert status(W=129) == -1                           # MSML_ERR_SHAPE
    assert b"W <= 128" in _lib.load().msml_last_error()
    assert status(C=3, R=5) == -1                        # R*S*C = 75 > 32
    assert status(stride=3) == -1
    for name in ("dy", "w", "dx"):
        assert status(null=name) == -1
    with pytest.raises(RuntimeError, match="stem_bwd_data"):        # the Python side raises
        ops.stem_bwd_data(torch.zeros(1, 8, 129, 32, dtype=torch.bfloat16, device="cuda"),
                          torch.zeros(32, 3, 3, 3, device="cuda"), 1, 3, 8, 129, 3, 3, 1, 1)


@pytest.mark.parametrize("dt", DTYPES, ids=("bf16", "f32"))
def test_two_launches_give_equal_bits(dt):
    for case in (CASES[1], CASES[3], CASES[9]):
        dy, w, _, _ = reference(case, dt, "random")
        dy, w = dy.cuda(), w.cuda()
        a, b = launch(GuardedDevice(), case, dy, w), launch(GuardedDevice(), case, dy, w)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), case


# ------------------------------------------------------------------------------------------- 2. whole-model steps
def hip_msml(fp16=False, use_osb=True):
    torch.manual_seed(0)       # (use_osb=False: FMNone stages, as in the reference -- an FM operator needs the masks)
    m = MSML("iresnet18", "unet", (1, 1, 1, 1) if use_osb else (0, 0, 0, 0), 1000, fp16=fp16,
             fm_params=(3, 2, "sigmoid", "mul"), header_type="AMArcFace", header_params=(64.0, 0.48, 0.0, 0.0),
             peer_params=dict(PEER_OFF), use_osb=use_osb)
    return fill_module(m).cuda()


def hip_lightcnn(fp16=False, use_osb=True):
    torch.manual_seed(0)
    m = MSML("lightcnn", "unet", (1, 1, 1, 1) if use_osb else (0, 0, 0, 0), 1000, fp16=fp16,
             fm_params=(3, 2, "sigmoid", "mul"), header_type="Softmax", header_params=(64.0, 0.5, 0.0, 0.0),
             peer_params=dict(PEER_OFF), use_osb=use_osb)
    return fill_module(m).cuda()


def eval_step(m, x, seed=20):
    """m.eval(), loss = (feature * r).sum() with the recorder's seeded r; returns x (on the device, with .grad)."""
    m.eval()
    x = x.cuda().requires_grad_(True)
    feature = m(x)[0]
    r = torch.randn(x.shape[0], feature.shape[1], generator=torch.Generator().manual_seed(seed))
    loss = (feature.float() * r.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    return x, loss


def train_step(m, requires_grad=True):
    """m.train() with live BatchNorm, CE + consensus seg loss (the train/ record)."""
    x, msk = eval_inputs(4)
    label = synthetic.labels(4, 1000, seed=1)
    m.train()
    x = x.cuda().requires_grad_(requires_grad)
    final_cls, final_seg, kd = m(x, label.cuda(), None)
    loss = F.cross_entropy(final_cls.float(), label.cuda()) + \
        StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")(final_seg, msk.cuda(), msk.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return x, loss


def check_xgrad(x, g, prefix, elementwise=True):
    """The bounds check_picks of tests/test_gpu_bn_eval_bwd.py applies to the parameter gradients of such a record:
    norm-wise and worst single element below 1e-2, the checksum within the 1e-3 assert_cs is used with there.
    elementwise=False (LightCNN): the norm-wise bound alone, see test_golden_lightcnn_f32."""
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype is torch.float32
    got, got0 = pick(x.grad, NPICK), x.grad[0].cpu().numpy()
    e, ee = rel_err(got, g[prefix + "xgrad_pick"]), elem_err(got, g[prefix + "xgrad_pick"])
    e0, ee0 = rel_err(got0, g[prefix + "xgrad_img0"]), elem_err(got0, g[prefix + "xgrad_img0"])
    d0 = np.abs(got0.astype(np.float64) - g[prefix + "xgrad_img0"])
    frac = float((d0 > 1e-3 * np.abs(g[prefix + "xgrad_img0"]).max()).mean())
    print("%s x.grad: picks rel err %.3e (norm-wise) %.3e (element-wise); image 0 %.3e / %.3e, %.2e of its elements off by "
          "more than 1e-3 of the largest" % (prefix, e, ee, e0, ee0, frac))
    assert e < 1e-2 and e0 < 1e-2, (prefix, e, e0)
    if elementwise:
        assert ee < 1e-2 and ee0 < 1e-2, (prefix, ee, ee0)
        assert_cs(x.grad, g[prefix + "xgrad_cs"], 1e-3, prefix + "xgrad")


def test_golden_eval_f32():
    g = load("g21_input_grad.npz")
    x, loss = eval_step(hip_msml(), eval_inputs(4)[0])
    assert abs(loss.item() - g["eval/loss"]) < 1e-3 * abs(g["eval/loss"])
    check_xgrad(x, g, "eval/")


def test_golden_train_f32():
    g = load("g21_input_grad.npz")
    x, loss = train_step(hip_msml())
    assert abs(loss.item() - g["train/loss"]) < 1e-3 * abs(g["train/loss"])
    check_xgrad(x, g, "train/")


def test_golden_lightcnn_f32():
    """The LightCNN record (gray 128, eval loss).  mfm -- a max of two channels -- and the max pool route the gradient
    through the larger of their inputs: where two inputs lie within rounding of each other, two correct f32
    implementations take different routes, and single elements of x.grad then differ by their own size whatever the
    precision of the arithmetic.  The reference shows it against itself: its f32 map differs from its f64 map 13 times
    more in the worst element than norm-wise (lightcnn/ref_f64_err, recorded by the same tool).  So the bound here is
    the norm-wise 1e-2 of the other records, over the picks and over image 0; the element-wise figures are printed."""
    from tests.test_gpu_lightcnn import inputs
    g = load("g21_input_grad.npz")
    ref = g["lightcnn/ref_f64_err"]
    print("the reference's own f32 map against its f64 map: %.3e norm-wise, %.3e worst element" % (ref[0], ref[1]))
    assert ref[1] > 10 * ref[0]
    x, loss = eval_step(hip_lightcnn(), inputs(4)[0], seed=21)
    assert abs(loss.item() - g["lightcnn/loss"]) < 1e-3 * abs(g["lightcnn/loss"])
    check_xgrad(x, g, "lightcnn/", elementwise=False)


class Captured:
    """ops.stem_bwd_data recorded from the test: what each stem's backward handed the kernel, and what it returned."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = ops.stem_bwd_data

        def spy(dy, weight, n, c, h, w, r, s, stride, pad):
            dx = real(dy, weight, n, c, h, w, r, s, stride, pad)
            self.calls.append((dy.detach().clone(), weight.detach().clone(), (n, c, h, w, r, s, stride, pad), dx.clone()))
            return dx
        monkeypatch.setattr(ops, "stem_bwd_data", spy)

    def check_locally(self):
        """dx of every recorded call recomputed in float64 from the dy it received, against the derived budget."""
        worst = 0.0
        for dy, weight, (n, c, h, w, r, s, stride, pad), dx in self.calls:
            case = S.Case(n, c, h, w, r, stride, weight.shape[0], dy.shape[3])
            assert r == s and pad == r // 2
            d64, w64 = S.operands(dy.cpu(), weight.cpu().float())
            d64[..., case.Cout:] = 0.0                       # (never used by the restatement)
            want, mag = S.adjoint_f64(d64, w64, case), S.adjoint_f64(d64, w64, case, absolute=True)
            ratio = S.worst_ratio(dx.cpu().numpy(), want, mag, case)
            print("   stem %s: worst |err| / budget %.3f" % (S.case_id(case), ratio))
            assert ratio <= 1.0, (case, ratio)
            worst = max(worst, ratio)
        return worst


@pytest.mark.parametrize("record,side_streams", (("eval", False), ("train", False), ("train", True)),
                         ids=("eval", "train", "train_side_streams"))
def test_bf16_stems_locally_and_end_to_end(record, side_streams, monkeypatch):
    """side_streams: the OSB (and its stem's backward) on a stream of its own and the weight gradients on another, as
    bench.py runs the step -- the two stems' image gradients then come from two streams and autograd's sum joins them."""
    g = load("g21_input_grad.npz")
    cap = Captured(monkeypatch)
    m = hip_msml(fp16=True)
    if side_streams:
        ops.WGRAD_STREAM, ops.OSB_STREAM = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        x, _ = eval_step(m, eval_inputs(4)[0]) if record == "eval" else train_step(m)
        ops.wgrad_stream_join()
        torch.cuda.synchronize()
    finally:
        ops.WGRAD_STREAM = ops.OSB_STREAM = None
    # eval: the FRB stem only (the OSB's maps are detached); train: both stems, summed by autograd
    shapes = sorted(c[2][6] for c in cap.calls)
    assert shapes == ([1] if record == "eval" else [1, 2]), shapes
    assert all(c[0].dtype is torch.bfloat16 and c[0].shape[3] == 64 for c in cap.calls)
    cap.check_locally()
    total = cap.calls[0][3] if len(cap.calls) == 1 else cap.calls[0][3] + cap.calls[1][3]
    assert torch.equal(x.grad, total)
    assert bool(torch.isfinite(x.grad).all()) and all(float(x.grad[i].abs().max()) > 0 for i in range(4))
    e = rel_err(pick(x.grad, NPICK), g[record + "/xgrad_pick"])
    e0 = rel_err(x.grad[0].cpu().numpy(), g[record + "/xgrad_img0"])
    print("bf16 %s x.grad against the f32 golden, norm-wise: picks %.3e, image 0 %.3e" % (record, e, e0))
    if record == "train":
        # the step of tests/test_gpu_parity2.py::test_train_step_g4_bf16_fused_path[fill-4]; its bound for
        # frb.conv1.weight's gradient, which is computed from the same dy
        assert param_group("frb.conv1.weight") == "frb_early"
        tol = bf16_tolerances("ires18_b4_fill", cap=0.5)["frb_early"]
        assert e < tol and e0 < tol, (e, e0, tol)
    # (eval: no bf16 golden test bounds a parameter gradient of this record -- finiteness and nonzero maps above)


@pytest.mark.parametrize("fp16", (False, True), ids=("f32", "bf16"))
def test_lightcnn_and_no_osb(fp16, monkeypatch):
    from tests.test_gpu_lightcnn import inputs
    g = load("g21_input_grad.npz")
    cap = Captured(monkeypatch)
    for name, m, src in (("lightcnn", hip_lightcnn(fp16), inputs(4)[0]),
                         ("lightcnn, use_osb=False", hip_lightcnn(fp16, use_osb=False), inputs(4)[0]),
                         ("iresnet18, use_osb=False", hip_msml(fp16, use_osb=False), eval_inputs(4)[0])):
        x, _ = eval_step(m, src, seed=21 if "lightcnn" in name else 20)
        assert x.grad is not None and x.grad.shape == src.shape, name
        assert bool(torch.isfinite(x.grad).all()) and all(float(x.grad[i].abs().max()) > 0 for i in range(4)), name
        if name == "lightcnn":
            e = rel_err(pick(x.grad, NPICK), g["lightcnn/xgrad_pick"])
            print("lightcnn %s x.grad against the f32 golden, norm-wise: %.3e" % ("bf16" if fp16 else "f32", e))
    # the mfm stem's dz went to the kernel directly (5x5, 96 of 128 channels), in the storage type of the mode
    lc = [c for c in cap.calls if c[2][4] == 5]
    assert len(lc) == 2 and all(c[0].shape[3] == 128 and c[1].shape[0] == 96 for c in lc)
    assert all(c[0].dtype is (torch.bfloat16 if fp16 else torch.float32) for c in lc)
    assert len(cap.calls) == (3 if fp16 else 2)          # (the f32 IResNet stem is a conv over the NHWC image: to_nchw)
    cap.check_locally()


# ------------------------------------------------------------------------------------------- 3. no cost when unused
def _profiled_train_step(requires_grad):
    m = hip_msml(fp16=True)
    ops.PROFILE.start()
    try:
        x, _ = train_step(m, requires_grad)
    finally:
        recs = ops.PROFILE.stop()
    return m, x, recs


def test_no_launch_when_the_image_does_not_ask():
    m, x, recs = _profiled_train_step(False)
    assert x.grad is None and "stem_bwd_data" not in recs and recs
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    assert len(grads) > 100
    old = ops.NO_STEM_BWD_DATA
    ops.NO_STEM_BWD_DATA = True                          # what MSML_NO_STEM_BWD_DATA in the environment sets
    try:
        m2, _, recs2 = _profiled_train_step(False)
        assert {k: v["n"] for k, v in recs2.items()} == {k: v["n"] for k, v in recs.items()}      # the same launches
        for n, p in m2.named_parameters():
            if n in grads:
                assert torch.equal(p.grad, grads[n]), n
        with pytest.raises(RuntimeError, match="MSML_NO_STEM_BWD_DATA"):      # refused, not None
            train_step(hip_msml(fp16=True), True)
    finally:
        ops.NO_STEM_BWD_DATA = old
    m3, x3, recs3 = _profiled_train_step(True)
    assert recs3["stem_bwd_data"]["n"] == 2 and x3.grad is not None
    assert {k: v["n"] for k, v in recs3.items() if k != "stem_bwd_data"} == {k: v["n"] for k, v in recs.items()}
    for n, p in m3.named_parameters():                   # the weight-gradient path is untouched
        if n in grads:
            assert torch.equal(p.grad, grads[n]), n


# ------------------------------------------------------------------------------------------- 4. pair_saliency
def test_pair_saliency():
    m = hip_msml().eval()
    x, _ = eval_inputs(4)
    a, b = x.cuda(), x.flip(0).contiguous().cuda()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()                                            # the helper runs in eval mode and puts the mode back
    cos, da, db = verification.pair_saliency(m, a, b)
    assert m.training and all(mod.training for mod in m.modules())
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in state.items())          # BatchNorm state, bit for bit
    assert all(p.grad is None for p in m.parameters())
    m.eval()

    def cosine(p, q):
        with torch.no_grad():
            return F.cosine_similarity(m(p)[0].double(), m(q)[0].double(), dim=1)
    c0 = cosine(a, b)
    assert cos.shape == (4,) and da.shape == a.shape and db.shape == b.shape
    assert float((cos.double() - c0).abs().max()) < 1e-5
    # a forward difference along da: cos(a + t da) - cos(a) = t |da|^2 + O(t^2).  The step is sized from the map's norm:
    # the predicted change is 1e-3 per pair: a thousand times the ~1e-6 noise of an f32 forward, and a step of
    # relative size 1e-3 / |cos'| along the steepest direction, for which a quadratic term of the same order as the
    # linear one would need a curvature a thousand times the slope.  Asserted: sign, and magnitude within 25 %.
    n2 = da.double().pow(2).sum((1, 2, 3))
    assert bool((n2 > 0).all())
    t = (1e-3 / n2).view(4, 1, 1, 1)
    predicted = (t.view(4) * n2)
    measured = cosine((a.double() + t * da.double()).float(), b) - c0
    print("pair_saliency: predicted change %s measured %s" % (predicted.tolist(), measured.tolist()))
    assert bool((measured > 0).all())
    assert float(((measured - predicted).abs() / predicted).max()) < 0.25
    cosf, _, _ = verification.pair_saliency(m, a, b, flip=True)
    with torch.no_grad():
        ea, eb = m(a)[0] + m(a.flip(3))[0], m(b)[0] + m(b.flip(3))[0]
    assert float((cosf.double() - F.cosine_similarity(ea.double(), eb.double(), dim=1)).abs().max()) < 1e-5
