"""Backward through an eval-mode (frozen) BatchNorm on the device: msml_bn_eval_act_bwd through the C ABI against the
float64 reference and derived budgets of tests/bn_eval_cases.py (the checks tests/test_bn_eval_cpu.py runs on the torch
restatement), its refusals, the padded (LightCNN-width) path of functional.bn_act, and whole training / attribution steps
of iresnet18-MSML with frozen BatchNorms against the reference's golden (tests/golden/g20_frozen_bn.npz, recorded by
tools/make_golden_frozen_bn.py).  Memory hygiene as in tests/test_gpu_bn.py (tests/abi_harness.py): outputs between
guard bands, NaN pre-fill, inputs compared after the call.  Every shape is one the entry point documents as supported or
must refuse on the host."""
import pytest
import torch
import torch.nn.functional as F
from torch.nn.modules.batchnorm import _BatchNorm

import msml_amd
from msml_amd import _lib, synthetic
from msml_amd import functional as Fh
from msml_amd.backbones import MSML
from msml_amd.tricks.consensus_loss import StructureConsensuLossFunction
from oracle.fill import fill_module
from oracle.inputs import eval_inputs
from tests import bn_cases as B
from tests import bn_eval_cases as E
from tests.abi_harness import DTC, SENTINEL, GuardedDevice
from tests.helpers import assert_cs, elem_err, load, pick, rel_err

pytestmark = pytest.mark.gpu
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}


class Device(GuardedDevice):
    """msml_bn_eval_act_bwd with the interface of bn_eval_cases.Restatement."""

    def eval_bwd(self, dy, x, scale, shift, alpha, mean, invstd, res, grads, accumulate):
        M, C = x.shape
        dx = self.out(tuple(x.shape), x.dtype)
        dres = self.out(tuple(x.shape), x.dtype) if res is not None else None
        gs = [None if g is None else self.out((C,), torch.float32, g) for g in grads]
        ws, need = None, 0                              # no sums asked for: a null workspace
        if any(g is not None for g in grads):
            need = E.eval_rows(M, C) * 3 * C
            ws = self.out((need,), torch.float32)
        self.call("msml_bn_eval_act_bwd", dy, x, scale, shift, alpha, mean, invstd, res, dx, dres, gs[1], gs[0], gs[2],
                  accumulate, M, C, ws, need, DTC[x.dtype])
        for g, o in zip(grads, gs):
            if g is not None:
                g.copy_(o)
        return dx, dres


# ------------------------------------------------------------------------------------------- 1. the kernel, C ABI
@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("C", E.CS)
def test_kernel_against_f64(C, dt):
    rep = B.Report()
    cases = E.case_table("normal", Cs=(C,), dtypes=(dt,)) + E.case_table("lattice", Cs=(C,), dtypes=(dt,))
    assert len(cases) >= len(E.MS) * len(B._VARIANTS)
    for case in cases:
        E.check_eval_case(Device(), case, rep, "cuda")
    print(rep.table())
    print("elements excused at a PReLU branch (|z| within its own budget, z != 0):", rep.ambiguous)
    assert not rep.failures, rep.failures[:10]


# ------------------------------------------------------------------------------------------- 2. refusals
def test_refusals_before_any_launch():
    M, C = 64, 64
    dev = GuardedDevice()
    f = torch.ones(4 * 2064, device="cuda")
    x = torch.ones(M * 2064, device="cuda")

    def status(M_, C_, dx_null=False, ws_floats=None, want=True):
        dx = dev.out((M * 2064,), torch.float32, 7.0)
        gs = [dev.out((2064,), torch.float32, 7.0) for _ in range(3)]
        ws = dev.out((1 << 16,), torch.float32, 7.0)
        rc = _lib.call_status("msml_bn_eval_act_bwd", x, x, f, f, f, f, f, None, None if dx_null else dx, None,
                              gs[0] if want else None, gs[1] if want else None, gs[2] if want else None, 0, M_, C_, ws,
                              (1 << 16) if ws_floats is None else ws_floats, _lib.F32)
        torch.cuda.synchronize()
        for t in [dx, ws] + gs:                         # untouched
            assert bool((t == 7.0).all())
        for buf, n in dev.bufs:
            assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + n:] == SENTINEL).all())
        return rc

    assert status(M, 24) == -4                          # MSML_ERR_UNSUPPORTED: 256 % (C / 8)
    assert b"must divide 256" in _lib.load().msml_last_error()
    assert status(M, 2056) == -1                        # MSML_ERR_SHAPE: C > 2048
    assert status(0, C) == -1
    assert status(M, C, dx_null=True) == -1
    rows = E.eval_rows(M, C)
    assert rows >= 1
    assert status(M, C, ws_floats=rows * 3 * C - 1) == -5   # MSML_ERR_WORKSPACE


def test_refusal_of_a_missing_workspace():
    M, C = 16, 8
    x = torch.ones(M, C, device="cuda")
    f = torch.ones(C, device="cuda")
    dx, db = torch.full((M, C), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda")
    rc = _lib.call_status("msml_bn_eval_act_bwd", x, x, f, f, None, f, f, None, dx, None, None, db, None, 0, M, C, None, 0,
                          _lib.F32)
    torch.cuda.synchronize()
    assert rc == -5 and bool((dx == 7.0).all()) and bool((db == 7.0).all())


# ------------------------------------------------------------------------------------------- 3. the padded path
@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("variant", ("plain", "prelu", "prelu_res", "prelu_res_first"))
def test_bn_act_padded_eval_backward(variant, dt):
    """functional.bn_act on a 24-channel BatchNorm stored in 32 channels (_bn_act_padded), eval mode, against
    F.batch_norm(training=False) [+ F.prelu] [+ residual] with autograd in f64.

    Budgets (u = 2^-24, SAFETY 2): scale = gamma / sqrtf(rvar + eps) carries 4 roundings, dx = scale * (dy * alpha) two
    more and the store one u_store: 7 u |dx| + u_store |dx|.  A parameter gradient is a sum over M pixels: (chain + 8) u
    sum |term| with chain the grid-stride trips + LDS lanes (bn_cases.grid_chain), + 2 u |sum| for the f32 result and the
    copy; for bf16 dres feeds nothing here.  Elements whose |z| < 1e-4 (either PReLU branch in f32) are excused and
    counted; there must be almost none."""
    g = torch.Generator().manual_seed(24)
    N, H, W, CR, CP = 2, 9, 7, 24, 32
    M = N * H * W
    bn = torch.nn.BatchNorm2d(CR, eps=1e-5)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.5 * torch.randn(CR, generator=g))
        bn.bias.copy_(0.5 * torch.randn(CR, generator=g))
        bn.running_mean.copy_(0.3 * torch.randn(CR, generator=g))
        bn.running_var.copy_(1.0 + 0.5 * torch.rand(CR, generator=g))
    prelu = torch.nn.PReLU(CR)
    with torch.no_grad():
        prelu.weight.copy_(0.25 + 0.1 * torch.randn(CR, generator=g))
    bn, prelu = bn.cuda().eval(), prelu.cuda()
    stats0 = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())

    def padded(t):
        return F.pad(t, (0, CP - CR)).to(dt).cuda()
    x0, r0, dy0 = (torch.randn(N, H, W, CR, generator=g) for _ in range(3))
    x = padded(x0).requires_grad_(True)
    res = padded(r0).requires_grad_(True) if "res" in variant else None
    dy = padded(dy0)
    use_prelu = variant != "plain"
    y = Fh.bn_act(x, None, bn, prelu if use_prelu else None, res, variant == "prelu_res_first")
    y.backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(bn.running_mean, stats0[0]) and torch.equal(bn.running_var, stats0[1])
    assert torch.equal(bn.num_batches_tracked, stats0[2])
    assert bool((x.grad[..., CR:] == 0).all()), "pad channels of dx"
    # f64 autograd on exactly the stored operands
    xd = x.detach()[..., :CR].double().reshape(M, CR).requires_grad_(True)
    rd = res.detach()[..., :CR].double().reshape(M, CR).requires_grad_(True) if res is not None else None
    gam, bet = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    al = prelu.weight.detach().double().requires_grad_(True)
    z = F.batch_norm(xd, bn.running_mean.double(), bn.running_var.double(), gam, bet, False, 0.1, bn.eps)
    if variant == "prelu_res_first":
        z = z + rd
    zpre = z.detach()
    if use_prelu:
        z = F.prelu(z, al)
    if variant == "prelu_res":
        z = z + rd
    dyd = dy[..., :CR].double().reshape(M, CR)
    z.backward(dyd)
    u, us = B.U32, B.u_store(dt)
    near = (zpre.abs() < 1e-4) if use_prelu else torch.zeros_like(zpre, dtype=torch.bool)
    assert int(near.sum()) <= 2
    got = x.grad[..., :CR].double().reshape(M, CR)
    bud = B.SAFETY * (7 * u + us) * xd.grad.abs() + 1e-30
    assert bool((((got - xd.grad).abs() <= bud) | near).all()), float(((got - xd.grad).abs() / bud)[~near].max())
    if res is not None:
        gotr = res.grad[..., :CR].double().reshape(M, CR)
        budr = B.SAFETY * (2 * u + us) * rd.grad.abs() + 1e-30
        assert bool((((gotr - rd.grad).abs() <= budr) | near).all())
        assert bool((res.grad[..., CR:] == dy[..., CR:]).all() if variant == "prelu_res" else (res.grad[..., CR:] == 0).all())
    chain = B.grid_chain(M, CP, E.eval_rows(M, CP))
    gg = dyd * torch.where(zpre <= 0, al.detach(), torch.ones_like(zpre)) if use_prelu else dyd
    xh = (xd.detach() - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps)
    jump = (near * (dyd * (1.0 - al.detach())).abs()) if use_prelu else torch.zeros_like(dyd)
    terms = {"weight": (bn.weight.grad, gam.grad, gg * xh, jump * xh.abs()), "bias": (bn.bias.grad, bet.grad, gg, jump)}
    if use_prelu:
        terms["alpha"] = (prelu.weight.grad, al.grad, dyd * zpre.clamp_max(0.0), near * dyd.abs() * 1e-4)
    for name, (gt, ref, t, extra) in terms.items():
        b = B.SAFETY * ((chain + 8) * u * t.abs().sum(0) + 2 * u * ref.abs() + extra.sum(0)) + 1e-30
        assert gt.shape == (CR,) and bool(((gt.double() - ref).abs() <= b).all()), (name, float(((gt.double() - ref).abs() / b).max()))


# ------------------------------------------------------------------------------------------- whole-model steps
def hip_msml(fp16=False):
    torch.manual_seed(0)
    m = MSML("iresnet18", "unet", (1, 1, 1, 1), 1000, fp16=fp16, fm_params=(3, 2, "sigmoid", "mul"),
             header_type="AMArcFace", header_params=(64.0, 0.48, 0.0, 0.0), peer_params=dict(PEER_OFF))
    return fill_module(m).cuda()


def bn_state(m, under=None):
    return {k: v.clone() for k, v in m.state_dict().items()
            if ("running_" in k or "num_batches_tracked" in k) and (under is None or k.startswith(under))}


def mixed_step(m, freeze=lambda m: msml_amd.freeze_batchnorm(m, affine=False)):
    """m.train(), BatchNorms frozen by `freeze`, one step of CE + consensus seg loss (no optimizer step)."""
    bs = 4
    x, msk = eval_inputs(bs)
    label = synthetic.labels(bs, 1000, seed=1)
    m.train()
    nfrozen = freeze(m)
    final_cls, final_seg, kd = m(x.cuda(), label.cuda(), None)
    seg_loss = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")(final_seg, msk.cuda(), msk.cuda())
    cls_loss = F.cross_entropy(final_cls, label.cuda())
    (cls_loss + seg_loss).backward()
    torch.cuda.synchronize()
    return final_cls, seg_loss, cls_loss, nfrozen


def check_picks(m, g, prefix):
    params = dict(m.named_parameters())
    worst, worst_el, n = 0.0, 0.0, 0
    for key in g.files:
        if key.startswith(prefix + "grad_pick/"):
            name = key.split("/", 2)[2]
            got = pick(params[name].grad, 32)
            e, ee = rel_err(got, g[key]), elem_err(got, g[key])
            worst, worst_el, n = max(worst, e), max(worst_el, ee), n + 1
            assert e < 1e-2 and ee < 1e-2, (name, e, ee)       # norm-wise AND worst single element
    print("%s worst picked-grad rel err %.3e (norm-wise), %.3e (element-wise) over %d picks" % (prefix, worst, worst_el, n))
    return n


# ------------------------------------------------------------------------------------------- 4. the golden records
def test_golden_mixed_f32():
    g = load("g20_frozen_bn.npz")
    m = hip_msml()
    final_cls, seg_loss, cls_loss, nfrozen = mixed_step(m)
    assert nfrozen == int(g["mixed/batchnorms"]) == 85
    tol = 1e-3
    assert abs(seg_loss.item() - g["mixed/seg_loss"]) < tol * abs(g["mixed/seg_loss"])
    assert abs(cls_loss.item() - g["mixed/cls_loss"]) < tol * abs(g["mixed/cls_loss"])
    assert_cs(final_cls, g["mixed/final_cls_cs"], tol, "final_cls")
    gnorm = torch.nn.utils.clip_grad_norm_(m.parameters(), 5, 2)      # (the recorder picks after the clip, as g4 does)
    assert abs(float(gnorm) - g["mixed/grad_norm"]) < 5e-3 * abs(g["mixed/grad_norm"])
    assert check_picks(m, g, "mixed/") >= 25


def test_golden_eval_f32():
    g = load("g20_frozen_bn.npz")
    m = hip_msml().eval()
    x, _ = eval_inputs(4)
    r = torch.randn(4, 512, generator=torch.Generator().manual_seed(20))      # tools/make_golden_frozen_bn.eval_weights
    before = bn_state(m)
    feature, final_seg = m(x.cuda())
    loss = (feature * r.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - g["eval/loss"]) < 1e-3 * abs(g["eval/loss"])
    assert_cs(feature, g["eval/feature_cs"], 1e-3, "feature")
    assert check_picks(m, g, "eval/") >= 15
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())


# ------------------------------------------------------------------------------------------- 5. frozen stays frozen
@pytest.mark.parametrize("fp16", (False, True))
def test_frozen_stays_frozen(fp16):
    m = hip_msml(fp16)
    before = bn_state(m)
    assert len(before) == 3 * 85
    mixed_step(m)
    after = m.state_dict()
    changed = [k for k, v in before.items() if not torch.equal(after[k], v)]
    assert not changed, changed[:8]
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(gr).all()) for gr in grads)


# ------------------------------------------------------------------------------------------- 6. freeze_batchnorm
def test_freeze_batchnorm_affine():
    runs = {}
    for affine in (False, True):
        m = hip_msml()
        _, _, _, n = mixed_step(m, lambda mod: msml_amd.freeze_batchnorm(mod, affine=affine))
        assert n == 85
        runs[affine] = m
    frozen = {id(p) for mod in runs[True].modules() if isinstance(mod, _BatchNorm) for p in (mod.weight, mod.bias)}
    assert len(frozen) == 2 * 85
    live = dict(runs[False].named_parameters())
    other = 0
    for name, p in runs[True].named_parameters():
        if id(p) in frozen:
            assert p.grad is None and not p.requires_grad, name
        elif p.grad is not None or live[name].grad is not None:
            # dx of a frozen BatchNorm does not depend on its sums: everything else is the same arithmetic
            assert torch.equal(p.grad, live[name].grad), name
            other += 1
    assert other > 100
    # as in torch, module.train() undoes the mode (not requires_grad)
    runs[True].train()
    assert all(mod.training for mod in runs[True].modules() if isinstance(mod, _BatchNorm))


# ------------------------------------------------------------------------------------------- autograd node names
def _node_names(*outputs):
    seen, names, stack = set(), [], [o.grad_fn for o in outputs]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    return names


# ------------------------------------------------------------------------------------------- 7 / 8. every block, locally
# The method of tests/test_gpu_block_local.py with the reference block's BatchNorms in the mode of the HIP block's: ONE
# block recomputed in f64 torch (the oracle's block class, the HIP block's parameters and running statistics) from the
# tensors the HIP block saw in the step -- its bf16 input, the gradient that arrived at its output -- and compared with
# what the HIP block produced: forward output, input gradient, every parameter gradient.  The unfused path has no
# blocks.TAP, so the tensors are taken with module / tensor hooks, for fused and unfused blocks alike.  Bound of every
# quantity: FLOOR_X (CHAN_X per channel) x the error of the same block under the bf16 rounding model of
# oracle/bf16_emul.py, worst of three draws, + the absolute terms of that file, all taken over unchanged.
def _step_with_hooks(freeze_roots):
    """One bf16 training step of iresnet18-MSML at batch 4 (gradients in place in FlatSGD's arena) with the BatchNorms
    under `freeze_roots(model)` frozen.  Returns (model, records by block name, gradients by parameter name, node names)."""
    from msml_amd.optim import FlatSGD
    m = hip_msml(True)
    bs = 4
    x, msk = eval_inputs(bs)
    label = synthetic.labels(bs, 1000, seed=1)
    m.train()
    for root in freeze_roots(m):
        msml_amd.freeze_batchnorm(root, affine=False)
    before = bn_state(m)
    opt = FlatSGD([{"params": [p for p in m.parameters() if p.requires_grad], "lr": 0.1 / 512 * bs}], 0.9, 5e-4, 5.0)
    recs, hooks = {}, []

    def watch(name):
        def fwd(mod, inp, out):
            r = recs.setdefault(name, {})
            r["x"], r["out"] = inp[0].detach().clone(), out.detach().clone()
            out.register_hook(lambda g: r.__setitem__("dout", g.detach().clone()))
            inp[0].register_hook(lambda g: r.__setitem__("dx", g.detach().clone()))
        return fwd
    for name, mod in m.named_modules():
        if name and hasattr(mod, "conv1") and hasattr(mod, "bn3"):
            hooks.append(mod.register_forward_hook(watch(name)))
    try:
        opt.zero_grad()
        final_cls, final_seg, _ = m(x.cuda(), label.cuda(), None)
        names = _node_names(final_cls, final_seg)
        loss = F.cross_entropy(final_cls, label.cuda()) + \
            StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")(final_seg, msk.cuda(), msk.cuda())
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().float().clone() for n, p in m.named_parameters() if p.grad is not None}
    finally:
        opt.release()
        for h in hooks:
            h.remove()
    return m, recs, grads, names, before


def _nchw64(t, c):
    return t[..., :c].permute(0, 3, 1, 2).float().double().contiguous()


def _ref_block(mod, dtype):
    from oracle import model as om
    if hasattr(mod, "prelu3"):
        cin = cout = mod.conv1.weight.shape[1]
        ref = om.ResBottle(cin)
    else:
        cout, cin = mod.conv1.weight.shape[:2]
        ref = om.IBasicBlock(cin, cout, mod.conv2.stride[0], mod.downsample is not None)
    ref = ref.to(dtype).train()
    ref.load_state_dict({k: v.detach().to(dtype) if v.is_floating_point() else v.detach() for k, v in mod.state_dict().items()},
                        strict=True)
    ref = ref.cuda()
    for n, sub in mod.named_modules():                       # each BatchNorm in the mode of the HIP block's
        if isinstance(sub, _BatchNorm):
            ref.get_submodule(n).train(sub.training)
    return ref, cin, cout


def _block_errors(got, want, terms, elem_tol):
    tens, chan = {}, {}
    for k, wv in want.items():
        if k in terms:
            chan[k] = float(((got[k] - wv).abs() / terms[k].clamp_min(1e-300)).max())
        else:
            rel = float((got[k] - wv).norm() / wv.norm().clamp_min(1e-30))
            frac = float(((got[k] - wv).abs() > elem_tol * wv.abs().max()).double().mean())
            tens[k] = (rel, frac)
    return tens, chan


def _check_block_local(name, mod, r, grads):
    from oracle import bf16_emul
    from tests.test_gpu_block_local import CHAN_ABS, CHAN_X, ELEM_TOL, FLOOR_X, FRAC_ABS, NORM_ABS
    ref, cin, cout = _ref_block(mod, torch.float64)
    x64 = _nchw64(r["x"], cin).requires_grad_()
    dout64 = _nchw64(r["dout"], cout)
    terms, hooks = {}, []

    def watch(mname, bm):
        def fwd(_m, inp, out):
            z = inp[0].detach()

            def bwd(g):
                if isinstance(bm, torch.nn.PReLU):
                    terms[mname + ".weight"] = (g * z.clamp_max(0)).pow(2).sum((0, 2, 3)).sqrt().double()
                    return
                if bm.training:
                    mu, var = z.mean((0, 2, 3), keepdim=True), z.var((0, 2, 3), unbiased=False, keepdim=True)
                else:
                    mu, var = bm.running_mean.view(1, -1, 1, 1), bm.running_var.view(1, -1, 1, 1)
                xh = (z - mu) / (var + bm.eps).sqrt()
                terms[mname + ".bias"] = g.pow(2).sum((0, 2, 3)).sqrt().double()
                terms[mname + ".weight"] = (g * xh).pow(2).sum((0, 2, 3)).sqrt().double()
            out.register_hook(bwd)
        hooks.append(bm.register_forward_hook(fwd))
    for mname, bm in ref.named_modules():
        if isinstance(bm, (torch.nn.BatchNorm2d, torch.nn.PReLU)):
            watch(mname, bm)
    y64 = ref(x64)
    y64.backward(dout64)
    for h in hooks:
        h.remove()
    want = {"dx": x64.grad.detach(), "out": y64.detach()}
    want.update({pn: p.grad.detach() for pn, p in ref.named_parameters()})
    got = {"dx": _nchw64(r["dx"], cin), "out": _nchw64(r["out"], cout)}
    got.update({pn: grads[name + "." + pn].double() for pn in want if pn not in ("dx", "out")})
    h_tens, h_chan = _block_errors(got, want, terms, ELEM_TOL)
    f_tens, f_chan = {}, {}
    for shift in (0.0, 0.31, -0.27):
        emu, _, _ = _ref_block(mod, torch.float32)
        bf16_emul.emulate(emu)
        bf16_emul.GRID_SHIFT = shift
        try:
            xe = x64.detach().float().requires_grad_()
            ye = emu(xe)
            ye.backward(dout64.float())
        finally:
            bf16_emul.GRID_SHIFT = 0.0
        ge = {"dx": bf16_emul._r(xe.grad).double(), "out": bf16_emul._r(ye.detach()).double()}
        ge.update({pn: p.grad.double() for pn, p in emu.named_parameters()})
        a, b = _block_errors(ge, want, terms, ELEM_TOL)
        for k, (e, fr) in a.items():
            f_tens[k] = (max(f_tens.get(k, (0, 0))[0], e), max(f_tens.get(k, (0, 0))[1], fr))
        for k, e in b.items():
            f_chan[k] = max(f_chan.get(k, 0.0), e)
    rows = [("norm-wise", name + "." + k, e, FLOOR_X * f_tens[k][0] + NORM_ABS) for k, (e, _) in h_tens.items()]
    rows += [("element fraction", name + "." + k, fr, FLOOR_X * f_tens[k][1] + FRAC_ABS) for k, (_, fr) in h_tens.items()]
    rows += [("per-channel", name + "." + k, e, CHAN_X * f_chan[k] + CHAN_ABS) for k, e in h_chan.items()]
    return rows


def _local_check_all(m, recs, grads):
    rows = []
    with torch.backends.cudnn.flags(enabled=False):          # torch's native f64 / f32 conv kernels on the device
        for name, mod in m.named_modules():
            if name in recs:
                assert {"x", "out", "dout", "dx"} <= set(recs[name]), (name, sorted(recs[name]))
                rows += _check_block_local(name, mod, recs[name], grads)
    for fam in ("norm-wise", "element fraction", "per-channel"):
        rr = [r for r in rows if r[0] == fam]
        top = sorted(rr, key=lambda r: -r[2] / r[3])[:3]
        print("   %s (%d rows), closest to their bounds: " % (fam, len(rr)) + "; ".join("%s %.2e (bound %.2e)" % r[1:] for r in top))
    return rows


def test_mixed_bf16_step_every_block_locally():
    """7. Every BatchNorm frozen: all 8 + 8 IBasicBlocks (FRB + OSB) and 8 FM bottlenecks run launch by launch."""
    m, recs, grads, names, before = _step_with_hooks(lambda m: (m,))
    assert names.count("_IBlockBackward") == 0 and names.count("_BottleBackward") == 0
    assert len(recs) == 8 + 8 + 8, len(recs)
    after = m.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items())
    rows = _local_check_all(m, recs, grads)
    bad = [r for r in rows if not r[2] < r[3]]
    assert not bad, bad[:10]


def test_partly_frozen_bf16_every_block_locally():
    """8. frb.layer1, frb.layer2 and the OSB frozen, the rest live: fused and unfused blocks side by side, each checked
    locally against the reference block with its BatchNorms in the same mode."""
    m, recs, grads, names, before = _step_with_hooks(lambda m: (m.frb.layer1, m.frb.layer2, m.osb))
    assert names.count("_IBlockBackward") == 4 and names.count("_BottleBackward") == 8
    assert len(recs) == 24
    after = m.state_dict()
    for k, v in before.items():
        if k.startswith(("frb.layer1.", "frb.layer2.", "osb.")):
            assert torch.equal(after[k], v), k
        elif "running_var" in k or "num_batches_tracked" in k:
            assert not torch.equal(after[k], v), k
    rows = _local_check_all(m, recs, grads)
    bad = [r for r in rows if not r[2] < r[3]]
    assert not bad, bad[:10]
