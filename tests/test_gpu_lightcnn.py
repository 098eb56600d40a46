"""LightCNN-29v2 FRB on the MI355X: the max-feature-map conv (msml_conv2d_mfm + msml_mfm_bwd) and the max + avg pool
(msml_pool2_*) against f64 torch, and the whole LightCNN-MSML against the goldens recorded from the reference
(tests/golden/g10_lightcnn_*.npz, tools/make_golden_lightcnn.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from msml_amd import _lib, ops, synthetic
from msml_amd import functional as Fh
from msml_amd.backbones import MSML
from msml_amd.backbones.frb.lightcnn import mfm
from msml_amd.tricks.consensus_loss import StructureConsensuLossFunction
from oracle.fill import fill_module
from tests.helpers import assert_cs, cosine, elem_err, load, pick, rel_err

pytestmark = pytest.mark.gpu
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
BS, C = 4, 1000


def hip_lightcnn(header="Softmax", fp16=False, fm_layers=(1, 1, 1, 1), use_osb=True):
    torch.manual_seed(0)
    m = MSML("lightcnn", "unet", fm_layers, C, fp16=fp16, fm_params=(3, 2, "sigmoid", "mul"), header_type=header,
             header_params=(64.0, 0.5, 0.0, 0.0), peer_params=dict(PEER_OFF), use_osb=use_osb)
    return fill_module(m).cuda()


def inputs(bs=BS):
    return synthetic.rect_occlusion(synthetic.gray_images(bs, seed=1), seed=1)


# ---------------------------------------------------------------------------------------------------------------------
# mfm conv, module level

def mfm_shapes():
    """(cin, C, k, stride, pad, H, residual) of every distinct mfm of the FRB, read off the model's own modules by a
    forward hook (the stem, which runs on its im2col patches, is read off frb.conv1)."""
    m = MSML("lightcnn", "unet", (0, 0, 0, 0), 10, use_osb=False).cuda().eval()
    shapes = set()
    f = m.frb.conv1.filter
    shapes.add((f.in_channels, m.frb.conv1.out_channels, f.kernel_size[0], f.stride[0], f.padding[0], 128, False))

    def hook(mod, args, kwargs):
        f = mod.filter
        shapes.add((f.in_channels, mod.out_channels, f.kernel_size[0], f.stride[0], f.padding[0], args[0].shape[1],
                    kwargs.get("residual") is not None))
    hs = [mod.register_forward_pre_hook(hook, with_kwargs=True) for mod in m.frb.modules() if isinstance(mod, mfm)]
    with torch.no_grad():
        m(torch.rand(1, 1, 128, 128, device="cuda"))
    for h in hs:
        h.remove()
    return sorted(shapes)


def _nhwc_grad(t_nchw, cp, dtype):
    return ops.to_nhwc(t_nchw.float().contiguous(), dtype, cp)


def mfm_case(shape, dtype, ties):
    cin, c, k, stride, pad, h, res = shape
    n = 2
    torch.manual_seed(cin * 7 + c + h)
    conv = torch.nn.Conv2d(cin, 2 * c, k, stride, pad).cuda()
    with torch.no_grad():
        if ties:                                 # equal pair weights on every other channel: exact ties
            conv.weight[c::2][: (c + 1) // 2].copy_(conv.weight[0:c:2])
            conv.bias[c::2][: (c + 1) // 2].copy_(conv.bias[0:c:2])
    tdt = torch.bfloat16 if dtype == _lib.BF16 else torch.float32
    x = torch.randn(n, cin, h, h, device="cuda").to(tdt).float()
    r = torch.randn(n, c, h, h, device="cuda").to(tdt).float() if res else None
    gy = torch.randn(n, c, h // stride, h // stride, device="cuda").to(tdt).float()
    cp = ops.cpad(c)
    # device side
    if k == 5:                                   # the stem: on the raw NCHW image
        raw = x.clone()
        y = Fh.mfm_stem(conv, c, raw, dtype)
        xh = None
    else:
        xh = ops.to_nhwc(x, dtype).requires_grad_()
        rh = ops.to_nhwc(r, dtype).requires_grad_() if res else None
        y = Fh.mfm_conv(conv, c, xh, rh)
    assert y.shape == (n, h // stride, h // stride, cp) and y.dtype == tdt
    assert not y[..., c:].float().abs().any(), "padded channels must stay zero"
    (y.float() * _nhwc_grad(gy, cp, dtype).float()).sum().backward()
    # f64 reference on the same (storage-rounded) operands
    wd = conv.weight.detach().to(tdt).double().requires_grad_()
    bd = conv.bias.detach().double().requires_grad_()
    xd = x.double().requires_grad_()
    z = F.conv2d(xd, wd, bd, stride, pad)
    yd = torch.max(z[:, :c], z[:, c:])
    rd = None
    if res:
        rd = r.double().requires_grad_()
        yd = yd + rd
    (yd * gy.double()).sum().backward()
    got_y = ops.to_nchw(y.detach(), c).double()
    out = {"y": rel_err(got_y.cpu().numpy(), yd.detach().cpu().numpy()),
           "dW": rel_err(conv.weight.grad.cpu().numpy(), wd.grad.cpu().numpy()),
           "db": rel_err(conv.bias.grad.cpu().numpy(), bd.grad.cpu().numpy())}
    if xh is not None:
        out["dX"] = rel_err(ops.to_nchw(xh.grad, cin).cpu().numpy(), xd.grad.cpu().numpy())
        if res:
            out["dR"] = rel_err(ops.to_nchw(rh.grad, c).cpu().numpy(), rd.grad.cpu().numpy())
    return out


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16], ids=["f32", "bf16"])
def test_mfm_conv_every_lightcnn_shape(dtype):
    """Forward (max in the epilogue, residual), backward (selector expansion -> dX, dW, db) of every distinct mfm shape
    of the model against F.conv2d + torch.max in f64; one pass with exact ties (equal pair weights), which torch splits
    0.5 / 0.5."""
    shapes = mfm_shapes()
    assert len(shapes) >= 8, shapes
    tol = 1e-4 if dtype == _lib.F32 else 3e-2
    for shape in shapes:
        for ties in (False, True):
            errs = mfm_case(shape, dtype, ties)
            print(shape, "ties" if ties else "", " ".join("%s %.2e" % kv for kv in errs.items()))
            for key, e in errs.items():
                assert e < tol, (shape, ties, key, e)


def test_mfm_pairing_exact_integers():
    """Fragment-layout check of the pair interleave (channel j with j + C of the REAL count, 48 stored as 64): integer
    data (exact in f32 and bf16), equal pair weights and an asymmetric bias -- the second half wins by j + 1 on even j,
    the first half on odd j -- so a wrong partner, lane or padding offset changes the result."""
    cin, c, h = 8, 48, 9
    conv = torch.nn.Conv2d(cin, 2 * c, 3, 1, 1).cuda()
    j = torch.arange(c, device="cuda").float()
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-1, 2, conv.weight.shape, device="cuda").float())
        conv.weight[c:] = conv.weight[:c]
        conv.bias[:c] = j % 5
        conv.bias[c:] = conv.bias[:c] + torch.where(j % 2 == 0, j + 1, -(j + 1))
    x = torch.randint(0, 2, (1, cin, h, h), device="cuda").float()
    z = F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), 1, 1)
    ref = torch.max(z[:, :c], z[:, c:])
    for dtype in (_lib.F32, _lib.BF16):
        y = Fh.mfm_conv(conv, c, ops.to_nhwc(x, dtype))
        assert torch.equal(ops.to_nchw(y, c).double(), ref), dtype
        assert not y[..., c:].float().abs().any()


# ---------------------------------------------------------------------------------------------------------------------
# pool

@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16], ids=["f32", "bf16"])
def test_pool_max_plus_avg(dtype):
    """F.max_pool2d(x, 2) + F.avg_pool2d(x, 2) and its backward against torch in f64, with tied maxima (small integers),
    a NaN and padded channels (48 -> 64)."""
    torch.manual_seed(3)
    n, c, h = 2, 48, 16
    x = torch.randint(0, 3, (n, c, h, h)).double()
    x[0, 5, 2, 3] = float("nan")
    x[1, 7, 9, 8] = float("nan")
    gy = torch.randn(n, c, h // 2, h // 2).double()
    if dtype == _lib.BF16:
        gy = gy.bfloat16().double()
    xd = x.clone().requires_grad_()
    yd = F.max_pool2d(xd, 2) + F.avg_pool2d(xd, 2)
    (yd * gy).sum().backward()
    xh = ops.to_nhwc(x.float().cuda(), dtype).requires_grad_()
    y = Fh.pool2(xh)
    assert y.shape == (n, h // 2, h // 2, 64) and not y[..., c:].float().abs().any()
    y.backward(ops.to_nhwc(gy.float().cuda(), dtype))
    got = ops.to_nchw(y.detach(), c).double().cpu()
    assert torch.allclose(got, yd.detach(), rtol=1e-2 if dtype == _lib.BF16 else 1e-6, atol=0, equal_nan=True)
    assert torch.isnan(got[0, 5, 1, 1]) and torch.isnan(got[1, 7, 4, 4])
    gx = ops.to_nchw(xh.grad, c).double().cpu()
    assert torch.allclose(gx, xd.grad, rtol=1e-2 if dtype == _lib.BF16 else 1e-6, atol=1e-6)
    assert not xh.grad[..., c:].float().abs().any()


# ---------------------------------------------------------------------------------------------------------------------
# whole model vs the reference's goldens

def test_lightcnn_eval_f32_golden():
    g = load("g10_lightcnn_eval.npz")
    m = hip_lightcnn().eval()
    x, _ = inputs()
    with torch.no_grad():
        feat, final_seg = m(x.cuda())
    torch.cuda.synchronize()
    err = rel_err(feat.cpu().numpy(), g["feature"])
    bits = np.packbits(Fh.mask_index(final_seg).cpu().numpy().reshape(-1))
    mism = int(np.unpackbits(bits ^ g["mask_bits"]).sum())
    print("lightcnn f32 eval: feature rel err %.3e, mask mismatches %d" % (err, mism))
    assert feat.shape == (BS, 256) and final_seg.shape == (BS, 2, 128, 128)
    assert err < 1e-3, err
    assert mism == 0, mism
    assert_cs(final_seg, g["final_seg_cs"], 1e-4, "final_seg")


def test_lightcnn_eval_bf16_and_split_bf16_refused():
    g = load("g10_lightcnn_eval.npz")
    m = hip_lightcnn(fp16=True).eval()
    x, _ = inputs()
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            m(x.cuda())                           # the default fp16 eval precision (bf16x3) is not built
        m.eval_precision = "bf16"
        feat, final_seg = m(x.cuda())
    err = rel_err(feat.float().cpu().numpy(), g["feature"])
    print("lightcnn bf16 eval: feature rel err %.3e" % err)
    assert err < 5e-2, err


def test_lightcnn_eval_without_osb():
    """use_osb=False, fm_layers (0,0,0,0): the FRB alone, against the same network in f64 torch (state dict of the
    HIP model loaded into an f64 copy built from plain torch ops)."""
    m = hip_lightcnn(fm_layers=(0, 0, 0, 0), use_osb=False).eval()
    x, _ = inputs(2)
    with torch.no_grad():
        feat, seg = m(x.cuda())
    assert seg is None
    sd = {k: v.double().cpu() for k, v in m.frb.state_dict().items()}

    def mf(name, t, res=None):
        z = F.conv2d(t, sd[name + ".filter.weight"], sd[name + ".filter.bias"], 1,
                     sd[name + ".filter.weight"].shape[-1] // 2)
        c = z.shape[1] // 2
        y = torch.max(z[:, :c], z[:, c:])
        return y if res is None else y + res

    def pool(t):
        return F.max_pool2d(t, 2) + F.avg_pool2d(t, 2)
    t = pool(mf("conv1", x.double()))
    for stage, blocks in ((1, 1), (2, 2), (3, 3), (4, 4)):
        for b in range(blocks):
            p = "block%d.%d" % (stage, b)
            t = mf(p + ".conv2", mf(p + ".conv1", t), t)
        t = mf("group%d.conv" % stage, mf("group%d.conv_a" % stage, t))
        if stage != 3:
            t = pool(t)
    ref = t.flatten(1) @ sd["fc.weight"].t() + sd["fc.bias"]
    err = rel_err(feat.cpu().numpy(), ref.numpy())
    print("lightcnn FRB-only eval vs f64: %.3e" % err)
    assert err < 1e-4, err


def run_train_step(m, bs=BS):
    x, msk = inputs(bs)
    label = synthetic.labels(bs, C, seed=1)
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=0.1 / 512 * bs, momentum=0.9, weight_decay=5e-4)
    final_cls, final_seg, kd = m(x.cuda(), label.cuda(), None)
    seg_loss = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")(final_seg, msk.cuda(), msk.cuda())
    cls_loss = F.cross_entropy(final_cls.float(), label.cuda())
    (cls_loss + seg_loss).backward()
    gnorm = torch.nn.utils.clip_grad_norm_(m.parameters(), 5, 2)
    return opt, final_cls, seg_loss, cls_loss, gnorm


HEADERS = {"softmax": "Softmax", "arcface": "AMArcFace"}


@pytest.mark.parametrize("head", sorted(HEADERS))
def test_lightcnn_train_step_f32_golden(head):
    """One full training step in exact-f32 mode against the reference's golden, with the tolerances of the g4 f32 test
    (tests/test_gpu_model.py::test_train_step_g4)."""
    g = load("g10_lightcnn_train_%s.npz" % head)
    m = hip_lightcnn(HEADERS[head])
    opt, final_cls, seg_loss, cls_loss, gnorm = run_train_step(m)
    tol = 1e-3
    print("lightcnn f32 %s: seg loss %.3e cls loss %.3e gnorm %.3e (rel)" % (
        head, abs(seg_loss.item() / g["seg_loss"] - 1), abs(cls_loss.item() / g["cls_loss"] - 1),
        abs(float(gnorm) / g["grad_norm"] - 1)))
    assert abs(seg_loss.item() - g["seg_loss"]) < tol * abs(g["seg_loss"])
    assert abs(cls_loss.item() - g["cls_loss"]) < tol * abs(g["cls_loss"])
    assert abs(float(gnorm) - g["grad_norm"]) < 5e-3 * abs(g["grad_norm"])
    assert_cs(final_cls, g["final_cls_cs"], tol, "final_cls")
    params = dict(m.named_parameters())
    worst, worst_el = 0.0, 0.0
    for key in g.files:
        if key.startswith("grad_pick/"):
            n = key.split("/", 1)[1]
            got = pick(params[n].grad, 32)
            e, ee = rel_err(got, g[key]), elem_err(got, g[key])
            worst, worst_el = max(worst, e), max(worst_el, ee)
            assert e < 1e-2 and ee < 1e-2, (n, e, ee)
    print("lightcnn f32 %s: worst picked-grad rel err %.3e (norm-wise), %.3e (element-wise)" % (head, worst, worst_el))
    opt.step()
    for key in g.files:
        if key.startswith("stat/"):
            n = key.split("/", 1)[1]
            assert rel_err(m.state_dict()[n].cpu().numpy(), g[key]) < 1e-3, n
    for key in g.files:
        if key.startswith("new_cs/"):
            assert_cs(params[key.split("/", 1)[1]].detach(), g[key], 1e-3, key)


def lightcnn_bf16_tolerances(case, cap):
    """The fixed rule of tests/helpers.bf16_tolerances applied to the LightCNN floor (tests/golden/g10_lightcnn_bf16_floor.npz,
    recorded by tools/make_bf16_floor_lightcnn.py: the reference's own step under oracle/bf16_emul.py's rounding model,
    32 draws): per parameter group (oracle.bf16_emul.param_group) min(2 x p90 over the draws of the group's worst
    gradient error, cap); losses / grad norm 2 x p90 of their per-draw errors; running statistics 2 x the maximum."""
    from oracle.bf16_emul import param_group
    fl = load("g10_lightcnn_bf16_floor.npz")
    draws = sorted({k.split("/")[1] for k in fl.files if k.startswith(case + "/draw")})
    assert len(draws) >= 32, case
    tol = {}
    for grp in ("osb", "head", "frb_early", "frb_late"):
        per = []
        for d in draws:
            v = [float(fl[k]) for k in fl.files
                 if k.startswith("%s/%s/" % (case, d)) and param_group(k.split("/", 2)[2]) == grp]
            if v:
                per.append(max(v))
        if per:
            tol[grp] = min(2.0 * float(np.percentile(per, 90)), cap)
    stat = max([float(fl[k]) for k in fl.files if k.startswith(case + "/stat/")] + [0.0])

    def scalar(name):
        per = [float(fl[k]) for k in fl.files if k.startswith(case + "/scalar") and k.endswith("/" + name)]
        return 2.0 * float(np.percentile(per, 90))
    tol["loss"] = max(scalar("loss_seg"), scalar("loss_cls"), 2e-3)
    tol["gnorm"] = max(scalar("gnorm"), 5e-3)
    tol["stat"] = max(2.0 * stat, 5e-3)
    return tol


@pytest.mark.parametrize("head", sorted(HEADERS))
def test_lightcnn_train_step_bf16_golden(head):
    """One bf16 training step against the same goldens.  The bounds are DERIVED, never fitted to this build: the bf16
    error floor of the reference's own LightCNN step under the rounding model of oracle/bf16_emul.py (plain PyTorch, no
    HIP code; tools/make_bf16_floor_lightcnn.py, 32 draws) through the fixed rule of tests/helpers.bf16_tolerances, with
    the batch-4 cap of tests/test_gpu_parity2.py (0.5: at batch 4 the emulated early-FRB floor of the ArcFace step already
    has a median of 0.40 at frb.fm_ops.0.same_conv, above the 0.35 cap the IResNet batch >= 8 steps use).  Per picked
    gradient: norm-wise error below its group's bound t and cosine >= 1 / sqrt(1 + t^2) (the cosine a norm-wise error t
    orthogonal to the gradient leaves; 0.94 at t = 0.35).  As in tests/test_gpu_parity2.py the gradients are compared
    before the clip, scaled by the REFERENCE's clip factor (the golden holds them after clip_grad_norm_(5))."""
    from oracle.bf16_emul import param_group
    g = load("g10_lightcnn_train_%s.npz" % head)
    tol = lightcnn_bf16_tolerances("lightcnn_%s_b4" % head, cap=0.5)
    m = hip_lightcnn(HEADERS[head], fp16=True)
    opt, final_cls, seg_loss, cls_loss, gnorm = run_train_step(m)
    unclip = float(max(1.0, (float(gnorm) + 1e-6) / 5.0))             # undo this build's clip ...
    ref_clip = float(min(1.0, 5.0 / (g["grad_norm"] + 1e-6)))          # ... and apply the reference's
    print("lightcnn bf16 %s: tolerances %s" % (head, " ".join("%s %.3f" % kv for kv in sorted(tol.items()))))
    print("lightcnn bf16 %s: grad norm %.4f vs %.4f (%.2e)" % (head, float(gnorm), g["grad_norm"],
                                                             abs(float(gnorm) / g["grad_norm"] - 1)))
    params = dict(m.named_parameters())
    bad = []
    for key in g.files:
        if key.startswith("grad_pick/"):
            n = key.split("/", 1)[1]
            got = pick(params[n].grad, 32) * (unclip * ref_clip)
            e, cs = rel_err(got, g[key]), cosine(got, g[key])
            t = tol[param_group(n)]
            print("lightcnn bf16 %s: %-42s rel %.3e cos %.4f (bound %.3f, %s)" % (head, n, e, cs, t, param_group(n)))
            if not (e < t and cs >= 1.0 / (1.0 + t ** 2) ** 0.5):
                bad.append((n, e, cs, t))
    print("lightcnn bf16 %s: seg loss %.3e cls loss %.3e (rel)" % (
        head, abs(seg_loss.item() / g["seg_loss"] - 1), abs(cls_loss.item() / g["cls_loss"] - 1)))
    assert not bad, bad
    assert abs(float(gnorm) - g["grad_norm"]) < tol["gnorm"] * abs(g["grad_norm"])
    assert abs(seg_loss.item() - g["seg_loss"]) < tol["loss"] * abs(g["seg_loss"])
    assert abs(cls_loss.item() - g["cls_loss"]) < tol["loss"] * abs(g["cls_loss"])
    opt.step()
    for key in g.files:
        if key.startswith("stat/"):
            n = key.split("/", 1)[1]
            assert rel_err(m.state_dict()[n].cpu().numpy(), g[key]) < tol["stat"], n


# ---------------------------------------------------------------------------------------------------------------------
# the training step as bench.py / train.py drive it: FlatSGD's in-place gradient arena, hipGraph replay

def _flat_run(use_graph, steps=3, arena=True):
    from msml_amd.optim import FlatSGD
    torch.manual_seed(0)
    m = fill_module(MSML("lightcnn", "unet", (1, 1, 1, 1), 50, fp16=True, fm_params=(3, 2, "sigmoid", "mul"),
                         header_type="Softmax", peer_params=dict(PEER_OFF))).cuda().train()
    params = [p for p in m.parameters() if p.requires_grad]
    opt = FlatSGD([{"params": params, "lr": 0.01}], 0.9, 5e-4, 5.0) if arena else None
    x, msk = inputs(4)
    x, msk, lab = x.cuda(), msk.cuda(), synthetic.labels(4, 50, seed=5).cuda()
    crit = StructureConsensuLossFunction(10.0, 5.0)

    def step():
        if opt is not None:
            opt.zero_grad()
        cls, seg, _ = m(x, lab)
        loss = F.cross_entropy(cls, lab) + crit(seg, msk, msk)
        loss.backward()
        if opt is not None:
            opt.step()
        return loss.detach()

    if not arena:                                   # one backward into plain .grad tensors
        step()
        torch.cuda.synchronize()
        return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    try:
        if use_graph is None:                        # one backward into the arena, no optimizer step
            opt.zero_grad()
            cls, seg, _ = m(x, lab)
            (F.cross_entropy(cls, lab) + crit(seg, msk, msk)).backward()
            ops.wgrad_stream_join()
            torch.cuda.synchronize()
            return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        losses = []
        if use_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = step()
            for _ in range(steps):
                graph.replay()
                losses.append(float(out))
        else:
            for _ in range(steps):
                losses.append(float(step()))
        torch.cuda.synchronize()
        return losses, opt.flat_w.clone(), {n: b.clone() for n, b in m.named_buffers() if "running" in n}
    finally:
        opt.release()


def test_lightcnn_gradients_into_the_flat_arena():
    """FlatSGD's in-place gradient arena (the mfm stem's dW through its (2C, 25, 1, 1) view of the (2C, 1, 5, 5)
    parameter, the filters' bias gradients, the padded FM BatchNorms) receives the gradients a plain backward computes."""
    plain = _flat_run(None, arena=False)
    flat = _flat_run(None)
    assert plain.keys() == flat.keys()
    worst = 0.0
    for n in plain:
        e = rel_err(flat[n].cpu().numpy(), plain[n].cpu().numpy())
        worst = max(worst, e)
        assert e < 1e-5, (n, e)
    print("lightcnn arena vs plain gradients: worst rel err %.3e" % worst)


def test_lightcnn_graph_replay_walks_the_eager_trajectory():
    """hipGraph capture of the bf16 LightCNN training step (FlatSGD): replays walk the eager trajectory.  Pins the
    per-step host state a replay does not re-run: the mfm packs (rebuilt when the weights changed) and the padded FM
    BatchNorms' running statistics (copied back to the modules)."""
    le, we, re_ = _flat_run(False)
    lg, wg, rg = _flat_run(True)
    print("lightcnn eager losses", le, "graph losses", lg, "bit-identical weights", bool(torch.equal(we, wg)))
    assert all(abs(a - b) <= 1e-5 * abs(a) for a, b in zip(le, lg)), (le, lg)
    assert float((we - wg).abs().max()) <= 1e-6 * float(we.abs().max())
    for n in re_:
        assert torch.allclose(re_[n], rg[n], rtol=1e-5, atol=1e-7), n


# ---------------------------------------------------------------------------------------------------------------------
# headers at the LightCNN embedding width (E = 256: head.hip's general path, not the E % 512 fast path)

def test_headers_at_256_against_cpu():
    from msml_amd.headers import AMArcFace, AMCosFace, Softmax
    from oracle import model as om
    torch.manual_seed(11)
    emb = torch.randn(6, 256)
    label = torch.tensor([3, 0, 7, -1, 5, 2])
    w = torch.randn(9, 256) * 0.05
    gy = torch.linspace(-1, 1, 6 * 9).reshape(6, 9)
    for cls, kind in ((AMArcFace, "arc"), (AMCosFace, "cos")):
        h = cls(256, 9, None, 64.0, 0.45, 0.0, 0.0).cuda()
        with torch.no_grad():
            h.weight.copy_(w)
        e = emb.cuda().requires_grad_(True)
        out = h(e, label.cuda())
        out.backward(gy.cuda())
        ed = emb.clone().requires_grad_(True)                 # CPU f32 (margin_logits builds its margin in f32)
        wd = w.clone().requires_grad_(True)
        cos = F.linear(F.normalize(ed), F.normalize(wd))
        ref = om.margin_logits(cos, label, kind, 64.0, 0.45, 0.0, 0.0)
        ref.backward(gy)
        errs = (rel_err(out.detach().cpu().numpy(), ref.detach().numpy()), rel_err(e.grad.cpu().numpy(), ed.grad.numpy()),
                rel_err(h.weight.grad.cpu().numpy(), wd.grad.numpy()))
        print(kind, "E=256: out %.2e demb %.2e dW %.2e" % errs)
        assert errs[0] < 1e-5 and errs[1] < 1e-4 and errs[2] < 1e-4, (kind, errs)
    h = Softmax(256, 9, None).cuda()
    with torch.no_grad():
        h.weight.copy_(w)
        h.bias.copy_(torch.linspace(-0.5, 0.5, 9))
    e = emb.cuda().requires_grad_(True)
    out = h(e, label.clamp_min(0).cuda())
    out.backward(gy.cuda())
    ref = emb.double() @ w.double().t() + torch.linspace(-0.5, 0.5, 9).double()
    assert rel_err(out.detach().cpu().numpy(), ref.numpy()) < 1e-5
    assert rel_err(e.grad.cpu().numpy(), (gy.double() @ w.double()).numpy()) < 1e-4
    assert rel_err(h.weight.grad.cpu().numpy(), (gy.double().t() @ emb.double()).numpy()) < 1e-4


def _pfc_reference(feat, label, w, s=64.0, m=0.48, eps=0.1):
    """CPU PartialFC step at W = 1 (every class local), as headers/partial_fc.py:115-175 of the reference computes it:
    ArcFace logits of x . normalize(W) (the features arrive normalised), loss = mean -log p(label), and the logit
    gradient (p - label-smoothed one-hot, eps 0.1) / batch."""
    from oracle import model as om
    xd = feat.float().clone().requires_grad_(True)           # (oracle.model.margin_logits builds its margin in f32)
    wd = w.float().clone().requires_grad_(True)
    logits = om.margin_logits(F.linear(xd, F.normalize(wd)), label, "arc", s, m, 0.0, 0.0)
    with torch.no_grad():
        p = torch.softmax(logits, 1)
        loss = -p.gather(1, label[:, None]).clamp_min(1e-30).log().mean()
        oh = torch.full_like(p, eps / (p.shape[1] - 1))
        oh.scatter_(1, label[:, None], 1.0 - eps)
    logits.backward((p - oh) / p.shape[0])
    return float(loss), xd.grad, wd.grad


def test_partial_fc_at_256_against_cpu():
    """PartialFC(embedding_size=256), W = 1, against the CPU formula -- which is first checked against the reference's
    own PartialFC golden at E = 512 (tests/golden/g6_partial_fc.npz)."""
    from msml_amd.headers import ArcMargin, PartialFC
    from oracle.inputs import PFC_B, PFC_C, pfc_inputs
    g = load("g6_partial_fc.npz")
    feat, label, w = pfc_inputs(1, 0)
    loss, xg, _ = _pfc_reference(feat, label, w)
    assert abs(loss - g["w1/r0/loss"]) < 1e-5 * abs(g["w1/r0/loss"])
    assert rel_err(xg.numpy(), g["w1/r0/x_grad"]) < 1e-5
    torch.manual_seed(12)
    feat = F.normalize(torch.randn(PFC_B, 256))
    w = torch.randn(PFC_C, 256) * 0.01
    p = PartialFC(0, 0, 1, PFC_B, False, ArcMargin(64.0, 0.48, 0.0, 0.0), PFC_C, embedding_size=256)
    with torch.no_grad():
        p.weight.copy_(w)
    opt = torch.optim.SGD([{"params": p.parameters()}], lr=0.01)
    x_grad, loss_v = p.forward_backward(label.cuda(), feat.cuda(), opt)
    loss, xg, wg = _pfc_reference(feat, label, w)
    errs = (abs(loss_v.item() / loss - 1), rel_err(x_grad.cpu().numpy(), xg.numpy()),
            rel_err(p.sub_weight.grad.cpu().numpy(), wg.numpy()))
    print("PartialFC E=256: loss %.2e x_grad %.2e dW %.2e" % errs)
    assert errs[0] < 1e-4 and errs[1] < 1e-4 and errs[2] < 1e-4, errs
