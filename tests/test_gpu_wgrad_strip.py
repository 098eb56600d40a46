"""Strip weight-gradient kernel (wgrad_halo.hip) with SEVERAL strips per workgroup: ragged splits, empty workgroups,
ragged maps and the in-LDS BatchNorm variant, through the public entry points, against f64 torch on bf16-rounded
inputs (the project's bound: 1.5e-2 x max|ref|) -- the cases the double-buffered strip loop can get wrong and the
tests in test_gpu_conv.py do not reach."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from msml_amd import _lib, ops

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(shape, group):
    """(dY, X) pairs of `group` layers as bf16 NHWC device tensors and their f64 weight gradients (computed once)."""
    n, cin, cout, h, w_ = shape
    g = torch.Generator().manual_seed(sum(shape) + group)
    us, vs, refs = [], [], []
    for _ in range(group):
        x = torch.randn(n, cin, h, w_, generator=g).bfloat16().float()
        dy = torch.randn(n, cout, h, w_, generator=g).bfloat16().float()
        w = torch.zeros(cout, cin, 3, 3, dtype=torch.double, requires_grad=True)
        F.conv2d(x.double(), w, None, 1, 1).backward(dy.double())
        refs.append(w.grad.float())
        us.append(ops.to_nhwc(dy.cuda(), _lib.BF16))
        vs.append(ops.to_nhwc(x.cuda(), _lib.BF16))
    return us, vs, refs


# (N, Cin, Cout, H, W), group.  256-channel 14 x 14 layers run 128-row tiles on 8 workgroups per split:
#   N = 16, group 3: 32 strips over 10 splits per layer = chunk 4, eight full splits and two empty ones
#   N = 17, group 3: 34 strips over 10 splits = chunk 4, the ninth split short (2 strips), the tenth empty
#   N = 5,  group 1: 10 strips over 10 splits = one strip per workgroup (no second stage is ever requested)
# ragged maps, group 4: partial strip rows and columns in both stages, several strips per workgroup
GROUPED = [((16, 256, 256, 14, 14), 3), ((17, 256, 256, 14, 14), 3), ((5, 256, 256, 14, 14), 1),
           ((12, 128, 256, 13, 27), 4), ((10, 128, 128, 21, 28), 4)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("shape,group", GROUPED)
def test_wgrad_strip_grouped(shape, group, accumulate):
    n, cin, cout, h, w_ = shape
    assert group <= _lib.value("msml_conv_wgrad_group_max", cout, cin, cout, cin, n, h, w_, h, w_, 3, 3, 1, 1, 1)
    us, vs, refs = _case(shape, group)
    dws = [torch.full((cout, cin, 3, 3), 1.0 + i, device="cuda") for i in range(group)]
    need = _lib.value("msml_conv_wgrad_workspace", cout, cin, n, h, w_, 3, 3)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    arr = ctypes.c_void_p * group
    _lib.call("msml_conv_wgrad_group", arr(*[t.data_ptr() for t in us]), arr(*[t.data_ptr() for t in vs]),
              arr(*[t.data_ptr() for t in dws]), group, cout, cin, cout, cin, cin, 0, n, h, w_, h, w_, 3, 3, 1, 1, 1,
              int(accumulate), ws, ws.numel(), _lib.BF16)
    for i in range(group):
        want = refs[i] + (1.0 + i if accumulate else 0.0)
        err = (dws[i].cpu() - want).abs().max().item()
        print("layer %d: max err %.3e of max|ref| %.3e" % (i, err, refs[i].abs().max().item()))
        assert err <= 1.5e-2 * refs[i].abs().max().item(), i


BNIN_SHAPE = (72, 256, 256, 14, 14)       # 144 strips over 32 splits: chunk 5, 29 workgroup rows busy, 3 empty


@functools.lru_cache(maxsize=None)
def _bnin_case(with_alpha):
    n, cin, cout, h, w_ = BNIN_SHAPE
    g = torch.Generator().manual_seed(sum(BNIN_SHAPE) + int(with_alpha))
    x = ops.to_nhwc(torch.randn(n, cin, h, w_, generator=g).cuda(), _lib.BF16)
    coef = torch.stack([torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.5]).cuda()
    alpha = (torch.rand(cin, generator=g) * 0.3).cuda() if with_alpha else None
    dy = ops.to_nhwc(torch.randn(n, cout, h, w_, generator=g).cuda(), _lib.BF16)
    act = torch.empty_like(x)
    _lib.call("msml_bn_act_fwd", x, coef[0], coef[1], alpha, None, 0, act, n * h * w_, cin, _lib.BF16)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.double, requires_grad=True)
    F.conv2d(act.cpu().permute(0, 3, 1, 2).double(), w, None, 1, 1).backward(dy.cpu().permute(0, 3, 1, 2).double())
    return x, coef, alpha, dy, act, w.grad.float()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("with_alpha", [False, True])
def test_wgrad_strip_bnin_several_strips(with_alpha, accumulate):
    """In-LDS BatchNorm(+PReLU) of the X strips with five strips per workgroup: bit-equal to msml_bn_act_fwd ->
    msml_conv_wgrad, and inside the f64 bound."""
    n, cin, cout, h, w_ = BNIN_SHAPE
    x, coef, alpha, dy, act, ref = _bnin_case(with_alpha)
    assert _lib.value("msml_conv_wgrad_bnin_applies", cout, cin, cout, cin, n, h, w_, h, w_, 3, 3, 1, 1, 1) == 1
    dref = torch.full((cout, cin, 3, 3), 0.5, device="cuda")
    dgot = dref.clone()
    ops.conv_wgrad(dy, act, dref, cout, cin, cin, 0, 3, 3, 1, 1, 1, accumulate=accumulate)
    ops.conv_wgrad_bnin(dy, x, coef, alpha, dgot, cout, cin, cin, 0, accumulate=accumulate)
    assert torch.equal(dgot, dref)
    want = ref + (0.5 if accumulate else 0.0)
    err = (dgot.cpu() - want).abs().max().item()
    print("max err %.3e of max|ref| %.3e" % (err, ref.abs().max().item()))
    assert err <= 1.5e-2 * ref.abs().max().item()
