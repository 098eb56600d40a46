"""Record the bf16 error FLOOR of the LightCNN-MSML training step (tests/golden/g10_lightcnn_bf16_floor.npz): the
IMPORTED reference run under the bf16 rounding model of oracle/bf16_emul.py (plain PyTorch hooks, no HIP code) against
the f32 goldens of tools/make_golden_lightcnn.py.  The GPU test derives its bf16 tolerances from these numbers with the
fixed rule of tests/helpers.bf16_tolerances instead of fitting them to the HIP path's own error.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_bf16_floor_lightcnn.py [REFERENCE_ROOT]

Rounding model (as oracle/bf16_emul.py states it for the IResNet oracle): conv / transposed conv / Linear operands and
outputs bf16 (weights in the forward only), the outputs of BatchNorm2d, PReLU, mfm, resblock, the OSB blocks, GCMs and FM
operators bf16 with bf16 gradients, the cosine / softmax head on bf16 operands with an f32 result whose gradient is
rounded.  Keys: "<case>/draw<u>/<parameter>" (norm-wise relative error of the picked gradient, the golden's clip factor
applied), "<case>/scalar<u>/{loss_seg,loss_cls,gnorm}", "<case>/stat/<buffer>" (maximum over the draws); 32 draws
(quantiser grid shifts) per case, as for the batch-4 IResNet cases.
"""
import contextlib
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

from msml_amd import synthetic  # noqa: E402
from oracle import bf16_emul  # noqa: E402
from oracle.fill import fill_module  # noqa: E402
from tests.helpers import load, pick, rel_err  # noqa: E402

BS, C = 4, 1000
CASES = [("lightcnn_softmax_b4", "g10_lightcnn_train_softmax.npz", "Softmax"),
         ("lightcnn_arcface_b4", "g10_lightcnn_train_arcface.npz", "AMArcFace")]
DRAWS = tuple(round((i + 0.5) / 32 - 0.5, 4) for i in range(32))
ROUNDED_OUTPUTS = ("BatchNorm2d", "PReLU", "mfm", "resblock", "IBasicBlock", "resblock_bottle", "_GlobalConvModule",
                   "FMCnn")
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}


class _HeadF:
    """torch.nn.functional as the reference's heads see it under emulation: F.linear on bf16 operands, its gradient
    rounded (bf16_emul._head_forward)."""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def linear(a, b, bias=None):
        # (a copy: the reference modifies the cosine in place)
        return bf16_emul._RoundBwd.apply(F.linear(bf16_emul.both(a), bf16_emul.both(b), bias)).clone()


def emulated_step(header, shift):
    import backbones
    import headers.margin_losses as ml
    bf16_emul.GRID_SHIFT = shift
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        m = backbones.MSML(frb_type="lightcnn", osb_type="unet", fm_layers=(1, 1, 1, 1), num_classes=C, fp16=False,
                           header_type=header, header_params=(64.0, 0.5, 0.0, 0.0), fm_params=(3, 2, "sigmoid", "mul"),
                           peer_params=dict(PEER_OFF))
    torch.manual_seed(0)
    fill_module(m)
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            mod.forward = bf16_emul._conv_forward(mod)
        elif isinstance(mod, torch.nn.Linear):
            mod.forward = bf16_emul._linear_forward(mod)
        elif type(mod).__name__ in ROUNDED_OUTPUTS:
            mod.register_forward_hook(bf16_emul._out_hook)
    from tricks.consensus_loss import StructureConsensuLossFunction
    x, msk = synthetic.rect_occlusion(synthetic.gray_images(BS, seed=1), seed=1)
    label = synthetic.labels(BS, C, seed=1)
    with contextlib.redirect_stderr(open(os.devnull, "w")):
        seg_crit = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")
    m.train()
    saved, ml.F = ml.F, _HeadF()
    try:
        final_cls, final_seg, _ = m(bf16_emul._r(x), label, None)
    finally:
        ml.F = saved
    seg_loss = seg_crit(final_seg, msk, msk)
    cls_loss = F.cross_entropy(final_cls, label)
    (cls_loss + seg_loss).backward()
    gnorm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None)))
    return m, float(seg_loss), float(cls_loss), gnorm


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rec = {}
    for key, fname, header in CASES:
        g = load(fname)
        worst = {}
        for shift in DRAWS:
            m, seg_loss, cls_loss, gnorm = emulated_step(header, shift)
            rec["%s/scalar%+.4f/loss_seg" % (key, shift)] = np.float64(abs(seg_loss / g["seg_loss"] - 1))
            rec["%s/scalar%+.4f/loss_cls" % (key, shift)] = np.float64(abs(cls_loss / g["cls_loss"] - 1))
            rec["%s/scalar%+.4f/gnorm" % (key, shift)] = np.float64(abs(gnorm / g["grad_norm"] - 1))
            params = dict(m.named_parameters())
            clip = float(min(1.0, 5.0 / (g["grad_norm"] + 1e-6)))
            for k in g.files:
                if k.startswith("grad_pick/"):
                    n = k.split("/", 1)[1]
                    e = rel_err(pick(params[n].grad, g[k].size) * clip, g[k])
                    rec["%s/draw%+.4f/%s" % (key, shift, n)] = np.float64(e)
                    worst[n] = max(worst.get(n, 0.0), e)
            sd = m.state_dict()
            for k in g.files:
                if k.startswith("stat/"):
                    n = k.split("/", 1)[1]
                    name = "%s/stat/%s" % (key, n)
                    rec[name] = np.float64(max(float(rec.get(name, 0.0)), rel_err(sd[n].numpy(), g[k])))
        bf16_emul.GRID_SHIFT = 0.0
        print(key, " ".join("%s %.3f" % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1])[:6]), flush=True)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g10_lightcnn_bf16_floor.npz"), **rec)


if __name__ == "__main__":
    main()
