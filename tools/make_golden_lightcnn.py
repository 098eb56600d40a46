"""Record the LightCNN-MSML goldens (tests/golden/g10_lightcnn_*.npz) from the IMPORTED reference.

Needs the reference checkout on the path (first argument, default ../reference next to this repository); runs on the
CPU.  Weights are the key-name fill of oracle/fill.py (gain 0.5), inputs are re-derived from seeds by the tests
(msml_amd.synthetic.gray_images + rect_occlusion), so the files hold outputs only.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_lightcnn.py [REFERENCE_ROOT]

  g10_lightcnn_eval.npz           bs 4, f32, fm_params (3, 2, sigmoid, mul), Softmax: feature, packed mask bits,
                                  final_seg checksums, state-dict keys and shapes
  g10_lightcnn_train_{softmax,arcface}.npz
                                  one train step at bs 4 (train-mode BN in OSB and FM), the g4 format of
                                  oracle/make_golden.py: losses, selected gradients, updated running statistics
"""
import contextlib
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

from msml_amd import synthetic  # noqa: E402
from oracle.fill import fill_module  # noqa: E402

BS, C = 4, 1000
FM_PARAMS = (3, 2, "sigmoid", "mul")
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
GRAD_NAMES = ["frb.conv1.filter.weight", "frb.conv1.filter.bias", "frb.block1.0.conv1.filter.weight",
              "frb.block1.0.conv2.filter.bias", "frb.group1.conv_a.filter.weight", "frb.group2.conv.filter.weight",
              "frb.block3.2.conv2.filter.weight", "frb.block4.3.conv1.filter.bias", "frb.group4.conv.filter.weight",
              "frb.fc.weight", "frb.fc.bias", "frb.fm_ops.0.same_conv.weight", "frb.fm_ops.3.res_block.1.conv2.weight",
              "osb.conv1.weight", "osb.layer4.1.conv2.weight", "osb.gcm1.conv_l1.weight", "osb.gcm5.conv_r2.bias",
              "osb.deconv1.weight", "osb.deconv5.weight", "osb.layer1.0.bn1.bias", "classification.weight"]
STAT_NAMES = ["osb.bn1.running_mean", "osb.bn1.running_var", "osb.layer4.1.bn3.running_var",
              "frb.fm_ops.0.res_block.0.bn1.running_mean", "frb.fm_ops.2.res_block.0.bn2.running_mean",
              "frb.fm_ops.3.res_block.1.bn3.running_var"]


def inputs(bs):
    return synthetic.rect_occlusion(synthetic.gray_images(bs, seed=1), seed=1)


def checksum(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), t.abs().max().item()], np.float64)


def pick(t, n=64):
    f = t.detach().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, n, dtype=torch.float32).long()
    return f[idx].float().numpy()


def ref_msml(header, header_params=(64.0, 0.5, 0.0, 0.0)):
    import backbones
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        m = backbones.MSML(frb_type="lightcnn", osb_type="unet", fm_layers=(1, 1, 1, 1), num_classes=C, fp16=False,
                           header_type=header, header_params=header_params, fm_params=FM_PARAMS,
                           peer_params=dict(PEER_OFF))
    torch.manual_seed(0)
    return fill_module(m)


def eval_record():
    m = ref_msml("Softmax")
    x, _ = inputs(BS)
    m.eval()
    with torch.no_grad():
        feat, final_seg = m(x)
    sd = m.state_dict()
    idx = final_seg.max(1)[1]
    return {
        "feature": feat.numpy(),
        "mask_bits": np.packbits(idx.numpy().astype(np.uint8).reshape(-1)),
        "final_seg_margin_min": np.array((final_seg[:, 0] - final_seg[:, 1]).abs().min().item(), np.float64),
        "final_seg_cs": checksum(final_seg),
        "final_seg_pick": pick(final_seg, 256),
        "keys": np.array(list(sd.keys())),
        "shapes": np.array([",".join(str(d) for d in t.shape) for t in sd.values()]),
    }


def train_record(header):
    from tricks.consensus_loss import StructureConsensuLossFunction
    m = ref_msml(header)
    x, msk = inputs(BS)
    label = synthetic.labels(BS, C, seed=1)
    m.train()
    with contextlib.redirect_stderr(open(os.devnull, "w")):
        seg_crit = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")
    cls_crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.SGD(m.parameters(), lr=0.1 / 512 * BS, momentum=0.9, weight_decay=5e-4)
    final_cls, final_seg, kd = m(x, label, None)
    seg_loss = seg_crit(final_seg, msk, msk)
    cls_loss = cls_crit(final_cls, label)
    total = cls_loss + 1.0 * seg_loss
    total.backward()
    gnorm = torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=5, norm_type=2)
    rec = {
        "final_cls_cs": checksum(final_cls), "final_cls_pick": pick(final_cls, 128),
        "final_seg_cs": checksum(final_seg),
        "seg_loss": np.float64(seg_loss.item()), "cls_loss": np.float64(cls_loss.item()),
        "total": np.float64(total.item()), "grad_norm": np.float64(float(gnorm)),
    }
    params = dict(m.named_parameters())
    for n in GRAD_NAMES:
        g = params[n].grad
        rec["grad_cs/" + n] = checksum(g)
        rec["grad_pick/" + n] = pick(g, 32)
    opt.step()
    for n in ("frb.conv1.filter.weight", "osb.deconv5.weight"):
        rec["new_cs/" + n] = checksum(params[n])
    sd = m.state_dict()
    for n in STAT_NAMES:
        rec["stat/" + n] = sd[n].numpy().copy()
    return rec


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    np.savez_compressed(os.path.join(OUT, "g10_lightcnn_eval.npz"), **eval_record())
    np.savez_compressed(os.path.join(OUT, "g10_lightcnn_train_softmax.npz"), **train_record("Softmax"))
    np.savez_compressed(os.path.join(OUT, "g10_lightcnn_train_arcface.npz"), **train_record("AMArcFace"))
    print("wrote", OUT)
