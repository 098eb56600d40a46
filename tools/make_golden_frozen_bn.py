"""Record the frozen-BatchNorm goldens (tests/golden/g20_frozen_bn.npz) from the IMPORTED reference.

Needs the reference checkout on the path (first argument, default ../reference next to this repository); runs on the
CPU.  iresnet18 MSML, AMArcFace, fm_params (3, 2, sigmoid, mul), the key-name fill of oracle/fill.py, batch 4, f32; inputs
are re-derived from seeds by the tests (oracle.inputs.eval_inputs, msml_amd.synthetic.labels, eval_weights below), so the
file holds outputs only, in the g4 format of oracle/make_golden.py with a record prefix.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_frozen_bn.py [REFERENCE_ROOT]

  mixed/...   m.train(), then every _BatchNorm in eval mode (fine-tuning with frozen BatchNorm): one step of CE +
              consensus seg loss; both losses, the final_cls checksum, picked gradients, the clipped-from grad norm.
              The recorder asserts that every running statistic (and num_batches_tracked) is bit-identical afterwards.
  eval/...    m.eval(), loss = (feature * r).sum() with the seeded r of eval_weights(): the picks of the same list that
              this loss reaches (the FRB reads the OSB's maps detached and the head is not run: the OSB and
              `classification.weight` have no gradient here and are not recorded).
Every recorded gradient is asserted finite with a nonzero norm.
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
from oracle.inputs import eval_inputs  # noqa: E402

BS, C = 4, 1000
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
GRAD_NAMES = [
    # conv weights: FRB, OSB, FM operators
    "frb.conv1.weight", "frb.layer1.0.conv1.weight", "frb.layer2.0.downsample.0.weight", "frb.layer4.1.conv2.weight",
    "frb.fm_ops.0.same_conv.weight", "frb.fm_ops.3.res_block.1.conv2.weight",
    "osb.conv1.weight", "osb.layer4.1.conv2.weight", "osb.gcm1.conv_l1.weight", "osb.deconv5.weight",
    # BatchNorm weights / biases (frozen statistics, live affine parameters)
    "frb.bn1.weight", "frb.layer1.0.bn1.bias", "frb.layer2.0.downsample.1.weight", "frb.layer3.1.bn2.weight",
    "frb.layer4.1.bn3.bias", "frb.bn2.weight", "frb.fm_ops.2.res_block.0.bn3.weight", "osb.layer1.0.bn1.bias",
    # PReLU weights
    "frb.prelu.weight", "frb.layer3.1.prelu.weight", "frb.fm_ops.1.res_block.0.prelu3.weight",
    "frb.fc.weight", "frb.fc.bias", "frb.features.bias", "classification.weight"]


def eval_weights():
    """The seeded r of the eval record's loss (feature * r).sum(); the tests call the same function."""
    return torch.randn(BS, 512, generator=torch.Generator().manual_seed(20))


def checksum(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), t.abs().max().item()], np.float64)


def pick(t, n=32):
    f = t.detach().reshape(-1)
    idx = torch.linspace(0, f.numel() - 1, n, dtype=torch.float32).long()
    return f[idx].float().numpy()


def ref_msml():
    import backbones
    torch.manual_seed(0)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        m = backbones.MSML(frb_type="iresnet18", osb_type="unet", fm_layers=(1, 1, 1, 1), num_classes=C, fp16=False,
                           header_type="AMArcFace", header_params=(64.0, 0.48, 0.0, 0.0),
                           fm_params=(3, 2, "sigmoid", "mul"), peer_params=dict(PEER_OFF))
    return fill_module(m)


def picks(m, rec, prefix, names):
    params = dict(m.named_parameters())
    for n in names:
        g = params[n].grad
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()) and float(g.norm()) > 0.0, (prefix, n)
        rec[prefix + "grad_cs/" + n] = checksum(g)
        rec[prefix + "grad_pick/" + n] = pick(g)
    return rec


def mixed_record(rec):
    from torch.nn.modules.batchnorm import _BatchNorm
    from tricks.consensus_loss import StructureConsensuLossFunction
    m = ref_msml()
    x, msk = eval_inputs(BS)
    label = synthetic.labels(BS, C, seed=1)
    m.train()
    nbn = 0
    for mod in m.modules():
        if isinstance(mod, _BatchNorm):
            mod.eval()
            nbn += 1
    before = {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}
    with contextlib.redirect_stderr(open(os.devnull, "w")):
        seg_crit = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")
    final_cls, final_seg, kd = m(x, label, None)
    seg_loss = seg_crit(final_seg, msk, msk)
    cls_loss = torch.nn.functional.cross_entropy(final_cls, label)
    total = cls_loss + 1.0 * seg_loss
    total.backward()
    gnorm = torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=5, norm_type=2)
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    rec.update({"mixed/final_cls_cs": checksum(final_cls), "mixed/final_seg_cs": checksum(final_seg),
                "mixed/seg_loss": np.float64(seg_loss.item()), "mixed/cls_loss": np.float64(cls_loss.item()),
                "mixed/total": np.float64(total.item()), "mixed/grad_norm": np.float64(float(gnorm)),
                "mixed/batchnorms": np.int64(nbn)})
    picks(m, rec, "mixed/", GRAD_NAMES)
    assert all("mixed/grad_pick/" + n in rec for n in GRAD_NAMES)
    return rec


def eval_record(rec):
    m = ref_msml()
    x, _ = eval_inputs(BS)
    m.eval()
    feature, final_seg = m(x)
    loss = (feature * eval_weights()).sum()
    loss.backward()
    rec.update({"eval/feature_cs": checksum(feature), "eval/loss": np.float64(loss.item())})
    picks(m, rec, "eval/", GRAD_NAMES)
    assert sum(k.startswith("eval/grad_pick/frb.") for k in rec) >= 15
    return rec


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rec = eval_record(mixed_record({}))
    np.savez_compressed(os.path.join(OUT, "g20_frozen_bn.npz"), **rec)
    print("wrote g20_frozen_bn.npz:", len(rec), "entries,", int(rec["mixed/batchnorms"]), "BatchNorms")
