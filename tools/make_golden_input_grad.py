"""Record the input-image gradient goldens (tests/golden/g21_input_grad.npz) from the IMPORTED reference.

Needs the reference checkout on the path (first argument, default ../reference next to this repository); runs on the
CPU.  The set-up of tools/make_golden_frozen_bn.py (iresnet18 MSML, AMArcFace, fm_params (3, 2, sigmoid, mul), the
key-name fill of oracle/fill.py, oracle.inputs.eval_inputs(4), f32) and of tools/make_golden_lightcnn.py for the third
record; inputs are re-derived from seeds by the tests, so the file holds outputs only.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_input_grad.py [REFERENCE_ROOT]

  eval/...      m.eval(), loss = (feature * r).sum() with the seeded r of make_golden_frozen_bn.eval_weights(): x.grad
                flows through the FRB stem only (the FRB reads the OSB's maps detached).
  train/...     m.train() with live BatchNorm, one step of CE + consensus seg loss as mixed_record there: x.grad flows
                through both stems.
  lightcnn/...  the LightCNN FRB (Softmax head, gray 128 x 128 inputs of make_golden_lightcnn.inputs), m.eval(),
                loss = (feature * r).sum() with lightcnn_weights(feature dim).
Each record: loss, xgrad_cs (sum, abs-sum, max-abs), xgrad_pick (4096 evenly spaced elements), xgrad_img0 (the full map
of image 0).  The gradient is asserted finite, of nonzero norm, and nonzero for every image.
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_frozen_bn as fb  # noqa: E402  (puts the repository and the reference on the path)
import make_golden_lightcnn as lc  # noqa: E402

from msml_amd import synthetic  # noqa: E402
from oracle.inputs import eval_inputs  # noqa: E402

NPICK = 4096


def lightcnn_weights(dim):
    """The seeded r of the lightcnn record's loss; the tests call the same function."""
    return torch.randn(fb.BS, dim, generator=torch.Generator().manual_seed(21))


def record(rec, prefix, x, loss):
    g = x.grad
    assert g is not None and g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.norm()) > 0.0, prefix
    assert all(float(g[i].abs().max()) > 0.0 for i in range(g.shape[0])), prefix
    rec.update({prefix + "loss": np.float64(loss.item()), prefix + "xgrad_cs": fb.checksum(g),
                prefix + "xgrad_pick": fb.pick(g, NPICK), prefix + "xgrad_img0": g[0].detach().float().numpy().copy()})
    return rec


def eval_record(rec):
    m = fb.ref_msml()
    x, _ = eval_inputs(fb.BS)
    x.requires_grad_(True)
    m.eval()
    feature, _ = m(x)
    loss = (feature * fb.eval_weights()).sum()
    loss.backward()
    return record(rec, "eval/", x, loss)


def train_record(rec):
    from tricks.consensus_loss import StructureConsensuLossFunction
    m = fb.ref_msml()
    x, msk = eval_inputs(fb.BS)
    x.requires_grad_(True)
    label = synthetic.labels(fb.BS, fb.C, seed=1)
    m.train()
    with contextlib.redirect_stderr(open(os.devnull, "w")):
        seg_crit = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")
    final_cls, final_seg, kd = m(x, label, None)
    total = torch.nn.functional.cross_entropy(final_cls, label) + 1.0 * seg_crit(final_seg, msk, msk)
    total.backward()
    return record(rec, "train/", x, total)


def lightcnn_record(rec):
    def run(dt):
        m = lc.ref_msml("Softmax").to(dt)
        x = lc.inputs(fb.BS)[0].to(dt).requires_grad_(True)
        m.eval()
        feature, _ = m(x)
        loss = (feature * lightcnn_weights(feature.shape[1]).to(dt)).sum()
        loss.backward()
        return x, loss
    x, loss = run(torch.float32)
    # The reference against itself in float64: mfm (a max of two channels) and the max pool route the gradient through
    # the larger input, so where two inputs are within rounding of each other the f32 and the f64 run take different
    # routes and single elements of x.grad move by far more than the norm does.  Recorded as [norm-wise, worst element /
    # largest element] over the whole map: what "equal to the reference" can mean for this network.
    g64 = run(torch.float64)[0].grad
    d = x.grad.double() - g64
    rec["lightcnn/ref_f64_err"] = np.array([float(d.norm() / g64.norm()), float(d.abs().max() / g64.abs().max())], np.float64)
    return record(rec, "lightcnn/", x, loss)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rec = lightcnn_record(train_record(eval_record({})))
    np.savez_compressed(os.path.join(fb.OUT, "g21_input_grad.npz"), **rec)
    print("wrote g21_input_grad.npz:", len(rec), "entries;",
          ", ".join("%s |x.grad| max %.3e" % (p, rec[p + "xgrad_cs"][2]) for p in ("eval/", "train/", "lightcnn/")))
