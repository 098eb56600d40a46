"""Training step of the reference's CASIA-WebFace LightCNN recipe (config.py:47-56,99-106) on one MI355X:
LightCNN-MSML, fm_layers (1,1,1,1), Softmax head over 10 572 identities, batch 256 gray 128x128 images, bf16, SGD
(momentum 0.9, weight decay 5e-4, gradient clip 5; msml_amd.optim.FlatSGD), eager with the side streams.  Prints one
JSON line: ms per step, images/s, algorithmic TFLOP/s at 31.1 GFLOP per image (3 x the 10.38 GFLOP forward), and the
achieved GB/s of the mfm-expansion and pool kernels; --detail adds the top launches by time (ops.PROFILE labels).

    python tools/bench_lightcnn.py [--steps 20] [--warmup 5] [--batch 256] [--detail]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GF_STEP_PER_IMAGE = 31.1
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10572)
    ap.add_argument("--detail", action="store_true")
    a = ap.parse_args()
    from msml_amd import ops, synthetic
    from msml_amd.backbones import MSML
    from msml_amd.optim import FlatSGD, reference_param_groups
    from msml_amd.tricks.consensus_loss import StructureConsensuLossFunction
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    model = MSML("lightcnn", "unet", (1, 1, 1, 1), a.classes, fp16=True, fm_params=(3, 2, "sigmoid", "mul"),
                 header_type="Softmax", peer_params=dict(PEER_OFF)).to(dev).train()
    opt = FlatSGD(reference_param_groups(model, a.batch, 1), 0.9, 5e-4, 5.0)
    seg_crit = StructureConsensuLossFunction(10.0, 5.0, "idx", "idx")
    batches = []
    for i in range(4):
        x, msk = synthetic.rect_occlusion(synthetic.gray_images(a.batch, seed=1 + 100 * i), seed=1 + 100 * i)
        batches.append((x.to(dev), msk.to(dev), synthetic.labels(a.batch, a.classes, seed=1 + 100 * i).to(dev)))
    it = [0]

    def step():
        x, msk, label = batches[it[0] % len(batches)]
        it[0] += 1
        opt.zero_grad()
        final_cls, final_seg, _ = model(x, label)
        loss = torch.nn.functional.cross_entropy(final_cls, label) + seg_crit(final_seg, msk, msk)
        loss.backward()
        opt.step()
        return loss

    ops.WGRAD_STREAM, ops.OSB_STREAM = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    assert torch.isfinite(loss).item(), "non-finite loss"
    # one profiled step, one stream: kernel times by launch label
    ops.WGRAD_STREAM = ops.OSB_STREAM = None
    step()
    ops.PROFILE.start()
    step()
    prof = ops.PROFILE.stop()
    ips = a.batch / dt
    out = {"metric": "lightcnn_msml_train_step", "batch": a.batch, "classes": a.classes, "dtype": "bf16",
           "ms_per_step": round(dt * 1e3, 2), "images_per_s": round(ips, 1),
           "tflops_algorithmic": round(ips * GF_STEP_PER_IMAGE / 1e3, 2), "gflop_per_image": GF_STEP_PER_IMAGE,
           "kernel_event_ms_per_step": round(sum(v["ms"] for v in prof.values()), 2)}
    for kind in ("mfm_bwd", "pool2_fwd", "pool2_bwd"):
        ms = sum(v["ms"] for k, v in prof.items() if k.startswith(kind))
        nb = sum(v["bytes"] for k, v in prof.items() if k.startswith(kind))
        out[kind] = {"ms": round(ms, 3), "GB_per_s": round(nb / max(ms, 1e-9) / 1e6, 1)}
    if a.detail:
        top = sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:25]
        out["top_launches"] = [{"name": k, "ms": round(v["ms"], 3), "n": v["n"],
                                "tflops": round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1) if v["flops"] else None}
                               for k, v in top]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
