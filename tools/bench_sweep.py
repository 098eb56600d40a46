"""Time the input kernel of the occlusion sweep (msml_eval_pairs, csrc/evalin.hip) and one full extraction of test.py
on synthetic data.  The kernel is timed with events after a warm-up (median of --reps) at N = 25 (the reference's batch)
and N = 1024, for the RGB 112 x 112 recipe and the gray 128 x 128 one, black and gauss fill at [40, 41), beside a device
copy that moves the same number of bytes (read + write) in the same run: the ratio to that copy is what to read, the
absolute numbers move with the clock.  The extraction: --images synthetic 112 x 112 faces (lfw: 12 000) through an
iresnet50 MSML at the default eval precision in batches of --batch, timed as a whole with a host clock around a device
synchronise, and the same loop with the model call left out: input preparation's share of the extraction.
Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_sweep.py [--images 12000 --batch 256] [--reps 20] [--out profiles/sweep_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import data  # noqa: E402
from msml_amd import verification as V  # noqa: E402
from msml_amd._lib import call  # noqa: E402
from tools.bench_align import copy_of, timed  # noqa: E402


def kernel_row(n, size, out, gray, norm, fill, reps):
    src = torch.empty(n, size, size, 3, dtype=torch.uint8, device="cuda").random_(0, 256)
    desc = data.draw(2 * n, 1, 0, mode="block", lo=40, hi=41, flip=False, size=out)
    dst = torch.empty(2 * n, 1 if gray else 3, out, out, dtype=torch.float32, device="cuda")
    med, low = timed(lambda: call("msml_eval_pairs", src, n, size, size, desc, dst, out, out, gray, norm,
                                  V.FILLS[fill], 0, 1, 0), reps)
    nbytes = src.numel() + dst.numel() * 4 + desc.numel() * 4
    cmed, clow = copy_of(nbytes, reps)
    return {"N": n, "source": size, "out": out, "gray": gray, "fill": fill, "us": round(med, 1), "us_min": round(low, 1),
            "bytes": int(nbytes), "GB/s": round(nbytes / med / 1e3, 1), "copy_us": round(cmed, 1),
            "copy_us_min": round(clow, 1), "fraction_of_copy_rate": round(cmed / med, 3)}


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=12000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frb", default="iresnet50")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--extract-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for n in (25, 1024):
        for size, out, gray, norm in ((112, 112, 0, 1), (112, 128, 1, 0)):
            for fill in ("black", "gauss"):
                rows.append(kernel_row(n, size, out, gray, norm, fill, a.reps))
    from msml_amd.backbones import MSML
    torch.manual_seed(0)
    model = MSML(a.frb, "unet", (1, 1, 1, 1), 8, fp16=True, fm_params=(3, 2, "sigmoid", "mul"), header_type="AMArcFace",
                 peer_params={"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}).cuda().eval()
    src = torch.empty(a.images, 112, 112, 3, dtype=torch.uint8, device="cuda").random_(0, 256)

    class InputsOnly(torch.nn.Module):                    # the same loop without the network
        def forward(self, x):
            return x[:, 0, 0, :8]
    kw = dict(batch=a.batch, seed=1, lo=40, hi=41)
    full = wall(lambda: V.extract_sum(model, src, **kw), a.extract_reps)
    prep = wall(lambda: V.extract_sum(InputsOnly(), src, **kw), a.extract_reps)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "kernel": rows,
           "extraction": {"images": a.images, "batch": a.batch, "frb": a.frb, "eval_precision": model.eval_precision,
                          "block": [40, 41], "reps": a.extract_reps, "ms": round(full[0], 1), "ms_min": round(full[1], 1),
                          "images_per_s": round(a.images / full[0] * 1e3),
                          "input_preparation_ms (draw + msml_eval_pairs + pair sum, no model)": round(prep[0], 2),
                          "input_preparation_share": round(prep[0] / full[0], 4)}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
