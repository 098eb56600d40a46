"""Time the segmentation-branch evaluation kernels (csrc/segeval.hip) with events after a warm-up, median of --reps.

* mask_counts on 256 x [2][112][112] logits, f32 and bf16, against an int64 ground truth (the `msk` of data.augment),
  beside the same result composed from functional.mask_index + torch comparisons and sums, and beside a device copy
  that moves the bytes the kernel reads (a copy reads n / 2 and writes n / 2 of its n bytes, so it is sized at twice the
  read): the ratio to that copy is what to read, the absolute numbers move with the clock;
* label_blobs + blob_table on 256 masks of data.augment(mode="train"), 256 half-density random masks and 256
  serpentines, at 112 x 112 and 128 x 128, connectivity 8, beside scipy.ndimage.label of the same masks on ONE host
  thread (the labelling alone, no table).
Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_segeval.py [--reps 20] [--out profiles/segeval_bench.json]
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

from msml_amd import data, segeval  # noqa: E402
from msml_amd import functional as Fh  # noqa: E402
from tools.bench_align import copy_of, timed  # noqa: E402

N = 256


def torch_counts(pred, gt):
    p, g = Fh.mask_index(pred) == 0, gt == 0
    return torch.stack([(p & g).sum((1, 2)), (p & ~g).sum((1, 2)), (~p & g).sum((1, 2)), (~p & ~g).sum((1, 2))], 1)


def counts_row(dtype, reps):
    pred = torch.randn(N, 2, 112, 112, device="cuda").to(dtype).contiguous()
    gt = (torch.rand(N, 112, 112, device="cuda") < 0.7).to(torch.int64)
    assert torch.equal(segeval.mask_counts(pred, gt), torch_counts(pred, gt))
    med, low = timed(lambda: segeval.mask_counts(pred, gt), reps)
    tmed, tlow = timed(lambda: torch_counts(pred, gt), reps)
    nbytes = pred.numel() * pred.element_size() + gt.numel() * 8
    cmed, clow = copy_of(2 * nbytes, reps)
    return {"pred": str(dtype).replace("torch.", ""), "gt": "int64", "N": N, "bytes_read": int(nbytes),
            "us": round(med, 1), "us_min": round(low, 1), "GB/s": round(nbytes / med / 1e3, 1),
            "torch_us": round(tmed, 1), "torch_us_min": round(tlow, 1),
            "copy_us": round(cmed, 1), "copy_us_min": round(clow, 1), "ratio_to_copy": round(med / cmed, 2)}


def serpentine(size):
    occ = np.zeros((size, size), bool)
    occ[0::2] = True
    for k, y in enumerate(range(1, size, 2)):
        occ[y, size - 1 if k % 2 == 0 else 0] = True
    return occ


def masks(pattern, size):
    if pattern == "augment":
        src = torch.empty(N, size, size, 3, dtype=torch.uint8, device="cuda").random_(0, 256)
        return data.augment(src, 1, 0, mode="train", want_ori=False)[1].to(torch.uint8)
    if pattern == "random0.5":
        return (torch.rand(N, size, size, device="cuda") < 0.5).to(torch.uint8)
    return torch.from_numpy(~serpentine(size)).to(torch.uint8).cuda().expand(N, size, size).contiguous()


def label_row(pattern, size, reps):
    from scipy import ndimage
    m = masks(pattern, size)
    other = m.roll(1, 0).contiguous()
    labels, count, status = segeval.label_blobs(m, 8)
    assert not bool(status.any())
    lmed, llow = timed(lambda: segeval.label_blobs(m, 8), reps)
    tmed, tlow = timed(lambda: segeval.blob_table(m, other, 8, 64), reps)
    host = m.cpu().numpy() == 0
    ones = np.ones((3, 3), int)
    t0 = time.perf_counter()
    ks = [ndimage.label(o, structure=ones)[1] for o in host]
    scipy_ms = (time.perf_counter() - t0) * 1e3
    assert ks == count.cpu().tolist()
    return {"pattern": pattern, "size": size, "N": N, "components_mean": round(float(np.mean(ks)), 1),
            "label_us": round(lmed, 1), "label_us_min": round(llow, 1),
            "label_and_table_us": round(tmed, 1), "label_and_table_us_min": round(tlow, 1),
            "scipy_label_one_thread_us": round(scipy_ms * 1e3, 1),
            "scipy_over_label": round(scipy_ms * 1e3 / lmed, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    torch.set_num_threads(1)
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "mask_counts": [counts_row(dt, a.reps) for dt in (torch.float32, torch.bfloat16)],
           "label_blobs": [label_row(p, s, a.reps) for s in (112, 128) for p in ("augment", "random0.5", "serpentine")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
