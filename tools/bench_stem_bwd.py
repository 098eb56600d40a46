"""msml_stem_bwd_data at the three real stem shapes (batch 256) beside a device copy of the same bytes (dy read + dx
written), the project's habit for byte-bound kernels.  Device events around `--reps` launches per sample, `--samples`
samples of kernel and copy INTERLEAVED, medians; inputs are seeded noise (the kernel's time does not depend on values).
Prints one JSON line: per shape the bytes, the kernel's and the copy's median ms and GB/s, their ratio, and the spread.

    python tools/bench_stem_bwd.py [--batch 256] [--reps 100] [--samples 9] [--warmup 3]

  frb       IResNet FRB stem   3 -> 64, 3x3, stride 1, 112 x 112     (bf16 dy, ldy 64)
  osb       OSB stem           3 -> 64, 3x3, stride 2, 112 x 112     (bf16 dy, ldy 64)
  lightcnn  LightCNN mfm stem  1 -> 96, 5x5, stride 1, 128 x 128     (bf16 dy, ldy 128: 96 real channels)
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"frb": (3, 112, 3, 1, 64, 64), "osb": (3, 112, 3, 2, 64, 64), "lightcnn": (1, 128, 5, 1, 96, 128)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from msml_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_stem_bwd: needs an MI355X (no CPU path)")
    out = {"metric": "stem_bwd_data", "batch": a.batch, "reps": a.reps, "samples": a.samples}
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, (c, hw, r, stride, cout, ldy) in SHAPES.items():
        p = ops.conv_out_size(hw, r, stride, r // 2, False)
        dy = torch.randn(a.batch, p, p, ldy, device="cuda", generator=g).to(torch.bfloat16)
        w = 0.1 * torch.randn(cout, c, r, r, device="cuda", generator=g)
        nbytes = dy.numel() * 2 + a.batch * c * hw * hw * 4
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")      # a copy moves its bytes twice: read + write
        dst = torch.empty_like(src)

        def kernel():
            return ops.stem_bwd_data(dy, w, a.batch, c, hw, hw, r, r, stride, r // 2)

        def copy():
            dst.copy_(src)
        for _ in range(a.warmup):
            kernel()
            copy()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(a.samples):
            tk.append(timed(kernel, a.reps))
            tc.append(timed(copy, a.reps))
        mk, mc = statistics.median(tk), statistics.median(tc)
        out[name] = {"MB": round(nbytes / 1e6, 1),
                     "band_rows": ops._lib.value("msml_stem_bwd_data_band", c, hw, hw, cout, r, stride),
                     "kernel_ms": round(mk, 4), "kernel_GB_per_s": round(nbytes / mk / 1e6, 1),
                     "kernel_ms_min_max": [round(min(tk), 4), round(max(tk), 4)],
                     "copy_ms": round(mc, 4), "copy_GB_per_s": round(nbytes / mc / 1e6, 1),
                     "copy_ms_min_max": [round(min(tc), 4), round(max(tc), 4)],
                     "kernel_over_copy": round(mk / mc, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
