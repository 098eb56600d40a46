"""Apply kernels of the device input pipeline on one MI355X, in one process, interleaved: the RGB 112 kernel
(msml_occ_apply, with and without ori) and the gray / resized one (msml_occ_apply_out) at the LightCNN recipe (gray,
128 x 128, no Normalize) and at RGB 128.  Device events around `--launches` launches after `--warmup`, `--rounds` rounds
with the cases alternating inside every round; the median round is reported, and the spread.

Bytes are ALGORITHMIC: the uint8 source read once, img / msk / ori written once.  (msml_occ_apply writes img, reads it
back and writes it again for  / max ; those extra bytes are not counted, so its rate is per useful byte, like the new
kernel's.)  Prints one JSON line per case and the ratio of every new case's rate to the same-shape-class yardstick --
the existing kernel's rate in the same run; 0.8 of it is the line below which the new kernel counts as a miss.

    python tools/bench_occ.py [--batch 256] [--launches 50] [--warmup 10] [--rounds 7] [--mode train] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(n, h, w, oh, ow, ch, want_ori):
    return n * (h * w * 3 + oh * ow * ch * 4 * (2 if want_ori else 1) + oh * ow * 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mode", default="train")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from msml_amd import data
    from msml_amd._lib import call
    if not torch.cuda.is_available():
        raise SystemExit("bench_occ: needs a GPU (a rate measured anywhere else says nothing)")
    n, h, w = a.batch, 112, 112
    src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    # name, (gray, out_size, use_norm), want_ori
    cases = [("occ_apply rgb112 norm ori", None, True), ("occ_apply rgb112 norm", None, False),
             ("occ_apply_out gray128 nonorm ori", (True, 128, False), True),
             ("occ_apply_out gray128 nonorm", (True, 128, False), False),
             ("occ_apply_out rgb128 norm ori", (False, 128, True), True),
             ("occ_apply_out rgb128 norm", (False, 128, True), False),
             ("occ_apply_out rgb112 norm ori", (False, 112, True), True)]
    runs = []
    for name, sw, want_ori in cases:
        gray, out_size, use_norm = sw or (False, None, True)
        desc = data.draw(n, 1234, 0, a.mode, size=h, device=src.device, out_size=out_size)
        oh, ow = data._out_hw(out_size, h, w)
        ch = 1 if gray else 3
        img = torch.empty(n, ch, oh, ow, device=src.device)
        ori = torch.empty(n, ch, oh, ow, device=src.device) if want_ori else None
        msk = torch.empty(n, oh, ow, dtype=torch.int64, device=src.device)
        if sw is None:
            args = ("msml_occ_apply", src, desc, img, msk, ori, n, h, w, 1)
        else:
            args = ("msml_occ_apply_out", src, desc, None, 0, data._out_table(w, ow, src.device),
                    data._out_table(h, oh, src.device), img, msk, ori, n, h, w, oh, ow, int(gray), int(use_norm), 1)
        runs.append((name, lambda args=args: call(*args), algorithmic_bytes(n, h, w, oh, ow, ch, want_ori), []))
    for _, fn, _, _ in runs:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for _, fn, _, times in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / a.launches)
    lines = []
    for name, _, nbytes, times in runs:
        ms = statistics.median(times)
        lines.append({"case": name, "batch": n, "mode": a.mode, "ms": round(ms, 4), "ms_min": round(min(times), 4),
                      "ms_max": round(max(times), 4), "algorithmic_bytes": nbytes,
                      "GB_per_s": round(nbytes / ms / 1e6, 1), "images_per_s": round(n / ms * 1e3)})
    rate = {ln["case"]: ln["GB_per_s"] for ln in lines}
    for ln in lines:
        if ln["case"].startswith("occ_apply_out"):
            ref = "occ_apply rgb112 norm ori" if ln["case"].endswith("ori") else "occ_apply rgb112 norm"
            ln["yardstick"] = ref
            ln["rate_over_yardstick"] = round(ln["GB_per_s"] / rate[ref], 3)
            ln["miss"] = ln["rate_over_yardstick"] < 0.8
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "launches": a.launches, "warmup": a.warmup,
                       "rounds": a.rounds, "timing": "device events around the launches of the entry point "
                       "(outputs preallocated, light on), median of the rounds", "cases": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
