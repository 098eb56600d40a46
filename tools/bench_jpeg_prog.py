"""Time progressive JPEG decoding (msml_jpeg_decode_scans, csrc/jpeg.hip k_jpeg_prog) beside the baseline decoder on
the same images: 256 faces of 112 x 112 in 4:2:0 at quality 95 as Pillow writes them progressive, and one 1000 x 750
photograph (a smooth random field plus noise; Pillow writes both kinds of file from the same pixels).  Every row is the
median of --reps calls after a warm-up, timed with events and ending in a device synchronise, and holds, from the same
run: the progressive batch through msml_jpeg_decode_scans, the baseline files of the same images through
msml_jpeg_decode, those baseline files packed with progressive=True (the new door: no scan table, the same entry),
Pillow decoding either kind on ONE host thread, the host time of pack_jpegs, and the share of each kernel (from the
profiler's kernel records; null where the profiler gives none).  No thresholds.  Prints one JSON line; `--out FILE`
also writes it.

    python tools/bench_jpeg_prog.py [--faces 256] [--reps 20] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from bench_jpeg import kernel_shares, timed  # noqa: E402
from msml_amd import jpeg  # noqa: E402


def make_pairs(count, w, h, seed=5):
    """[(progressive bytes, baseline bytes)] of `count` images, quality 95, 4:2:0."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        low = Image.fromarray(rng.randint(0, 256, (max(2, h // 7), max(2, w // 7), 3)).astype(np.uint8))
        a = np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int64) + rng.randint(-12, 13, (h, w, 3))
        im = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
        pair = []
        for progressive in (True, False):
            f = io.BytesIO()
            im.save(f, "JPEG", quality=95, subsampling=2, progressive=progressive)
            pair.append(f.getvalue())
        out.append(tuple(pair))
    return out


def pillow_one_thread(streams):
    from PIL import Image
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        for b in streams:
            np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def measure(streams, h, w, reps, progressive):
    from PIL import Image
    n = len(streams)
    t0 = time.perf_counter()
    batch = jpeg.pack_jpegs(streams, progressive=progressive)
    pack_us = (time.perf_counter() - t0) * 1e6
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda")
    meta = np.empty((n, 4), np.int64)
    meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3] = np.arange(n) * h * w * 3, h, w, w * 3
    ws = torch.empty(batch.ws_bytes, dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")

    def run():
        jpeg.decode_into(batch, out, meta, 3, "rgb", ws=ws, status=status)

    med, low = timed(run, reps)
    assert int(status.abs().sum()) == 0
    assert np.array_equal(out[n - 1].cpu().numpy(), np.asarray(Image.open(io.BytesIO(streams[-1])).convert("RGB")))
    return {"decode_us": round(med, 1), "decode_us_min": round(low, 1), "images_per_s": round(n / med * 1e6),
            "pack_jpegs_host_us": round(pack_us, 1), "compressed_bytes": int(sum(len(s) for s in streams)),
            "scans": 0 if batch.scans is None else int(batch.scans.shape[0]), "kernel_us": kernel_shares(run)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for name, n, w, h, distinct in (("faces", a.faces, 112, 112, a.distinct), ("photograph", 1, 1000, 750, 1)):
        pool = make_pairs(min(distinct, n), w, h)
        prog = [pool[i % len(pool)][0] for i in range(n)]
        base = [pool[i % len(pool)][1] for i in range(n)]
        row = {"case": name, "n": n, "width": w, "height": h,
               "progressive": measure(prog, h, w, a.reps, True),
               "baseline": measure(base, h, w, a.reps, False),
               "baseline_through_progressive_door": measure(base, h, w, a.reps, True),
               "pillow_1_thread_progressive_us": round(pillow_one_thread(prog), 1),
               "pillow_1_thread_baseline_us": round(pillow_one_thread(base), 1)}
        row["progressive_to_baseline"] = round(row["progressive"]["decode_us"] / row["baseline"]["decode_us"], 2)
        row["pillow_1_thread_to_progressive"] = round(row["pillow_1_thread_progressive_us"] / row["progressive"]["decode_us"], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
