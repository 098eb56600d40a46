"""Time the PNG decoder (msml_png_decode, csrc/png.hip): 256 faces of 112 x 112 RGB as Pillow writes them at its
default level, and one batch of 1000 x 750 photographs (a smooth random field plus noise, --distinct different images
cycled).  Every row is the median of --reps calls after a warm-up, on the host clock ending in a device synchronise,
beside, in the same run: (i) a device copy of the same decoded bytes, (ii) Pillow decoding the same files on the host
one at a time, (iii) the host time of pack_pngs (chunk walk and CRCs) and the share of each of the three passes (from
the profiler's kernel records; null where the profiler gives none).  No thresholds: the ratios are what to read.
Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_png.py [--faces 256] [--photos 16] [--reps 20] [--out FILE]
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
sys.path.insert(0, ROOT)

from msml_amd import png  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t) * 1e6)
    return float(np.median(us)), float(np.min(us))


def make_streams(distinct, h, w, noise, seed=5):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(distinct):
        low = Image.fromarray(rng.randint(0, 256, (h // 7, w // 7, 3)).astype(np.uint8))
        a = np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int64) + rng.randint(-noise, noise + 1, (h, w, 3))
        f = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(f, "PNG")
        out.append(f.getvalue())
    return out


def pillow_decode(streams):
    from PIL import Image
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        for b in streams:
            np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def kernel_shares(run):
    """{kernel: mean us per call} from the profiler's kernel records of 3 calls, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                run()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "k_png" in e.key:
                total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                out[e.key.split("(")[0]] = round(float(total) / max(e.count, 1), 1)
        return out or None
    except Exception as e:                                  # the profiler is a convenience of this tool only
        print("bench_png: no kernel records (%r)" % (e,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=256)
    ap.add_argument("--photos", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for name, n, h, w, noise in (("faces 112x112", a.faces, 112, 112, 12), ("photos 1000x750", a.photos, 750, 1000, 4)):
        if n < 1:
            continue
        pool = make_streams(min(a.distinct, n), h, w, noise)
        streams = [pool[i % len(pool)] for i in range(n)]
        t0 = time.perf_counter()
        batch = png.pack_pngs(streams)
        pack_us = (time.perf_counter() - t0) * 1e6
        out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda")
        meta = np.empty((n, 4), np.int64)
        meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3] = np.arange(n) * h * w * 3, h, w, w * 3
        meta = torch.from_numpy(meta).cuda()
        ws = torch.empty(batch.ws_bytes, dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        batch.to_device("cuda")

        def run():
            png.decode_into(batch, out, meta, 3, "rgb", ws=ws, status=status)

        med, low = timed(run, a.reps)
        assert int(status.abs().sum()) == 0
        from PIL import Image
        assert np.array_equal(out[n - 1].cpu().numpy(), np.asarray(Image.open(io.BytesIO(streams[-1])).convert("RGB")))
        other = torch.empty_like(out)
        copy_us, _ = timed(lambda: other.copy_(out), a.reps)
        pil_us = pillow_decode(streams)
        rows.append({"batch": name, "n": n, "decode_us": round(med, 1), "decode_us_min": round(low, 1),
                     "images_per_s": round(n / med * 1e6), "copy_of_output_us": round(copy_us, 1),
                     "ratio_to_copy": round(med / copy_us, 1), "pillow_one_at_a_time_us": round(pil_us, 1),
                     "ratio_to_pillow": round(med / pil_us, 3), "pack_pngs_host_us": round(pack_us, 1),
                     "compressed_bytes": int(sum(len(s) for s in streams)), "decoded_bytes": out.numel(),
                     "workspace_bytes": batch.ws_bytes, "kernel_us": kernel_shares(run)})
        print(json.dumps(rows[-1]), file=sys.stderr)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
