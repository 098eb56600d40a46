"""Time the JPEG decoder (msml_jpeg_decode, csrc/jpeg.hip) on training-sized batches: 256 and 4 096 faces of 112 x 112
at quality 95, in 4:2:0 and in 4:4:4 (Pillow writes the streams: a smooth random field plus noise, --distinct different
images cycled).  Every row is the median of --reps calls after a warm-up, timed with events and ending in a device
synchronise, beside, in the same run: (i) a device copy of the output bytes, (ii) Pillow decoding the same streams on
--threads host threads, (iii) the host-to-device copy of the compressed bytes against that of the decoded bytes, the
host time of pack_jpegs (header parsing), and the share of each of the three passes (from the profiler's kernel
records; null where the profiler gives none).  No thresholds: the ratios are what to read.  Prints one JSON line;
`--out FILE` also writes it.

    python tools/bench_jpeg.py [--sizes 256,4096] [--reps 20] [--threads 16] [--out FILE]
"""
import argparse
import concurrent.futures
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import jpeg  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return float(np.median(us)), float(np.min(us))


def make_streams(distinct, subsampling, seed=5):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(distinct):
        low = Image.fromarray(rng.randint(0, 256, (16, 16, 3)).astype(np.uint8))
        a = np.asarray(low.resize((112, 112), Image.BICUBIC)).astype(np.int64) + rng.randint(-12, 13, (112, 112, 3))
        f = io.BytesIO()
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(f, "JPEG", quality=95, subsampling=subsampling)
        out.append(f.getvalue())
    return out


def pillow_decode(streams, threads):
    from PIL import Image

    def one(b):
        return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))

    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, streams[:threads]))
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            list(ex.map(one, streams, chunksize=16))
            ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6


def kernel_shares(run):
    """{kernel: mean us per call} from the profiler's kernel records of 5 calls, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                run()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "k_jpeg" in e.key:
                total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                out[e.key.split("(")[0]] = round(float(total) / max(e.count, 1), 1)
        return out or None
    except Exception as e:                                  # the profiler is a convenience of this tool only
        print("bench_jpeg: no kernel records (%r)" % (e,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    cache = jpeg.HeaderCache()           # as a RecordFaceSource keeps one: pack_jpegs_host_us is warm after the first row
    for name, sub in (("4:2:0", 2), ("4:4:4", 0)):
        pool = make_streams(a.distinct, sub)
        for n in [int(v) for v in a.sizes.split(",")]:
            streams = [pool[i % len(pool)] for i in range(n)]
            t0 = time.perf_counter()
            batch = jpeg.pack_jpegs(streams, cache)
            pack_us = (time.perf_counter() - t0) * 1e6
            out = torch.empty(n, 112, 112, 3, dtype=torch.uint8, device="cuda")
            meta = np.empty((n, 4), np.int64)
            meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3] = np.arange(n) * 112 * 112 * 3, 112, 112, 336
            ws = torch.empty(batch.ws_bytes, dtype=torch.uint8, device="cuda")
            status = torch.empty(n, dtype=torch.int32, device="cuda")

            def run():
                jpeg.decode_into(batch, out, meta, 3, "rgb", ws=ws, status=status)

            med, low = timed(run, a.reps)
            assert int(status.abs().sum()) == 0
            from PIL import Image
            assert np.array_equal(out[n - 1].cpu().numpy(), np.asarray(Image.open(io.BytesIO(streams[-1])).convert("RGB")))
            other = torch.empty_like(out)
            copy_us, _ = timed(lambda: other.copy_(out), a.reps)
            dev = torch.empty(batch.streams.numel(), dtype=torch.uint8, device="cuda")
            h2d_jpeg, _ = timed(lambda: dev.copy_(batch.streams, non_blocking=True), a.reps)
            pinned = torch.empty(out.shape, dtype=torch.uint8).pin_memory()
            h2d_raw, _ = timed(lambda: other.copy_(pinned, non_blocking=True), a.reps)
            rows.append({"sampling": name, "n": n, "decode_us": round(med, 1), "decode_us_min": round(low, 1),
                         "images_per_s": round(n / med * 1e6), "copy_of_output_us": round(copy_us, 1),
                         "ratio_to_copy": round(med / copy_us, 1), "pillow_%d_threads_us" % a.threads:
                         round(pillow_decode(streams, a.threads), 1), "pack_jpegs_host_us": round(pack_us, 1),
                         "compressed_bytes": int(sum(len(s) for s in streams)), "decoded_bytes": out.numel(),
                         "h2d_compressed_us": round(h2d_jpeg, 1), "h2d_decoded_us": round(h2d_raw, 1),
                         "workspace_bytes": batch.ws_bytes, "kernel_us": kernel_shares(run)})
            print(json.dumps(rows[-1]), file=sys.stderr)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "host_threads": a.threads, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
