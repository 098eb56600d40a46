"""Time the JPEG encoder (msml_jpeg_encode, csrc/jpeg_enc.hip) on a batch of aligned faces: --n faces of 112 x 112 (a smooth
random field plus noise, --distinct different images cycled) at the two option sets that matter, quality 75 / 4:2:0
(PIL.Image.save of eval/align_dataset.py) and quality 97 / 4:2:0 (pack_img of cvt_casia_webface.py).  Every row is the
median of --reps calls of encode_into (caller-owned buffers, no allocation) after a warm-up, timed with events and
ending in a device synchronise, beside, in the same run: (i) a device copy of the same source bytes, (ii) Pillow
encoding the same images on the host, one image at a time, (iii) the mean time of each of the five kernels (from the
profiler's kernel records; null where the profiler gives none) and the device-to-host copy EncodedBatch.to_bytes makes.
The first image's bytes are checked against Pillow's.  No thresholds.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_jpeg_enc.py [--n 256] [--reps 20] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_jpeg import kernel_shares, timed  # noqa: E402
from msml_amd import jpeg, packed  # noqa: E402


def make_faces(distinct, seed=5):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(distinct):
        low = Image.fromarray(rng.randint(0, 256, (16, 16, 3)).astype(np.uint8))
        a = np.asarray(low.resize((112, 112), Image.BICUBIC)).astype(np.int64) + rng.randint(-12, 13, (112, 112, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def pillow_encode(faces, quality):
    from PIL import Image
    ims = [Image.fromarray(a) for a in faces]
    ts, out = [], None
    for _ in range(3):
        t = time.perf_counter()
        out = []
        for im in ims:
            f = io.BytesIO()
            im.save(f, "JPEG", quality=quality)
            out.append(f.getvalue())
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    pool = make_faces(a.distinct)
    faces = [pool[i % len(pool)] for i in range(a.n)]
    src = torch.from_numpy(np.stack(faces)).cuda()
    rows = []
    for quality in (75, 97):
        n = a.n
        t0 = time.perf_counter()
        plan = jpeg.EncodePlan([(112, 112)] * n, quality, "420", 0)
        plan_us = (time.perf_counter() - t0) * 1e6
        slots = np.stack([np.cumsum(plan.bounds) - plan.bounds, plan.bounds], 1)
        dst = torch.empty(int(plan.bounds.sum()), dtype=torch.uint8, device="cuda")
        ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device="cuda")
        length = torch.empty(n, dtype=torch.int32, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        meta = packed.uniform_meta(n, 112, 112, 3, src.device)
        sdev = torch.from_numpy(slots).cuda()
        flat = src.reshape(-1)

        def run():
            jpeg.encode_into(plan, flat, meta, dst, sdev, 3, "rgb", length=length, status=status, ws=ws)

        med, low = timed(run, a.reps)
        assert int(status.abs().sum()) == 0
        enc = jpeg.EncodedBatch(dst, sdev, slots, length, status, plan)
        t0 = time.perf_counter()
        streams = enc.to_bytes()
        to_bytes_us = (time.perf_counter() - t0) * 1e6
        pil_us, want = pillow_encode(faces, quality)
        assert streams == want, "the device's bytes are not Pillow's"
        other = torch.empty_like(src)
        copy_us, _ = timed(lambda: other.copy_(src), a.reps)
        rows.append({"quality": quality, "sampling": "4:2:0", "n": n, "encode_us": round(med, 1), "encode_us_min": round(low, 1),
                     "images_per_s": round(n / med * 1e6), "copy_of_source_us": round(copy_us, 1),
                     "ratio_to_copy": round(med / copy_us, 1), "pillow_one_at_a_time_us": round(pil_us, 1),
                     "plan_host_us": round(plan_us, 1), "to_bytes_us": round(to_bytes_us, 1), "source_bytes": src.numel(),
                     "stream_bytes": int(sum(len(s) for s in streams)), "slot_bytes": dst.numel(),
                     "workspace_bytes": plan.ws_bytes, "kernel_us": kernel_shares(run)})
        print(json.dumps(rows[-1]), file=sys.stderr)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
