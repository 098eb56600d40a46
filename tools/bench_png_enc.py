"""Time the PNG encoder (msml_png_encode, csrc/png_enc.hip): 256 faces of 112 x 112 RGB (a smooth random field plus
noise, --distinct different images cycled) and one 1000 x 750 photograph-sized image of the same kind.  Every figure is
the median of --reps calls after a warm-up, on the host clock around the call ending in a device synchronise, beside, in
the same run: (i) a device copy of the same source bytes, (ii) Pillow saving the same arrays as PNG on one host thread.
Also the total bytes against Pillow's files and against zlib.compress(filtered, 1) of the same filtered bytes (plus the
57 bytes of container).  No thresholds: the ratios are what to read.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_png_enc.py [--faces 256] [--reps 20] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import png  # noqa: E402
from tests import png_enc_cases as E  # noqa: E402


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


def make_images(distinct, h, w, noise, seed=5):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(distinct):
        low = Image.fromarray(rng.randint(0, 256, (h // 7, w // 7, 3)).astype(np.uint8))
        a = np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int64) + rng.randint(-noise, noise + 1, (h, w, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return out


def pillow_save(arrays):
    from PIL import Image
    ts, size = [], 0
    for _ in range(3):
        t = time.perf_counter()
        size = 0
        for a in arrays:
            f = io.BytesIO()
            Image.fromarray(a).save(f, "PNG")
            size += f.tell()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e6, size


def row(name, arrays, reps):
    x = torch.from_numpy(np.stack(arrays)).cuda()
    plan = png._plan([tuple(x.shape[1:3])] * x.shape[0], 3)
    caps = plan.bounds
    slots = torch.from_numpy(np.stack([np.cumsum(caps) - caps, caps], 1)).cuda()
    dst = torch.empty(int(caps.sum()), dtype=torch.uint8, device="cuda")
    ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device="cuda")
    meta = png.packed.uniform_meta(x.shape[0], x.shape[1], x.shape[2], 3, x.device)
    length = torch.empty(x.shape[0], dtype=torch.int32, device="cuda")
    status = torch.empty_like(length)
    flat = x.reshape(-1)
    enc_us, enc_min = timed(lambda: png.encode_into(flat, meta, dst, slots, 3, length=length, status=status, ws=ws, plan=plan), reps)
    batch_us, _ = timed(lambda: png.encode_batch(x), reps)
    y = torch.empty_like(x)
    copy_us, _ = timed(lambda: y.copy_(x), reps)
    assert int(status.abs().sum()) == 0
    ours = int(length.sum())
    pil_us, pil_bytes = pillow_save(arrays)
    distinct = {a.tobytes(): a for a in arrays}
    z1 = {k: len(zlib.compress(E.filtered_bytes(a), 1)) + 57 for k, a in distinct.items()}
    z1_bytes = sum(z1[a.tobytes()] for a in arrays)
    return {"case": name, "images": len(arrays), "size": list(x.shape[1:3]), "encode_into_us": round(enc_us, 1),
            "encode_into_min_us": round(enc_min, 1), "encode_batch_us": round(batch_us, 1), "device_copy_us": round(copy_us, 1),
            "pillow_one_thread_us": round(pil_us, 1), "pillow_over_device": round(pil_us / enc_us, 2),
            "bytes": ours, "pillow_bytes": pil_bytes, "zlib1_bytes": z1_bytes, "raw_bytes": int(x.numel()),
            "bytes_over_pillow": round(ours / pil_bytes, 4), "bytes_over_zlib1": round(ours / z1_bytes, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    faces = make_images(a.distinct, 112, 112, 6)
    rows = [row("faces", [faces[i % a.distinct] for i in range(a.faces)], a.reps),
            row("photo", make_images(1, 750, 1000, 6, seed=9), a.reps)]
    line = json.dumps({"bench": "png_enc", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
