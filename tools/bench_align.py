"""Time the face alignment kernels (csrc/align.hip) at an IJB-like size on synthetic data: --images sources of
--size x --size BGR bytes under random similarity draws (tests/align_cases.random_landmarks) -> 112 x 112 faces ->
[2N][3][112][112] f32 input pairs.  Every stage is timed with events after a warm-up (median of --reps) beside a device
copy that moves the same number of bytes (read + write) in the same run; the ratio to that copy is what to read, the
absolute numbers move with the clock.  The warp's byte count is what it MUST move (every source byte once + the output);
a face that covers part of its source touches less.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_align.py [--images 1024 --size 300 --out-size 112] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import data, ijb  # noqa: E402
from msml_amd._lib import call  # noqa: E402
from tests import align_cases as A  # noqa: E402


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


def copy_of(nbytes, reps):
    """A device-to-device copy that reads nbytes / 2 and writes nbytes / 2."""
    half = max(4, int(nbytes) // 2 // 4 * 4)
    a = torch.empty(half, dtype=torch.uint8, device="cuda").random_(0, 256)
    b = torch.empty_like(a)
    return timed(lambda: b.copy_(a), reps)


def stage(name, t, nbytes, reps, note=""):
    med, low = t
    cmed, clow = copy_of(nbytes, reps)
    return {"stage": name, "us": round(med, 1), "us_min": round(low, 1), "bytes": int(nbytes),
            "GB/s": round(nbytes / med / 1e3, 1), "copy_us": round(cmed, 1), "copy_us_min": round(clow, 1),
            "ratio_to_copy": round(med / cmed, 2), "note": note}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--size", type=int, default=300)
    ap.add_argument("--out-size", type=int, default=112)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    n, s, o = a.images, a.size, a.out_size
    rng = np.random.default_rng(1)
    lm, _ = A.random_landmarks(rng, n, (s, s))
    minv = torch.from_numpy(ijb.invert_matrices(ijb.align_matrices(lm, o))).cuda()
    src = torch.empty(n * s * s * 3, dtype=torch.uint8, device="cuda").random_(0, 256)
    meta = np.empty((n, 4), np.int64)
    meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3] = np.arange(n) * (s * s * 3), s, s, 3 * s
    assert (meta[:, 0] % 4 == 0).all()
    meta = torch.from_numpy(meta).cuda()
    faces = torch.empty(n, o, o, 3, dtype=torch.uint8, device="cuda")
    rows = []
    t = timed(lambda: call("msml_align_warp", src, meta, minv, faces, n, o, o, 1), a.reps)
    covered = float((faces != 0).any(-1).float().mean())
    rows.append(stage("align_warp", t, src.numel() + faces.numel(), a.reps,
                      "bytes = every source byte once + the output; %.0f %% of the output pixels see the source" % (100 * covered)))
    rows.append(stage("align_warp (output bytes x 5: four taps in, one out)", t, 5 * faces.numel(), a.reps,
                      "the bytes the lanes REQUEST"))
    desc = data.draw(n, 1, 0, mode="block", lo=40, hi=41, flip=False, size=o)
    pairs = torch.empty(2 * n, 3, o, o, dtype=torch.float32, device="cuda")
    t = timed(lambda: call("msml_align_pairs", faces, desc, pairs, n, o, o), a.reps)
    rows.append(stage("align_pairs", t, faces.numel() + pairs.numel() * 4 + desc.numel() * 4, a.reps))
    t = timed(lambda: ijb.eval_inputs(ijb.align_faces(src, meta.cpu().numpy(), ijb.align_matrices(lm, o), o), 1, 0, 40, 41),
              max(3, a.reps // 4))
    res = {"device": torch.cuda.get_device_name(0), "images": n, "source": [s, s], "out_size": o, "reps": a.reps,
           "python_path_us (matrices + meta check + uploads + draw + 2 kernels)": round(t[0], 1), "stages": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
