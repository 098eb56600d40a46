"""Time the facial-mask branch of the device input pipeline (msml_occ_draw_mask + msml_occ_apply_mask, csrc/occ.hip):
`augment` at --batch with p_mask 0 and p_mask 0.2 (and 1, the overlay on every sample) in the two recipes -- RGB at the
source size with Normalize, and gray, 128 x 128, unnormalised -- on the synthetic renders of SynthFaceSource(masks=True).
Every row is timed with events after a warm-up (median of --reps) beside a device copy of the bytes the call must move
(the faces, the renders of the flagged samples, img, msk, ori) in the same run; the ratio to that copy is what to read,
the absolute numbers move with the clock.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_maskaug.py [--batch 256] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import data  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    n = a.batch
    faces, masked, mask, _ = (t.cuda() for t in data.SynthFaceSource(n, 1000, pool=1, masks=True).pool[0])
    rows = []
    for name, kw, ch, o in (("rgb 112 norm", {}, 3, 112), ("gray 128", {"gray": True, "out_size": 128, "use_norm": False}, 1, 128)):
        base = None
        for p in (0.0, 0.2, 1.0):
            flagged = int(data.mask_flags(1, 0, n, p).sum())
            t = timed(lambda: data.augment(faces, 1, 0, "train", p_mask=p, masked=masked, mask=mask, **kw), a.reps)
            nbytes = faces.numel() + flagged * 112 * 112 * 4 + n * o * o * (2 * ch * 4 + 8) + flagged * o * o * (ch * 4 + 8)
            cmed, clow = copy_of(nbytes, a.reps)
            base = t[0] if base is None else base
            rows.append({"recipe": name, "p_mask": p, "flagged": flagged, "us": round(t[0], 1), "us_min": round(t[1], 1),
                         "us_over_p_mask_0": round(t[0] - base, 1), "bytes": int(nbytes), "copy_us": round(cmed, 1),
                         "ratio_to_copy": round(t[0] / cmed, 2)})
    res = {"device": torch.cuda.get_device_name(0), "batch": n, "reps": a.reps, "rows": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
