"""Times msml_img_orient, msml_img_resize and mtcnn_align.align_multi beside a device-to-device copy of the same bytes.

    python tools/bench_mtcnn_align.py [--batch 256] [--repeat 20]

The input is the recorded 300 x 170 composite of tests/golden/g13_mtcnn.npz, rolled by a few pixels per copy so that
the images differ.  orient: ROTATE_90 of every image; resize: 300 x 170 -> 320 x 181 bicubic, the fast-mode step of
align_fully (coefficient tables cached after the warm-up).  The copy moves the bytes a kernel reads plus the bytes it
writes (for the resize: source + intermediate written and read + destination), so `x_copy` is the kernel's time over
the time a plain copy needs for its traffic.  align_multi is timed whole (detector, host fit, warp) beside detect_faces
alone.  Prints one JSON line.  There is no pass / fail threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msml_amd import detect, ijb, mtcnn_align as MA        # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def copy_time(nbytes, repeat):
    """A device-to-device copy that reads and writes nbytes / 2 each."""
    a = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    return timed(lambda: b.copy_(a), repeat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    with np.load(os.path.join(GOLDEN, "g13_mtcnn.npz")) as z:
        composite = z["composite"]
    images = [np.ascontiguousarray(np.roll(composite, (i % 3, i % 5), (0, 1))) for i in range(a.batch)]
    buf, meta = ijb.pack_images(images)
    packed = (buf.cuda(), meta)
    src_bytes = int(buf.numel())
    out = {"batch": a.batch, "device": torch.cuda.get_device_name(0), "source_bytes": src_bytes}

    methods = np.full(a.batch, MA.ROTATE_90, np.int64)
    t = timed(lambda: MA.img_orient(packed, methods), a.repeat)
    dst_bytes = int(MA.img_orient(packed, methods)[0].numel())
    c = copy_time(src_bytes + dst_bytes, a.repeat)
    out.update(orient_us_per_image=1e6 * t / a.batch, orient_gb_per_s=(src_bytes + dst_bytes) / t / 1e9,
               orient_x_copy=t / c)

    sizes = np.array([(320, 181)], np.int64).repeat(a.batch, 0)
    t = timed(lambda: MA.img_resize(packed, sizes, MA.BICUBIC), a.repeat)
    dst_bytes = int(MA.img_resize(packed, sizes, MA.BICUBIC)[0].numel())
    inter = a.batch * 170 * 960
    traffic = src_bytes + 2 * inter + dst_bytes
    c = copy_time(traffic, a.repeat)
    out.update(resize_us_per_image=1e6 * t / a.batch, resize_gb_per_s=traffic / t / 1e9, resize_x_copy=t / c)

    det = detect.Detector(detect.load_weights(GOLDEN))
    t_det = timed(lambda: det.detect_faces(packed, 24.5), a.repeat)
    t_all = timed(lambda: MA.align_multi(det, packed, min_face_size=24.5), a.repeat)
    crops = MA.align_multi(det, packed, min_face_size=24.5)[0]
    t_full = timed(lambda: MA.align_fully(det, packed), max(1, a.repeat // 4))
    out.update(detect_ms_per_image=1e3 * t_det / a.batch, align_multi_ms_per_image=1e3 * t_all / a.batch,
               align_multi_over_detect=t_all / t_det, faces=int(sum(c.shape[0] for c in crops)),
               align_fully_ms_per_image=1e3 * t_full / a.batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
