"""Times Detector.detect_faces on a batch of composites beside the same three nets in plain torch on the device, driven
per image as the reference drives them (a PIL resize and a P-Net call per scale, a vectorised numpy NMS, a PIL crop per
box; box generation and the refine step come from tests/mtcnn_cases.py).

    python tools/bench_detect.py [--batch 256] [--baseline-images 256] [--min-face-size 24.5] [--repeat 20]

The input is the recorded 300 x 170 composite of tests/golden/g13_mtcnn.npz, rolled by a few pixels per copy so that
the images differ.  Prints one JSON line: images per second and milliseconds per image of both, and whether the two
found the same number of faces.  There is no pass / fail threshold.  The baseline needs Pillow; without it only the
detector is timed."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msml_amd import detect                      # noqa: E402
from tests import mtcnn_cases as M               # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def nms(boxes, threshold, mode="union"):
    """Greedy NMS, one vectorised numpy pass per pick; ties go to the higher index, as in tests/mtcnn_cases.nms."""
    if len(boxes) == 0:
        return []
    x1, y1, x2, y2, score = boxes[:, :5].T
    area = (x2 - x1 + 1.0) * (y2 - y1 + 1.0)
    ids = np.lexsort((np.arange(len(score)), score))
    pick = []
    while ids.size:
        i, ids = ids[-1], ids[:-1]
        pick.append(int(i))
        w = np.maximum(0.0, np.minimum(x2[i], x2[ids]) - np.maximum(x1[i], x1[ids]) + 1.0)
        h = np.maximum(0.0, np.minimum(y2[i], y2[ids]) - np.maximum(y1[i], y1[ids]) + 1.0)
        inter = w * h
        over = inter / np.minimum(area[i], area[ids]) if mode == "min" else inter / (area[i] + area[ids] - inter)
        ids = ids[over <= threshold]
    return pick


class TorchNets:
    """P-Net, R-Net and O-Net as plain torch calls on the device, outputs as the reference's modules give them."""

    def __init__(self, weights, device):
        self.w = [{k: torch.from_numpy(v).to(device) for k, v in d.items()} for d in weights]
        self.device = device

    @staticmethod
    def _features(x, d, convs, pools, fc):
        f = "features."
        for i in range(1, convs + 1):
            x = F.prelu(F.conv2d(x, d[f + "conv%d.weight" % i], d[f + "conv%d.bias" % i]), d[f + "prelu%d.weight" % i])
            if i in pools:
                x = F.max_pool2d(x, pools[i], 2, ceil_mode=True)
        if fc:
            x = x.transpose(3, 2).contiguous().view(x.size(0), -1)
            x = F.prelu(F.linear(x, d[f + "conv%d.weight" % fc], d[f + "conv%d.bias" % fc]), d[f + "prelu%d.weight" % fc])
        return x

    def pnet(self, x):
        d = self.w[0]
        x = self._features(x, d, 3, {1: 2}, 0)
        a = F.conv2d(x, d["conv4_1.weight"], d["conv4_1.bias"])
        return F.conv2d(x, d["conv4_2.weight"], d["conv4_2.bias"]), F.softmax(a, dim=-1)

    def rnet(self, x):
        d = self.w[1]
        x = self._features(x, d, 3, {1: 3, 2: 3}, 4)
        return F.linear(x, d["conv5_2.weight"], d["conv5_2.bias"]), F.softmax(F.linear(x, d["conv5_1.weight"], d["conv5_1.bias"]), -1)

    def onet(self, x):
        d = self.w[2]
        x = self._features(x, d, 4, {1: 3, 2: 3, 3: 2}, 5)
        return (F.linear(x, d["conv6_3.weight"], d["conv6_3.bias"]), F.linear(x, d["conv6_2.weight"], d["conv6_2.bias"]),
                F.softmax(F.linear(x, d["conv6_1.weight"], d["conv6_1.bias"]), -1))

    def crops(self, Image, img, boxes, size):
        b, win, valid = M.refine(boxes[:, :5], boxes[:, 5:9], img.shape[0], img.shape[1])
        out = np.zeros((len(b), size, size, 3), np.uint8)
        for i, (x0, y0, w, h) in enumerate(win):
            if valid[i]:
                out[i] = np.asarray(Image.fromarray(M.window(img, int(x0), int(y0), int(w), int(h))).resize((size, size),
                                                                                                        Image.BILINEAR))
        return b, torch.from_numpy(M.normalise_batch(out)).to(self.device), valid

    @torch.no_grad()
    def detect(self, Image, img, min_face_size, thr=(0.6, 0.7, 0.8), nthr=(0.7, 0.7, 0.7), factor=0.707):
        pil = Image.fromarray(img)
        per = []
        for s in M.scales(img.shape[0], img.shape[1], min_face_size, factor):
            lvl = np.asarray(pil.resize((math.ceil(img.shape[1] * s), math.ceil(img.shape[0] * s)), Image.BILINEAR))
            b, a = self.pnet(torch.from_numpy(M.normalise(lvl)[None]).to(self.device))
            boxes = M.generate_boxes(a.cpu().numpy()[0, 1], b.cpu().numpy()[0], s, thr[0])
            if len(boxes):
                per.append(boxes[nms(boxes[:, :5], 0.5)])
        if not per:
            return 0
        boxes = np.vstack(per)
        boxes = boxes[nms(boxes[:, :5], nthr[0])]
        boxes, x, valid = self.crops(Image, img, boxes, 24)
        off, prob = (t.cpu().numpy() for t in self.rnet(x))
        keep = np.nonzero((prob[:, 1] > thr[1]) & valid)[0]
        boxes, off = boxes[keep], off[keep]
        boxes[:, 4] = prob[keep, 1]
        keep = nms(boxes, nthr[1])
        boxes, x, valid = self.crops(Image, img, np.hstack([boxes[keep], off[keep]]), 48)
        if len(boxes) == 0:
            return 0
        lm, off, prob = (t.cpu().numpy() for t in self.onet(x))
        keep = np.nonzero((prob[:, 1] > thr[2]) & valid)[0]
        boxes = M.calibrate(boxes[keep], off[keep])
        boxes[:, 4] = prob[keep, 1]
        return len(nms(boxes, nthr[2], "min"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--baseline-images", type=int, default=256)
    ap.add_argument("--min-face-size", type=float, default=24.5)
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    with np.load(os.path.join(GOLDEN, "g13_mtcnn.npz")) as z:
        composite = z["composite"]
    images = [np.ascontiguousarray(np.roll(composite, (i % 3, i % 5), (0, 1))) for i in range(a.batch)]
    weights = detect.load_weights(GOLDEN)
    det = detect.Detector(weights)
    res = det.detect_faces(images, min_face_size=a.min_face_size)            # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        res = det.detect_faces(images, min_face_size=a.min_face_size)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t_dev = float(np.median(times))
    faces = [len(b) for b in res.boxes]
    out = {"batch": a.batch, "min_face_size": a.min_face_size, "device": torch.cuda.get_device_name(0),
           "detector_ms_per_image": 1e3 * t_dev / a.batch, "detector_img_per_s": a.batch / t_dev,
           "faces": int(sum(faces)), "dropped": res.dropped}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None and a.baseline_images > 0:
        nets = TorchNets(weights, det.device)
        n = min(a.baseline_images, a.batch)
        nets.detect(Image, images[0], a.min_face_size)                       # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = [nets.detect(Image, im, a.min_face_size) for im in images[:n]]
        torch.cuda.synchronize()
        t_ref = time.perf_counter() - t0
        out.update({"baseline_images": n, "baseline_ms_per_image": 1e3 * t_ref / n, "baseline_img_per_s": n / t_ref,
                    "same_face_counts": found == faces[:n], "speedup": (t_ref / n) / (t_dev / a.batch)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
