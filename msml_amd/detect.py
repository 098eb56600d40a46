"""MTCNN face detection on the device: boxes and 5-point landmarks for a batch of images of any sizes.

The reference's MTCNN.detect_faces (eval/preprocess/mtcnn.py:160-274; eval/preprocess/mtcnn_pytorch/src/first_stage.py,
box_utils.py, get_nets.py) is a per-image Python loop: a PIL resize and a P-Net call per pyramid scale, numpy NMS, a PIL
crop per box.  Here every image of a batch goes through each step in one launch (csrc/detect.hip, the msml_det_* family):
pyramid, fused P-Net, candidates, NMS per scale and per image, refine, crops, R-Net, O-Net, landmarks.  Pixel data never
returns to the host.  Five small device-to-host copies per call: the candidate counts per level (they size the candidate
rows), the survivors of stage 1 per image (they size R-Net's batch), the survivors of stage 2 per image (O-Net's batch),
and the result as its per-image offsets and its rows.

Deliberate differences from the reference, all documented where they occur:
  * an image without a detection gives (0, 5) / (0, 10) arrays (the reference: np.zeros([0]) twice);
  * a box with no pixel inside the image is dropped and counted (the reference's get_image_boxes raises there);
  * more candidates than `max_candidates` in one image is an error (MSML_ERR_CAPACITY), never a silent cut.
"""
import collections
import glob
import math
import os

import numpy as np
import torch

from . import _lib, packed
from ._lib import call

COLS = 16                      # doubles per candidate row: x1 y1 x2 y2 score | image | offsets[4] / landmarks[10]
ERR_CAPACITY = -6              # MSML_ERR_CAPACITY

Detections = collections.namedtuple("Detections", "boxes landmarks dropped")


class CapacityError(RuntimeError):
    """More candidates in one image than the fixed capacity holds; `.code` is MSML_ERR_CAPACITY."""
    code = ERR_CAPACITY


def load_weights(folder):
    """The three parameter sets (P-Net, R-Net, O-Net) as dicts of f32 arrays under the reference's parameter names.
    Reads the caller's own pnet.npy / rnet.npy / onet.npy (the pickled dicts of mtcnn_pytorch/src/weights), or, when
    those are absent, plain-array files mtcnn_{pnet,rnet,onet}*.npz, where a large array may be split row-wise over
    several files as NAME.part0, NAME.part1, ..."""
    out = []
    for name in ("pnet", "rnet", "onet"):
        path = os.path.join(folder, name + ".npy")
        if os.path.exists(path):
            d = dict(np.load(path, allow_pickle=True)[()])
        else:
            files = sorted(glob.glob(os.path.join(folder, "mtcnn_%s*.npz" % name)))
            if not files:
                raise FileNotFoundError("load_weights: neither %s nor mtcnn_%s*.npz in %s" % (name + ".npy", name, folder))
            d = {}
            for f in files:
                with np.load(f) as z:
                    d.update({k: z[k] for k in z.files})
            parts = sorted(k for k in d if ".part" in k)
            for base in sorted({k.split(".part")[0] for k in parts}):
                d[base] = np.concatenate([d.pop(k) for k in parts if k.startswith(base + ".part")], 0)
        out.append({k: np.ascontiguousarray(v, np.float32) for k, v in d.items()})
    return tuple(out)


def _conv_block(d, idx):
    f = "features."
    return [d[f + "conv%d.weight" % idx].ravel(), d[f + "conv%d.bias" % idx].ravel(), d[f + "prelu%d.weight" % idx].ravel()]


def _fc_block(d, idx, c, side):
    """Linear after Flatten: the reference flattens x.transpose(3, 2), so its feature order is (c, x, y); the device
    keeps (c, y, x), and the kernel wants [In][Out]."""
    f = "features."
    w = d[f + "conv%d.weight" % idx]
    w = w.reshape(w.shape[0], c, side, side).transpose(0, 1, 3, 2).reshape(w.shape[0], -1)
    return [np.ascontiguousarray(w.T).ravel(), d[f + "conv%d.bias" % idx].ravel(), d[f + "prelu%d.weight" % idx].ravel()]


def _heads(d, names, width):
    w = np.zeros((16, width), np.float32)
    b = np.zeros(16, np.float32)
    r = 0
    for n in names:
        k = d[n + ".weight"].shape[0]
        w[r:r + k] = d[n + ".weight"].reshape(k, width)
        b[r:r + k] = d[n + ".bias"]
        r += k
    return [np.ascontiguousarray(w.T).ravel(), b]


def pack_pnet(d):
    parts = _conv_block(d, 1) + _conv_block(d, 2) + _conv_block(d, 3)
    w = np.concatenate([d["conv4_1.weight"].reshape(2, 32), d["conv4_2.weight"].reshape(4, 32)], 0)
    parts += [w.ravel(), np.concatenate([d["conv4_1.bias"], d["conv4_2.bias"]])]
    return np.concatenate(parts).astype(np.float32)


def pack_rnet(d):
    parts = _conv_block(d, 1) + _conv_block(d, 2) + _conv_block(d, 3) + _fc_block(d, 4, 64, 3)
    return np.concatenate(parts + _heads(d, ("conv5_1", "conv5_2"), 128)).astype(np.float32)


def pack_onet(d):
    parts = (_conv_block(d, 1) + _conv_block(d, 2) + _conv_block(d, 3) + _conv_block(d, 4)
             + _fc_block(d, 5, 128, 3))
    return np.concatenate(parts + _heads(d, ("conv6_1", "conv6_2", "conv6_3"), 256)).astype(np.float32)


def pyramid_scales(height, width, min_face_size=64.0, factor=0.707):
    """detect_faces' own loop (mtcnn.py:176-196), in Python floats as there."""
    scales = []
    m = 12 / min_face_size
    length = min(height, width) * m
    count = 0
    while length > 12:
        scales.append(m * factor ** count)
        length *= factor
        count += 1
    return scales


def pnet_out(n):
    """P-Net's output size for an input side n: conv 3, ceil-mode pool 2, conv 3, conv 3."""
    return (n - 1) // 2 - 4


class Detector:
    """MTCNN with its parameters packed once on the device.  weights: load_weights' result."""

    def __init__(self, weights, device="cuda"):
        pw, rw, ow = weights
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("Detector: needs a GPU device; msml_amd has no other compute path")
        self.pnet = torch.from_numpy(pack_pnet(pw)).to(self.device)
        self.rnet = torch.from_numpy(pack_rnet(rw)).to(self.device)
        self.onet = torch.from_numpy(pack_onet(ow)).to(self.device)
        if self.pnet.numel() != _lib.value("msml_det_pnet_params"):
            raise ValueError("Detector: P-Net has %d parameters, not %d" % (self.pnet.numel(),
                                                                           _lib.value("msml_det_pnet_params")))
        for net, p in ((0, self.rnet), (1, self.onet)):
            if p.numel() != _lib.value("msml_det_net_params", net):
                raise ValueError("Detector: net %d has %d parameters, not %d" % (net, p.numel(),
                                                                               _lib.value("msml_det_net_params", net)))
        self.tile = _lib.value("msml_det_pnet_tile")
        self.nms_capacity = _lib.value("msml_det_nms_capacity")

    # -- helpers --------------------------------------------------------------------------------------------------

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def resample(self, src, meta_dev, jobs, out, max_px):
        call("msml_det_resample", src, meta_dev, jobs, out, jobs.shape[0], int(max_px))

    def run_pnet(self, pyr, levels):
        """levels: int64 numpy [L][6] = input offset, H, W, output offset, oh, ow.  Returns the maps buffer."""
        t = self.tile
        tx = -(-levels[:, 5] // t)
        per_level = -(-levels[:, 4] // t) * tx
        first = np.cumsum(per_level) - per_level
        within = np.arange(int(per_level.sum())) - np.repeat(first, per_level)
        tx = np.repeat(tx, per_level)
        tiles = np.stack([np.repeat(np.arange(levels.shape[0]), per_level), within // tx, within % tx], 1).astype(np.int32)
        maps = torch.empty(int(levels[-1, 3] + 6 * levels[-1, 4] * levels[-1, 5]), dtype=torch.float32, device=self.device)
        call("msml_det_pnet", pyr, self._dev(levels), self._dev(tiles), self.pnet, maps, tiles.shape[0])
        return maps

    def nms(self, rows, seg_off, valid, nseg, max_n, threshold, mode, capacity=None):
        """keep [n] int32 (-1 padded per segment) and keep_cnt [nseg] int32 of msml_det_nms."""
        n = rows.shape[0]
        order = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        keep = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        cnt = torch.zeros(max(nseg, 1), dtype=torch.int32, device=self.device)
        rc = _lib.call_status("msml_det_nms", rows, seg_off, valid, nseg, int(max_n),
                              int(self.nms_capacity if capacity is None else capacity), float(threshold),
                              1 if mode == "min" else 0, order, keep, cnt)
        if rc == ERR_CAPACITY:
            raise CapacityError("msml_det_nms failed (%d): %s" % (rc, _lib.load().msml_last_error().decode()))
        if rc != 0:
            raise RuntimeError("msml_det_nms failed (%d): %s" % (rc, _lib.load().msml_last_error().decode()))
        return keep, cnt

    def compact(self, rows, keep, seg_off, cnt, nseg, n_out=None):
        """Rows in pick order, segment after segment, and their offsets [nseg + 1] (int64, device)."""
        new_off = torch.zeros(nseg + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(cnt[:nseg], 0, out=new_off[1:])
        out = torch.empty(rows.shape[0] if n_out is None else n_out, COLS, dtype=torch.float64, device=self.device)
        call("msml_det_compact", rows, keep, seg_off, cnt, new_off, out, nseg)
        return out, new_off

    def run_net(self, net, crops, n):
        ws_bytes = _lib.value("msml_det_net_workspace", net, n)
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=self.device)
        out = torch.zeros(n, 16, dtype=torch.float32, device=self.device)
        call("msml_det_net", net, crops, self.rnet if net == 0 else self.onet, n, ws, ws_bytes, out)
        return out

    def crops(self, src, meta_dev, rows, n, size):
        """msml_det_refine on rows[:n] in place, then the size x size crops.  Returns (crops [n][3][s][s], valid [n])."""
        jobs = torch.empty(n, 8, dtype=torch.int64, device=self.device)
        valid = torch.empty(n, dtype=torch.uint8, device=self.device)
        call("msml_det_refine", rows, meta_dev, n, size, jobs, valid)
        out = torch.empty(n, 3, size, size, dtype=torch.float32, device=self.device)
        self.resample(src, meta_dev, jobs, out, size * size)
        return out, valid

    # -- the detector ---------------------------------------------------------------------------------------------

    @torch.no_grad()
    def detect_faces(self, images, min_face_size=64.0, thresholds=(0.6, 0.7, 0.8), nms_thresholds=(0.7, 0.7, 0.7),
                     factor=0.707, max_candidates=None):
        """images: a list of H x W x 3 uint8 RGB arrays of any sizes, or (buf, meta) as ijb.pack_images returns them
        (a meta row that is not an image inside buf is a ValueError before anything is uploaded).  Returns Detections(boxes, landmarks, dropped): per image boxes f64 [n][5] = x1 y1 x2 y2 score and landmarks f32
        [n][10] = x0..x4 y0..y4 in image coordinates, in the reference's order (descending score).  An image without a
        detection gives arrays of shape (0, 5) and (0, 10); the reference returns np.zeros([0]) for both there.
        dropped: the number of boxes that had no pixel inside their image after a calibration step -- the reference's
        get_image_boxes raises on such a box, here it leaves the list -- or a side of 32 768 pixels or more (the reference
        would try to allocate that cut).  max_candidates: the PER-IMAGE capacity for P-Net
        candidates (default and upper limit: msml_det_nms_capacity()); an image with more raises CapacityError, however
        many the batch holds in all.  min_face_size: one number, or one per image ([B])."""
        buf, meta = packed.sources(images, "detect_faces")     # msml_det_resample leaves the check of meta to its caller
        B = meta.shape[0]
        dev = self.device
        capacity = self.nms_capacity if max_candidates is None else int(max_candidates)
        empty = Detections([np.zeros((0, 5)) for _ in range(B)], [np.zeros((0, 10), np.float32) for _ in range(B)], 0)

        # the pyramid: one job and one P-Net level per (image, scale); the tables are built per DISTINCT image size
        if np.ndim(min_face_size) == 0:
            sizes, which = np.unique(meta[:, 1:3], axis=0, return_inverse=True)
            per_size = [pyramid_scales(int(h), int(w), min_face_size, factor) for h, w in sizes]
        else:                                                                  # one min_face_size per image
            mfs = np.asarray(min_face_size, np.float64).reshape(-1)
            if mfs.shape[0] != B or not (np.isfinite(mfs) & (mfs > 0)).all():
                raise ValueError("detect_faces: min_face_size must be one positive number, or one per image")
            keys, which = np.unique(np.concatenate([meta[:, 1:3].astype(np.float64), mfs[:, None]], 1), axis=0,
                                    return_inverse=True)
            sizes = keys[:, 0:2].astype(np.int64)
            per_size = [pyramid_scales(int(h), int(w), float(m), factor) for h, w, m in keys]
        which = which.reshape(-1)
        size_levels = np.array([len(p) for p in per_size], np.int64)
        if size_levels.sum() == 0:
            return empty
        size_first = np.cumsum(size_levels) - size_levels
        g_scale = np.array([s for p in per_size for s in p], np.float64)
        g_h = np.array([math.ceil(int(h) * s) for (h, w), p in zip(sizes, per_size) for s in p], np.int64)
        g_w = np.array([math.ceil(int(w) * s) for (h, w), p in zip(sizes, per_size) for s in p], np.int64)
        nlev = size_levels[which]                                              # levels of every image
        L = int(nlev.sum())
        owner = np.repeat(np.arange(B, dtype=np.int64), nlev)
        image_first_level = np.concatenate([[0], np.cumsum(nlev)])
        g = np.repeat(size_first[which], nlev) + np.arange(L) - np.repeat(image_first_level[:-1], nlev)
        scales, sh, sw = g_scale[g], g_h[g], g_w[g]
        oh, ow = pnet_out(sh), pnet_out(sw)
        in_off, out_off = np.cumsum(3 * sh * sw), np.cumsum(6 * oh * ow)
        in_total, in_off, out_off = int(in_off[-1]), in_off - 3 * sh * sw, out_off - 6 * oh * ow
        zeros = np.zeros(L, np.int64)
        jobs = np.stack([owner, zeros, zeros, meta[owner, 2], meta[owner, 1], sw, sh, in_off], 1)
        levels = np.stack([in_off, sh, sw, out_off, oh, ow], 1)
        src = buf if buf.is_cuda else buf.to(dev, non_blocking=True)
        meta_dev = self._dev(meta)
        pyr = torch.empty(in_total, dtype=torch.float32, device=dev)
        self.resample(src, meta_dev, self._dev(jobs), pyr, int((sw * sh).max()))
        levels_dev = self._dev(levels)
        maps = self.run_pnet(pyr, levels)

        # candidates: count, copy 1 (the per-level totals), write
        level_first_row = np.concatenate([[0], np.cumsum(oh)])
        nrows = int(level_first_row[-1])
        rowtab = np.stack([np.repeat(np.arange(L), oh), np.arange(nrows) - np.repeat(level_first_row[:-1], oh)],
                          1).astype(np.int32)
        rowtab_dev, scales_dev, owner_dev = self._dev(rowtab), self._dev(scales), self._dev(owner)
        counts = torch.empty(nrows, dtype=torch.int64, device=dev)
        args = (maps, levels_dev, scales_dev, owner_dev, rowtab_dev, nrows, float(thresholds[0]))
        call("msml_det_candidates", *args, 0, counts, None, None)
        offs = torch.zeros(nrows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=offs[1:])
        lev_off = offs[self._dev(level_first_row)]
        lev_off_host = lev_off.cpu().numpy()                                   # copy 1
        total = int(lev_off_host[-1])
        if total == 0:
            return empty
        longest = int(np.diff(lev_off_host[image_first_level]).max())          # candidates of the fullest image
        rows = torch.empty(total, COLS, dtype=torch.float64, device=dev)
        call("msml_det_candidates", *args, 1, None, offs, rows)

        # NMS inside every scale (0.5), then across the scales of an image; copy 2: the survivors of every image
        keep, cnt = self.nms(rows, lev_off, None, L, longest, 0.5, "union", capacity)
        rows, new_off = self.compact(rows, keep, lev_off, cnt, L)
        img_off = new_off[self._dev(image_first_level)]
        keep, cnt = self.nms(rows, img_off, None, B, longest, nms_thresholds[0], "union", capacity)
        per_image = cnt[:B].cpu().numpy()                                      # copy 2
        n2, longest = int(per_image.sum()), int(per_image.max())
        if n2 == 0:
            return empty
        rows, img_off = self.compact(rows, keep, img_off, cnt, B, n2)

        # stage 2: 24 x 24 crops, R-Net; copy 3: the survivors of every image and the dropped boxes
        crops, valid = self.crops(src, meta_dev, rows, n2, 24)
        dropped = (valid == 0).sum(dtype=torch.int32).reshape(1)
        net = self.run_net(0, crops, n2)
        call("msml_det_select", rows, net, n2, float(thresholds[1]), 0, valid)
        keep, cnt = self.nms(rows, img_off, valid, B, longest, nms_thresholds[1], "union", capacity)
        per_image = torch.cat([cnt[:B], dropped]).cpu().numpy()                # copy 3
        ndropped, per_image = int(per_image[B]), per_image[:B]
        n3, longest = int(per_image.sum()), int(per_image.max())
        if n3 == 0:                                                            # R-Net rejected every box of the batch
            return empty._replace(dropped=ndropped)
        rows, img_off = self.compact(rows, keep, img_off, cnt, B, n3)

        # stage 3: 48 x 48 crops, O-Net, landmarks; the result comes back as its offsets (copy 4) and its rows (copy 5)
        crops, valid = self.crops(src, meta_dev, rows, n3, 48)
        dropped = (valid == 0).sum(dtype=torch.int64).reshape(1)
        net = self.run_net(1, crops, n3)
        call("msml_det_select", rows, net, n3, float(thresholds[2]), 1, valid)
        keep, cnt = self.nms(rows, img_off, valid, B, longest, nms_thresholds[2], "min", capacity)
        rows, img_off = self.compact(rows, keep, img_off, cnt, B)
        tail = torch.cat([img_off, dropped]).cpu().numpy()                     # copy 4
        off, ndropped = tail[:B + 1], ndropped + int(tail[B + 1])
        res = rows[:int(off[-1])].cpu().numpy()                                # copy 5
        boxes = np.split(np.ascontiguousarray(res[:, 0:5]), off[1:-1])
        marks = np.split(res[:, 6:16].astype(np.float32), off[1:-1])
        return Detections(boxes, marks, ndropped)


def first_landmarks(landmarks_list):
    """The landmarks[0] pick of MTCNN.align (mtcnn.py:27-30) for every image: ([B][5][2] f32 (x, y) points, zeros where
    nothing was found; found [B] bool)."""
    out = np.zeros((len(landmarks_list), 5, 2), np.float32)
    found = np.zeros(len(landmarks_list), bool)
    for i, lm in enumerate(landmarks_list):
        if len(lm):
            out[i, :, 0], out[i, :, 1] = lm[0][0:5], lm[0][5:10]
            found[i] = True
    return out, found


@torch.no_grad()
def detect_and_embed(model, images, detector, min_face_size=64.0, thresholds=(0.6, 0.7, 0.8),
                     nms_thresholds=(0.7, 0.7, 0.7), factor=0.707, **embed):
    """Photo in, embedding out: detect_faces, first_landmarks, then ijb.align_and_embed (align_matrices, align_faces, the
    eval input pairs, the model) for the images in which a face was found.  images: cv2.imread results (BGR), as
    ijb.align_and_embed takes them; the detector sees their RGB view.  The alignment is the project's Umeyama estimate of
    ijb.align_matrices, not the reference's cp2tform / warp_and_crop_face (those: mtcnn_align.align_and_embed).  Returns (feats [F][2E] f32 on the device, one
    row per found image in order; found [B] bool; Detections).  embed: align_and_embed's batch, lo, hi, seed, out_size."""
    from . import ijb
    det = detector.detect_faces([im[:, :, ::-1] for im in images], min_face_size, thresholds, nms_thresholds, factor)
    points, found = first_landmarks(det.landmarks)
    idx = np.flatnonzero(found)
    if idx.size == 0:
        return None, found, det
    feats = ijb.align_and_embed(model, [images[i] for i in idx], points[idx], **embed)
    return feats, found, det
