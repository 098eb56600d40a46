"""Scores of the occlusion segmentation branch on the device (csrc/segeval.hip).  The reference only looks at the branch
by eye: train.py:357-364 saves `_seg.jpg` beside `_gt_occ.jpg`, eval/qeval_mxnet.py:350-363 `_learned.jpg` beside
`_truth.jpg`.  Here:

* `mask_counts` / `metrics_from_counts` / `SegMeter`: per-image confusion counts (tp, fp, fn, tn; positive = occluded) of a
  predicted mask against the ground truth in one launch, and the pixel metrics that follow from them on the host;
* `label_blobs` / `blob_table` / `blob_detection`: connected components of the occluded pixels (the `blobs` of
  tricks/consensus_loss.py:83), their area, overlap and bounding box, and blob-level detection / false-alarm rates.

A MASK is `final_seg`-style logits [N][2][H][W] (f32 or bf16, contiguous; a pixel is clean iff channel 1 > channel 0, as
functional.mask_index and train.py:357's max(0)[1]) or an index mask [N][H][W] (uint8 or int64; 0 = occluded, the `msk` of
data.augment).  Arguments are checked on the host (ValueError) before anything is launched; only `SegMeter.compute` and
`blob_detection` wait for the device.
"""
import numpy as np
import torch

from ._lib import call

KINDS = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2, torch.int64: 3}      # MSML_SEG_* of include/msml_hip.h
MAX_SIDE = 256
MAX_LABEL_PIXELS = 16384
MAX_CAP = 1024
COUNT_NAMES = ("tp", "fp", "fn", "tn")


def _mask(who, name, t, logits_ok=True):
    """(kind, N, H, W) of a mask argument, or ValueError."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a tensor" % (who, name))
    if t.dtype not in KINDS:
        raise ValueError("%s: %s has dtype %s (logits: float32, bfloat16; index masks: uint8, int64)" % (who, name, t.dtype))
    logits = t.dtype in (torch.float32, torch.bfloat16)
    if logits and not logits_ok:
        raise ValueError("%s: %s must be an index mask (uint8 or int64), not %s" % (who, name, t.dtype))
    if logits and not (t.dim() == 4 and t.shape[1] == 2):
        raise ValueError("%s: %s logits must be [N][2][H][W], got %s" % (who, name, tuple(t.shape)))
    if not logits and t.dim() != 3:
        raise ValueError("%s: %s index mask must be [N][H][W], got %s" % (who, name, tuple(t.shape)))
    n, h, w = t.shape[0], t.shape[-2], t.shape[-1]
    if n < 1 or not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError("%s: %s is %d images of %d x %d: N >= 1, sides 1..%d" % (who, name, n, h, w, MAX_SIDE))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))
    return KINDS[t.dtype], n, h, w


def _on_device(who, *tensors):
    """The last host check: everything on one GPU."""
    if not all(t.is_cuda for t in tensors):
        raise ValueError("%s: the masks must be on the device" % who)
    if any(t.device != tensors[0].device for t in tensors):
        raise ValueError("%s: the masks are on different devices" % who)


def _same_size(who, a, b, names):
    if a[1:] != b[1:]:
        raise ValueError("%s: %s is %d x %d x %d but %s is %d x %d x %d (a mask is not resized)"
                         % ((who, names[0]) + a[1:] + (names[1],) + b[1:]))


def mask_counts(pred, gt, total=None):
    """Confusion counts of the predicted mask against the ground truth: int64 [N][4] = (tp, fp, fn, tn) per image on the
    device, positive = occluded (msml_seg_counts, one launch).  pred: a mask of any form; gt: an index mask of the same
    N, H, W.  total: int64 [4] on the device, which the launch ADDS the sums over the N images to.  No synchronisation."""
    p = _mask("mask_counts", "pred", pred)
    g = _mask("mask_counts", "gt", gt, logits_ok=False)
    _same_size("mask_counts", p, g, ("pred", "gt"))
    _on_device("mask_counts", pred, gt)
    if total is not None and not (isinstance(total, torch.Tensor) and total.dtype == torch.int64
                                  and tuple(total.shape) == (4,) and total.is_contiguous() and total.device == pred.device):
        raise ValueError("mask_counts: total must be a contiguous int64 [4] tensor on pred's device")
    counts = torch.empty(p[1], 4, dtype=torch.int64, device=pred.device)
    call("msml_seg_counts", pred, p[0], gt, g[0], counts, total, p[1], p[2], p[3])
    return counts


def _ratio(num, den):
    return float(num) / float(den) if den > 0 else float("nan")


def metrics_from_counts(counts):
    """The pixel metrics of (tp, fp, fn, tn) counts, [4] or [N][4] (a tensor, which is copied to the host, or an array),
    in f64 on the host.  [N][4] is pooled over the images first.  A zero denominator gives NaN for that entry.
    pixel_acc = (tp + tn) / all, iou_occ = tp / (tp + fp + fn), iou_clean = tn / (tn + fp + fn), miou = the mean of the
    defined ones of the two, dice_occ = 2 tp / (2 tp + fp + fn), precision = tp / (tp + fp), recall = tp / (tp + fn),
    false_alarm = fp / (fp + tn).  For [N][4] also image_iou_occ, the mean of the per-image iou_occ over the images with
    tp + fp + fn > 0, and images_defined, their number."""
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts)
    if c.dtype.kind not in "iu" or c.shape[-1:] != (4,) or c.ndim not in (1, 2):
        raise ValueError("metrics_from_counts: integer counts [4] or [N][4], got %s %s" % (c.dtype, c.shape))
    c = c.astype(np.int64)
    tp, fp, fn, tn = (int(v) for v in (c.sum(0) if c.ndim == 2 else c))
    out = {"tp": tp, "fp": fp, "fn": fn, "tn": tn,
           "pixel_acc": _ratio(tp + tn, tp + fp + fn + tn),
           "iou_occ": _ratio(tp, tp + fp + fn),
           "iou_clean": _ratio(tn, tn + fp + fn),
           "dice_occ": _ratio(2 * tp, 2 * tp + fp + fn),
           "precision": _ratio(tp, tp + fp),
           "recall": _ratio(tp, tp + fn),
           "false_alarm": _ratio(fp, fp + tn)}
    defined = [v for v in (out["iou_occ"], out["iou_clean"]) if v == v]
    out["miou"] = sum(defined) / len(defined) if defined else float("nan")
    if c.ndim == 2:
        den = c[:, 0] + c[:, 1] + c[:, 2]
        ok = den > 0
        out["images_defined"] = int(ok.sum())
        out["image_iou_occ"] = float(np.mean(c[ok, 0].astype(np.float64) / den[ok].astype(np.float64))) if ok.any() \
            else float("nan")
    return out


class SegMeter:
    """Running pixel metrics of a training or evaluation loop: update(final_seg, msk) adds the batch's counts into an int64
    [4] total on the device without waiting for it; compute() copies the total to the host (the only synchronising call)
    and returns metrics_from_counts of it; reset() zeroes it."""

    def __init__(self):
        self.total = None

    def update(self, pred, gt):
        if self.total is None:
            _mask("SegMeter.update", "pred", pred)
            _on_device("SegMeter.update", pred)
            self.total = torch.zeros(4, dtype=torch.int64, device=pred.device)
        return mask_counts(pred, gt, total=self.total)

    def compute(self):
        return metrics_from_counts(np.zeros(4, np.int64) if self.total is None else self.total)

    def reset(self):
        if self.total is not None:
            self.total.zero_()


def _check_blob_args(who, connectivity, cap=1):
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity %r is not 4 or 8" % (who, connectivity))
    if not 1 <= int(cap) <= MAX_CAP:
        raise ValueError("%s: cap %r outside 1..%d" % (who, cap, MAX_CAP))


def _label(who, mask, connectivity, want_labels=True):
    k, n, h, w = _mask(who, "mask", mask)
    if h * w > MAX_LABEL_PIXELS:
        raise ValueError("%s: %d x %d images have more than %d pixels" % (who, h, w, MAX_LABEL_PIXELS))
    _on_device(who, mask)
    labels = torch.empty(n, h, w, dtype=torch.int32, device=mask.device) if want_labels else None
    count = torch.empty(n, dtype=torch.int32, device=mask.device)
    status = torch.empty(n, dtype=torch.int32, device=mask.device)
    call("msml_seg_label", mask, k, labels, count, status, n, h, w, int(connectivity))
    return labels, count, status


def label_blobs(mask, connectivity=8):
    """Connected components of the OCCLUDED pixels of a mask (msml_seg_label): (labels int32 [N][H][W]: 0 on clean pixels,
    1..K on the components, numbered in raster order of each component's first pixel as scipy.ndimage.label numbers them;
    count int32 [N] = K; status int32 [N], 0 = ok).  H W <= 16384.  No synchronisation."""
    _check_blob_args("label_blobs", connectivity)
    return _label("label_blobs", mask, connectivity)


def blob_table(mask_a, mask_b, connectivity=8, cap=64):
    """Per-component statistics of mask A against mask B (msml_seg_label + msml_seg_blob_table): (table int32 [N][cap][6],
    count, status).  Row k - 1 of image n is (area, hit, x0, y0, x1, y1) of A's component k: its pixels, how many of them
    are occluded in B, its inclusive bounding box; rows from min(count, cap) on are zeros, and count > cap says that the
    table overflowed.  No synchronisation."""
    _check_blob_args("blob_table", connectivity, cap)
    a = _mask("blob_table", "mask_a", mask_a)
    b = _mask("blob_table", "mask_b", mask_b)
    _same_size("blob_table", a, b, ("mask_a", "mask_b"))
    if a[2] * a[3] > MAX_LABEL_PIXELS:
        raise ValueError("blob_table: %d x %d images have more than %d pixels" % (a[2], a[3], MAX_LABEL_PIXELS))
    _on_device("blob_table", mask_a, mask_b)
    labels, count, status = _label("blob_table", mask_a, connectivity)
    table = torch.empty(a[1], int(cap), 6, dtype=torch.int32, device=mask_a.device)
    call("msml_seg_blob_table", labels, count, mask_b, b[0], table, a[1], a[2], a[3], int(cap))
    return table, count, status


def blob_totals(pred, gt, tau=0.5, min_area=1, connectivity=8, cap=64):
    """The device half of blob_detection, without synchronisation: (totals int64 [N][4] = n_gt, n_found, n_pred, n_false
    of every image, on the device; over bool [N]: the image has more than `cap` components in either mask, so its row
    counts only the first `cap` of them; failed bool [N]: a labelling status other than 0).  The caller refuses or
    leaves out the images of `over` and refuses those of `failed`."""
    if not 0.0 <= float(tau) <= 1.0:
        raise ValueError("blob_detection: tau = %r is not in 0..1" % (tau,))
    tg, cg, sg = blob_table(gt, pred, connectivity, cap)
    tp, cp, sp = blob_table(pred, gt, connectivity, cap)
    out = []
    for t in (tg, tp):
        area, hit = t[:, :, 0], t[:, :, 1]
        big = (area >= int(min_area)) & (area > 0)
        found = hit.double() >= float(tau) * area.double()
        out += [big.sum(1), (big & found).sum(1), (big & ~found).sum(1)]
    totals = torch.stack([out[0], out[1], out[3], out[5]], 1).to(torch.int64)
    return totals, (cg > int(cap)) | (cp > int(cap)), (sg != 0) | (sp != 0)


def detection_from_totals(totals):
    """n_gt, n_found, n_pred, n_false -> the dict blob_detection returns."""
    n_gt, n_found, n_pred, n_false = (int(v) for v in totals)
    return {"n_gt": n_gt, "n_found": n_found, "n_pred": n_pred, "n_false": n_false,
            "detection_rate": _ratio(n_found, n_gt), "false_alarm_rate": _ratio(n_false, n_pred)}


def blob_detection(pred, gt, tau=0.5, min_area=1, connectivity=8, cap=64):
    """Blob-level detection of the ground-truth occluders.  A ground-truth blob (component of gt's occluded pixels) with
    area >= min_area is FOUND iff hit >= tau * area, hit = its pixels the prediction calls occluded; a predicted blob with
    area >= min_area is a FALSE ALARM iff hit < tau * area against the ground truth (both compared in f64).  pred: a mask
    of any form; gt: an index mask.  Returns n_gt, n_found, n_pred, n_false, detection_rate = n_found / n_gt and
    false_alarm_rate = n_false / n_pred (NaN without blobs).  RuntimeError naming the first image whose labelling status
    is not 0 or which has more than `cap` components in either mask.  Waits for the device."""
    _mask("blob_detection", "gt", gt, logits_ok=False)
    totals, over, failed = blob_totals(pred, gt, tau, min_area, connectivity, cap)
    raise_if_failed(failed)
    over = over.cpu().numpy()
    if over.any():
        raise RuntimeError("blob_detection: image %d has more than cap = %d components" % (int(np.flatnonzero(over)[0]), cap))
    return detection_from_totals(totals.sum(0).cpu().numpy())


def raise_if_failed(failed, index0=0):
    failed = failed.cpu().numpy()
    if failed.any():
        raise RuntimeError("blob_detection: the labelling of image %d ended with a status other than 0"
                           % (int(index0) + int(np.flatnonzero(failed)[0])))
