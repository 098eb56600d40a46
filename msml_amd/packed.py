"""The packed image buffer, the one form in which the image stages hand images of any sizes to each other: a flat uint8
buffer and meta int64 [N][4] = byte offset, H, W, row pitch in bytes.  A row holds W * channels bytes; an offset is a
multiple of 4; H and W lie in 1..32767 (cv2 saturates source coordinates to int16; that is not emulated) and a pitch
below 2^31.  This module alone knows the layout and the host check; csrc/packed_image.h is its device side.
"""
import numpy as np
import torch


def layout(heights, widths, channels=3):
    """meta [N][4] of new images packed back to back with rows of a multiple of 4 bytes, and the total length."""
    heights, widths = np.asarray(heights, np.int64).reshape(-1), np.asarray(widths, np.int64).reshape(-1)
    pitch = (channels * widths + 3) & ~3
    size = heights * pitch
    off = np.cumsum(size) - size
    return np.ascontiguousarray(np.stack([off, heights, widths, pitch], 1)), int(size.sum())


_UNIFORM_META = {}       # (n, h, w, channels, device) -> meta of a contiguous [n, h, w, channels] tensor, on the device


def uniform_meta(n, h, w, channels, device):
    """meta of a contiguous [n, h, w, channels] tensor (tight rows), on the device: uploaded once per shape."""
    key = (n, h, w, channels, device)
    m = _UNIFORM_META.get(key)
    if m is None:
        if len(_UNIFORM_META) >= 64:
            _UNIFORM_META.clear()
        meta = np.empty((n, 4), np.int64)
        meta[:, 0] = np.arange(n, dtype=np.int64) * (h * w * channels)
        meta[:, 1], meta[:, 2], meta[:, 3] = h, w, w * channels
        m = _UNIFORM_META[key] = torch.from_numpy(meta).to(device)
    return m


def check(buf, meta, who):
    """meta as contiguous int64 numpy [N][4], checked on the host against buf.numel() before anything is uploaded,
    because the 3-channel consumers (msml_align_warp, msml_det_resample, msml_img_*) cannot: offsets, pitch >= 3 W,
    sizes in 1..32767, the last byte of every image inside the buffer.  ValueError starting with `who` otherwise."""
    if not (isinstance(buf, torch.Tensor) and buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_contiguous()):
        raise ValueError("%s: buf must be a contiguous 1-D uint8 tensor" % who)
    mt = meta.cpu().numpy() if isinstance(meta, torch.Tensor) else np.asarray(meta)
    if mt.ndim != 2 or mt.shape[1] != 4 or mt.shape[0] == 0 or not np.issubdtype(mt.dtype, np.integer):
        raise ValueError("%s: meta must be [N][4] integers" % who)
    mt = np.ascontiguousarray(mt, dtype=np.int64)
    off, h, w, pitch = mt[:, 0], mt[:, 1], mt[:, 2], mt[:, 3]
    ok = (h >= 1) & (h <= 32767) & (w >= 1) & (w <= 32767) & (off >= 0) & (off % 4 == 0) & (pitch >= 3 * w)
    ok &= (pitch < 2 ** 31) & (off + (h - 1) * pitch + 3 * w <= buf.numel())
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise ValueError("%s: meta row %d (offset %d, %d x %d, pitch %d) does not describe an image inside the %d-byte "
                         "buffer" % (who, i, off[i], h[i], w[i], pitch[i], buf.numel()))
    return mt


def pack_images(images):
    """images: a list of H x W x 3 uint8 arrays as cv2.imread returns them (BGR, any sizes, any strides).  Returns
    (buf, meta): one uint8 tensor holding them back to back with tight rows (pinned when a GPU is present), and meta
    [N][4] int64 numpy = byte offset (a multiple of 4), H, W, row pitch 3 W.  Refuses an empty list, other dtypes, a
    channel count other than 3 and H or W outside 1..32767."""
    if not isinstance(images, (list, tuple)) or len(images) == 0:
        raise ValueError("pack_images: needs a non-empty list of images")
    meta = np.empty((len(images), 4), np.int64)
    off = 0
    for i, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8:
            raise ValueError("pack_images: image %d is not a uint8 array" % i)
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("pack_images: image %d has shape %s, not H x W x 3" % (i, tuple(im.shape)))
        h, w = im.shape[:2]
        if not (1 <= h <= 32767 and 1 <= w <= 32767):
            raise ValueError("pack_images: image %d is %d x %d, outside 1..32767" % (i, h, w))
        meta[i] = (off, h, w, 3 * w)
        off += (h * w * 3 + 3) & ~3
    buf = torch.empty(off, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    flat = buf.numpy()
    for i, im in enumerate(images):
        o, h, w, _ = meta[i]
        flat[o:o + h * w * 3].reshape(h, w, 3)[...] = im
    return buf, meta


def sources(images, who):
    """(buf, meta numpy int64 [N][4]) of a list of RGB uint8 arrays or of a (buf, meta) pair, through check().  Nothing
    is uploaded."""
    if isinstance(images, tuple) and len(images) == 2 and isinstance(images[0], torch.Tensor):
        buf, meta = images
    else:
        buf, meta = pack_images(list(images))
    return buf, check(buf, meta, who)


def meta_on_device(meta, n, device, who):
    """meta for a launch: a tensor must be contiguous int64 [n][4] on `device` and is taken as it is; anything else is
    uploaded (a copy from pageable memory, for which the host waits).  The device checks the rows."""
    if isinstance(meta, torch.Tensor):
        if meta.dtype != torch.int64 or tuple(meta.shape) != (n, 4) or meta.device != device or not meta.is_contiguous():
            raise ValueError("%s: a meta tensor must be contiguous int64 [%d][4] on %s" % (who, n, device))
        return meta
    meta = np.ascontiguousarray(meta, dtype=np.int64)
    if meta.shape != (n, 4):
        raise ValueError("%s: meta must be [%d][4]" % (who, n))
    return torch.from_numpy(meta).to(device)
