"""One door for compressed images: PIL.Image.open(f).convert('RGB') of the reference (eval/qeval_folder.py:48,
eval/align_dataset.py:44) for a list of files of either format.  Each byte string is sniffed (FF D8: JPEG, the 8-byte
PNG signature: PNG), one packed destination is laid out for all of them, and msml_jpeg_decode / msml_png_decode write
their own images into it: two device calls, whatever the mix."""
import numpy as np
import torch

from . import _codec, jpeg, packed, png

UNKNOWN_FORMAT = 64          # the status of a byte string that is neither JPEG nor PNG


class DecodeError(ValueError):
    """decode_images(strict=True): image `index` could not be decoded, with the decoder's `status`."""

    def __init__(self, index, kind, status):
        super().__init__("decode_images: image %d: %s (status %d)" % (index, reason(kind, status), status))
        self.index, self.status = int(index), int(status)


def sniff(blob):
    """'jpeg', 'png' or None."""
    head = bytes(blob[:8])
    if head[:2] == b"\xff\xd8":
        return "jpeg"
    if head == png.SIGNATURE:
        return "png"
    return None


def reason(kind, status):
    if kind == "jpeg":
        return jpeg.STATUS.get(int(status), "?")
    if kind == "png":
        return png.reason(status)
    return "neither a JPEG nor a PNG signature"


@torch.no_grad()
def decode_images(blobs, order="rgb", strict=True, device="cuda", progressive=False):
    """A list of JPEG / PNG byte strings -> (buf, meta): the packed 3-channel form ijb.align_faces, mtcnn_align and
    detect.Detector take (buf uint8 on the device, meta int64 numpy [N][4] = byte offset, H, W, pitch), in the caller's
    order.  order "rgb" or "bgr".  strict=True: ValueError naming the first image that cannot be decoded and why (reads
    the statuses back: a synchronisation); strict=False: (buf, meta, status) with status int32 [N] on the device -- the
    decoder's own status word (jpeg.STATUS / png.STATUS), or UNKNOWN_FORMAT; failing images hold unspecified pixels.
    progressive=True: progressive JPEG streams decode too (jpeg.pack_jpegs); by default they are status 17."""
    if order not in ("rgb", "bgr"):
        raise ValueError("decode_images: order must be 'rgb' or 'bgr'")
    if not isinstance(blobs, (list, tuple)) or len(blobs) == 0:
        raise ValueError("decode_images: needs a non-empty list of byte strings")
    n = len(blobs)
    kinds = [sniff(b) for b in blobs]
    rows = {k: [i for i in range(n) if kinds[i] == k] for k in ("jpeg", "png")}
    host = np.full(n, UNKNOWN_FORMAT, np.int32)
    hw = np.ones((n, 2), np.int64)
    batches = {}
    for k, mod, pack in (("jpeg", jpeg, jpeg.pack_jpegs), ("png", png, png.pack_pngs)):
        if rows[k]:
            batches[k] = pack([blobs[i] for i in rows[k]], **({"progressive": True} if progressive and k == "jpeg" else {}))
            host[rows[k]] = batches[k].status
            hw[rows[k]] = _codec.extents(batches[k])
    if strict:
        for i in np.flatnonzero(host):
            raise DecodeError(i, kinds[i], host[i])
    meta, total = packed.layout(hw[:, 0], hw[:, 1])
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    status = torch.from_numpy(host).to(buf.device)
    for k, mod in (("jpeg", jpeg), ("png", png)):
        if rows[k] and (batches[k].status == 0).any():
            st = mod.decode_into(batches[k], buf, meta[rows[k]], 3, order)
            status[torch.as_tensor(rows[k], device=buf.device)] = st
    if strict:
        got = status.cpu().numpy()
        for i in np.flatnonzero(got):
            raise DecodeError(i, kinds[i], got[i])
        return buf, meta
    return buf, meta, status


# ------------------------------------------------------------------------------------------------------------ writing
# PIL.Image.save(path) of eval/align_dataset.py:52-75 for a batch on the device: the format comes from the file name's
# suffix as Pillow takes it, the JPEG and the PNG subsets each go out in one launch (jpeg.encode_batch,
# png.encode_batch), and one device-to-host copy brings every file over.
SUFFIXES = {".jpg": "jpeg", ".jpeg": "jpeg", ".jpe": "jpeg", ".jfif": "jpeg", ".png": "png"}


def format_of(name):
    """'jpeg' or 'png' from a format name ('png', 'JPEG', 'jpg') or a path / suffix ('.png', 'a/b.JPG'), as
    PIL.Image.save reads it; ValueError for anything else."""
    s = str(name).lower()
    if s in ("jpeg", "jpg", "png"):
        return "png" if s == "png" else "jpeg"
    dot = s.rfind(".")
    kind = SUFFIXES.get(s[dot:]) if dot >= 0 else None
    if kind is None:
        raise ValueError("unknown image format or suffix %r (JPEG: .jpg .jpeg .jpe .jfif, PNG: .png)" % (name,))
    return kind


class EncodedImages:
    """encode_images' result: the JPEG and the PNG subset as jpeg.EncodedBatch each (None for an empty one) and the rows
    of the caller's list each holds.  to_bytes() -> the files in the caller's order, after ONE device-to-host copy."""

    def __init__(self, n, batches):
        self.n, self.batches = n, batches                 # batches: [(kind, rows, EncodedBatch)]

    def __len__(self):
        return self.n

    def to_bytes(self, strict=True):
        parts, spans, o = [], [], 0
        for kind, rows, b in self.batches:
            tail = torch.stack([b.length, b.status]).view(torch.uint8).reshape(-1)
            parts += [b.buf.reshape(-1), tail]
            spans.append((o, o + b.buf.numel()))
            o += b.buf.numel() + tail.numel()
        host = torch.cat(parts).cpu().numpy()
        out = [b""] * self.n
        for (kind, rows, b), (lo, hi) in zip(self.batches, spans):
            ls = host[hi:hi + 8 * len(rows)].view(np.int32).reshape(2, len(rows))
            for k, i in enumerate(rows):
                if ls[1, k] and strict:
                    table = jpeg.ENCODE_STATUS if kind == "jpeg" else png.ENCODE_STATUS
                    raise ValueError("encode_images: image %d: %s (status %d)" % (i, table.get(int(ls[1, k]), "?"), ls[1, k]))
                s = lo + int(b.slots_host[k, 0])
                out[i] = host[s:s + int(ls[0, k])].tobytes()
        return out


@torch.no_grad()
def encode_images(images, formats, order="rgb", filter="adaptive", device="cuda", **jpeg_options):
    """One door for writing: images uint8 [N, H, W, 3] (or [N, H, W]) or the packed 3-channel (buf, meta); formats one
    name / suffix / path for all or one per image (format_of).  The JPEG rows go through jpeg.encode_batch with
    jpeg_options (quality, sampling, restart), the PNG rows through png.encode_batch with `filter`: one launch sequence
    per codec, the same bytes as the two codecs called on their rows.  -> EncodedImages.  No synchronisation."""
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8 or images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[3] != 3):
            raise ValueError("encode_images: images must be a uint8 [N, H, W, 3] or [N, H, W] tensor, or the packed (buf, meta)")
        n, h, w = (int(v) for v in images.shape[:3])
        channels = 3 if images.dim() == 4 else 1
        meta = np.empty((n, 4), np.int64)
        meta[:, 0] = np.arange(n, dtype=np.int64) * (h * w * channels)
        meta[:, 1], meta[:, 2], meta[:, 3] = h, w, w * channels
        buf = images.to(device).contiguous().reshape(-1)
    else:
        buf, meta = images
        meta = np.ascontiguousarray(meta.cpu().numpy() if isinstance(meta, torch.Tensor) else meta, dtype=np.int64)
        n, channels = len(meta), 3
    kinds = [format_of(formats)] * n if isinstance(formats, str) else [format_of(f) for f in formats]
    if len(kinds) != n:
        raise ValueError("encode_images: %d formats for %d images" % (len(kinds), n))
    batches = []
    for kind in ("jpeg", "png"):
        rows = [i for i in range(n) if kinds[i] == kind]
        if not rows:
            continue
        sub = (buf, meta[rows])
        if kind == "jpeg":
            opts = {k: (v if isinstance(v, (str, int, np.integer)) else [v[i] for i in rows]) for k, v in jpeg_options.items()}
            b = jpeg.encode_batch(sub, order=order, device=device, channels=channels, **opts)
        else:
            b = png.encode_batch(sub, order=order, filter=filter, device=device, channels=channels)
        batches.append((kind, rows, b))
    return EncodedImages(n, batches)


def save_images(images, paths, order="rgb", filter="adaptive", device="cuda", **jpeg_options):
    """PIL.Image.save(path) for every image: the format from each path's suffix (format_of), encode_images, one
    device-to-host copy for which the host waits, then the file writes.  The directories must exist.  -> the paths."""
    paths = [str(p) for p in paths]
    files = encode_images(images, paths, order, filter, device, **jpeg_options).to_bytes()
    for p, data in zip(paths, files):
        with open(p, "wb") as f:
            f.write(data)
    return paths
