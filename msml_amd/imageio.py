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
