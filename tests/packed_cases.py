"""What the GPU tests of the stages that write packed images (buf, meta int64 [N][4] = byte offset, H, W, pitch) share:
destinations between guard bands, a layout written without msml_amd.packed, and the reading back of a packed output with
its checks."""
import numpy as np
import torch

GUARD = 64
FILL = 0xA5


def guarded(total, fill=FILL, guard=GUARD):
    """A buffer of `fill` with `total` bytes between two guard bands, and the view of the middle."""
    whole = torch.full((total + 2 * guard,), fill, dtype=torch.uint8, device="cuda")
    return whole, whole[guard:guard + total]


def bands_untouched(whole, fill=FILL, guard=GUARD):
    h = whole.cpu().numpy()
    return bool((h[:guard] == fill).all() and (h[-guard:] == fill).all())


def batch_sizes(batch):
    """(H, W) of every stream of a JpegBatch / PngBatch; 1 x 1 for one the parser refused."""
    return [(d.height, d.width) if d.status == 0 else (1, 1) for d in batch.descriptors]


def packed_meta(sizes, channels=3, gap=0, offset=0, pitch_extra=None):
    """meta of rectangles for images of `sizes` [(H, W)], and the bytes they span.  Every rectangle starts `offset`
    bytes behind the next multiple of 4 and has `gap` bytes behind it (a canary between every two of them).  Pitches
    are the rows rounded up to dwords, or row bytes + pitch_extra when that is given."""
    meta = np.empty((len(sizes), 4), np.int64)
    end = 0
    for i, (h, w) in enumerate(sizes):
        pitch = (w * channels + 3) & ~3 if pitch_extra is None else w * channels + pitch_extra
        start = ((end + 3) & ~3) + offset
        meta[i] = start, h, w, pitch
        end = start + h * pitch + gap
    return meta, end


def canaries_intact(buf, meta, fill=FILL, least=32):
    """Every byte of buf outside the rectangles of meta still holds the fill (at least `least` such bytes per image)."""
    flat = buf.cpu().numpy()
    outside = np.ones(flat.size, bool)
    for off, h, w, pitch in np.asarray(meta):
        outside[off:off + h * pitch] = False
    return bool((flat[outside] == fill).all()) and int(outside.sum()) >= least * len(meta)


def unpack(buf, meta, channels=3, check_pad=True, ok=None, pad=0, fill=FILL):
    """The images of a packed output.  Of an image that decoded, the bytes between the row and its pitch must be `pad`
    (0: what an aligned store writes there; the fill for a destination whose pad bytes must not be touched; skipped
    with check_pad=False); of one with a status (ok[i] false), every byte of the rectangle must still hold the fill."""
    flat = buf.cpu().numpy()
    out = []
    for i, (off, h, w, pitch) in enumerate(np.asarray(meta)):
        rows = flat[off:off + h * pitch].reshape(h, pitch)
        if ok is not None and not ok[i]:
            assert (rows == fill).all(), "image %d has a status, yet its rectangle was written" % i
            out.append(None)
            continue
        if check_pad:
            assert (rows[:, w * channels:] == pad).all(), "image %d: the bytes behind its rows are not %d" % (i, pad)
        img = rows[:, :w * channels]
        out.append(img.reshape(h, w, channels) if channels != 1 else img.reshape(h, w))
    return out


def decode_at(batch, decode_into, channels, offset, pitch_extra, pad):
    """One launch of `batch` into rectangles that start `offset` bytes behind a dword boundary with a pitch of row bytes
    + pitch_extra (None: the row rounded up to dwords), 32 canary bytes apart, in a guarded buffer of FILL -> the images.
    Asserts status 0 for all, `pad` in every byte between a row's end and its pitch, the gaps and the bands untouched."""
    meta, total = packed_meta(batch_sizes(batch), channels, gap=32, offset=offset, pitch_extra=pitch_extra)
    whole, dst = guarded(total)
    status = decode_into(batch, dst, meta, channels)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    assert bands_untouched(whole) and canaries_intact(dst, meta)
    return unpack(dst, meta, channels, pad=pad)
