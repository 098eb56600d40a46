"""What the JPEG and the PNG decoder (jpeg.py, png.py) do alike around their own parsers and device calls: the packed
stream buffer, the batch object, and the decode_batch driver."""
import collections

import numpy as np
import torch

from . import packed


def pinned(shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=torch.cuda.is_available())


def raise_first(status, what, reasons):
    bad = np.flatnonzero(status)
    if bad.size:
        i = int(bad[0])
        raise ValueError("%s: image %d: %s (status %d)" % (what, i, reasons.get(int(status[i]), "?"), int(status[i])))


def pack_streams(lengths, who):
    """The buffer that holds streams of `lengths` bytes (0: an image without one) back to back at 4-byte-aligned
    offsets -> (uint8 tensor of whole dwords, pinned when a GPU is present; the offsets as a list).  The bytes between
    a stream's end and the next offset are 0; the caller copies the streams in."""
    size = (np.asarray(lengths, np.int64) + 3) & ~3
    offs = np.cumsum(size) - size
    total = int(size.sum())
    if total >= 2 ** 33:
        raise ValueError("%s: more than 8 GiB of streams in one batch" % who)
    buf = pinned(max(total, 4), torch.uint8)
    words = buf.numpy().view(np.uint32)
    words[(offs + size)[size > 0] // 4 - 1] = 0           # the last dword of every stream: its padding
    if total == 0:
        words[0] = 0
    return buf, offs.tolist()


class StreamBatch:
    """A packed batch of compressed images on the host: `desc` int32 [N, words] with the parser's status in column
    STATUS_WORD, `descriptors` (height, width, status of every stream), and the tensors named in FIELDS (streams and
    desc first), which to_device copies."""
    FIELDS = ()
    STATUS_WORD = 0

    def __len__(self):
        return self.desc.shape[0]

    @property
    def status(self):
        return self.desc[:, self.STATUS_WORD].numpy()

    @property
    def sizes(self):
        return [(d.height, d.width) for d in self.descriptors]

    def to_device(self, device="cuda"):
        """The tensors of FIELDS on the device, copied once (non_blocking, on the current stream)."""
        if self._dev is None or self._dev[0].device != torch.device(device):
            self._dev = tuple(getattr(self, f).to(device, non_blocking=True) for f in self.FIELDS)
        return self._dev


def extents(batch):
    """int64 [N][2] = H, W of every stream of a StreamBatch; 1 x 1 for one the parser refused."""
    return np.array([(d.height, d.width) if d.status == 0 else (1, 1) for d in batch.descriptors], np.int64).reshape(-1, 2)


# What differs between the two decoders: pack(list of byte strings) -> batch, the batch class, the channel counts
# decode_batch takes, colour(descriptor) -> None for a stream channels=1 accepts or what it is instead, decode_into,
# and the status table.
Codec = collections.namedtuple("Codec", "pack batch channels colour decode_into reasons")


@torch.no_grad()
def decode_batch(codec, batch, size, order, strict, channels, device):
    """jpeg.decode_batch / png.decode_batch (their docstrings say what comes back)."""
    if order not in ("rgb", "bgr"):
        raise ValueError("decode_batch: order must be 'rgb' or 'bgr'")
    if channels not in codec.channels:
        raise ValueError("decode_batch: channels must be %s or %d"
                         % (", ".join(str(c) for c in codec.channels[:-1]), codec.channels[-1]))
    if not isinstance(batch, codec.batch):
        batch = codec.pack(batch)
    n = len(batch)
    host = batch.status
    if strict:
        raise_first(host, "decode_batch", codec.reasons)
    ok = host == 0
    hw = extents(batch)
    if channels == 1:
        for i in np.flatnonzero(ok):
            what = codec.colour(batch.descriptors[i])
            if what is not None:
                raise ValueError("decode_batch: channels=1 takes gray streams; image %d has %s" % (i, what))
    if size is not None:
        h, w = int(size[0]), int(size[1])
        for i in np.flatnonzero(ok):
            if tuple(hw[i]) != (h, w):
                raise ValueError("decode_batch: image %d is %d x %d, not %d x %d" % (i, hw[i, 0], hw[i, 1], h, w))
        out = torch.empty((n, h, w, channels) if channels != 1 else (n, h, w), dtype=torch.uint8, device=device)
        dst = out
        meta = packed.uniform_meta(n, h, w, channels, out.device)      # on the device, uploaded once per shape
    else:
        meta, total = packed.layout(hw[:, 0], hw[:, 1], channels)
        dst = torch.empty(total, dtype=torch.uint8, device=device)
        out = (dst, meta)
    if ok.any():
        status = codec.decode_into(batch, dst, meta, channels, order)
    else:
        status = torch.from_numpy(host.astype(np.int32)).to(device)
    if strict:
        raise_first(status.cpu().numpy(), "decode_batch", codec.reasons)
        return out
    return (out, status) if size is not None else out + (status,)
