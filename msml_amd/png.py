"""PNG decoding on the device, Pillow's pixels (csrc/png.hip): what PIL.Image.open(f).convert(mode) does in front of the
folder evaluation (eval/qeval_folder.py:43-49), the alignment tool (eval/align_dataset.py:44) and the occluder folders
(datasets/augment/rand_occ.py:345-366).

The host walks the chunks only (parse_png checks their order and CRCs and never inflates); the concatenated IDAT bytes
go to the device, where msml_png_decode inflates them (zlib wrapper, stored / fixed / dynamic blocks, the tables built
on the device), undoes the row filters and writes the uint8 pixels Pillow gives for mode L / RGB / RGBA, either as one
[N, H, W, C] tensor or in the packed (buf, meta) form ijb.align_faces, mtcnn_align and detect.Detector take.

A stream is accepted exactly when `d = zlib.decompressobj(); out = d.decompress(idat)` runs without an exception,
d.eof is true and len(out) == H * (1 + ceil(W * bits_per_pixel / 8)); bytes behind the end of the zlib stream are
ignored.  That is STRICTER than Pillow in a few truncation cases: Pillow returns the pixels of a stream whose last
block or Adler-32 trailer is cut off once every row has arrived (and, with LOAD_TRUNCATED_IMAGES, of shorter ones);
here such a stream has a status and its rectangle stays untouched.  tests/png_cases.py restates the arithmetic.
"""
import struct
import zlib

import numpy as np
import torch

from . import _codec, packed
from ._codec import StreamBatch, pack_streams, pinned
from ._lib import call, value

SIGNATURE = b"\x89PNG\r\n\x1a\n"
DESC_WORDS = 16
(PD_BASE, PD_END, PD_H, PD_W, PD_DEPTH, PD_CTYPE, PD_PAL, PD_STATUS, PD_WS, PD_KEY, PD_KEY0, PD_KEY1, PD_KEY2) = range(13)

# status[n] of a decode: 1-12 from the device (csrc/png_core.h), 16.. from the parser
STATUS = {
    0: "ok", 1: "bad zlib header", 2: "reserved block type", 3: "stored-block length check failed",
    4: "bad code-length set or repeat", 5: "bad literal/length or distance symbol", 6: "distance before the start",
    7: "the data ends early", 8: "more data than the image holds", 9: "Adler-32 mismatch", 10: "filter byte above 4",
    11: "the output rectangle does not match the image", 12: "4 channels asked of a stream the expand step has no rule for",
    16: "not a PNG stream, or malformed chunks", 17: "a chunk's CRC does not match", 18: "16-bit samples are unsupported",
    19: "Adam7 interlace is unsupported", 20: "compression or filter method other than 0",
    21: "a colour type / bit depth pair the specification does not allow", 22: "a palette stream without PLTE",
    23: "image size outside 1..32767", 24: "a zero-length IDAT stream", 25: "APNG (acTL) is unsupported",
}
STATUS_FILTER, STATUS_OUTPUT = 10, 11
(BAD_HEADER, BAD_CRC, SIXTEEN_BIT, INTERLACE, METHOD, COLOUR, NO_PLTE, SIZE, NO_IDAT, APNG) = range(16, 26)

CHANNELS_OF = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}                 # samples per pixel of each colour type
DEPTHS_OF = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


def reason(status):
    return STATUS.get(int(status), "?")


class PngDescriptor:
    """What parse_png read.  status 0: a supported stream, every field is set; otherwise `reason` says why not and
    the fields read up to that point are set.  idat: [(begin, end)] byte ranges of the IDAT payloads in `data`."""

    def __init__(self, data):
        self.data = data
        self.status = 0
        self.width = self.height = self.depth = self.colour_type = 0
        self.plte = self.trns = None
        self.idat = []

    @property
    def reason(self):
        return STATUS[self.status]

    @property
    def bits_per_pixel(self):
        return self.depth * CHANNELS_OF[self.colour_type]

    @property
    def row_bytes(self):
        return (self.width * self.bits_per_pixel + 7) // 8

    @property
    def expected(self):
        return self.height * (1 + self.row_bytes)

    @property
    def has_alpha(self):
        return self.colour_type in (4, 6)

    def zlib_stream(self):
        return b"".join(self.data[a:b] for a, b in self.idat)

    def palette(self):
        """256 RGBA entries, uint8 [256][4]: PLTE + tRNS; alpha 255 where tRNS is short or absent; an entry past
        PLTE's end is (0, 0, 0, 255), what Pillow gives for such an index (recorded in tests/golden/g17_png.npz)."""
        p = np.zeros((256, 4), np.uint8)
        p[:, 3] = 255
        n = len(self.plte) // 3
        p[:n, :3] = np.frombuffer(self.plte, np.uint8, n * 3).reshape(n, 3)
        if self.trns:
            t = np.frombuffer(self.trns, np.uint8)[:256]
            p[:len(t), 3] = t
        return p

    def key(self):
        """The tRNS colour key of a gray or RGB stream as samples (masked to the bit depth), or None."""
        if self.trns is None or self.colour_type not in (0, 2):
            return None
        n = 1 if self.colour_type == 0 else 3
        if len(self.trns) < 2 * n:
            return None
        return tuple(v & ((1 << self.depth) - 1) for v in struct.unpack(">%dH" % n, self.trns[:2 * n]))


def _refuse(d, status):
    d.status = status
    return d


def parse_png(data):
    """Walk the chunks (signature, IHDR first and 13 bytes long, PLTE before IDAT, consecutive IDATs, IEND) ->
    PngDescriptor.  Never inflates and never raises.  Every chunk's CRC is checked (Pillow raises on a bad one; here it
    is a status).  Refused with a reason each: 16-bit samples, Adam7, compression / filter method != 0, a colour type /
    depth pair outside the specification, a palette stream without PLTE, sizes outside 1..32767, no IDAT bytes, APNG.
    Ancillary chunks (gAMA, iCCP, sRGB, pHYs, tEXt ...) are skipped, as Pillow's convert ignores them."""
    data = bytes(data)
    d = PngDescriptor(data)
    n = len(data)
    if data[:8] != SIGNATURE:
        return _refuse(d, BAD_HEADER)
    pos = 8
    first, seen_idat, idat_closed, seen_end = True, False, False, False
    while pos < n:
        if pos + 12 > n:
            return _refuse(d, BAD_HEADER)
        ln = struct.unpack(">I", data[pos:pos + 4])[0]
        typ = data[pos + 4:pos + 8]
        if ln > 0x7fffffff or pos + 12 + ln > n:
            return _refuse(d, BAD_HEADER)
        body = data[pos + 8:pos + 8 + ln]
        if zlib.crc32(data[pos + 4:pos + 8 + ln]) != struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])[0]:
            return _refuse(d, BAD_CRC)
        if first != (typ == b"IHDR"):
            return _refuse(d, BAD_HEADER)
        if typ == b"IHDR":
            if ln != 13:
                return _refuse(d, BAD_HEADER)
            d.width, d.height, d.depth, d.colour_type, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            first = False
            if d.colour_type not in DEPTHS_OF or d.depth not in DEPTHS_OF[d.colour_type]:
                return _refuse(d, COLOUR)
            if d.depth == 16:
                return _refuse(d, SIXTEEN_BIT)
            if comp != 0 or filt != 0:
                return _refuse(d, METHOD)
            if lace == 1:
                return _refuse(d, INTERLACE)
            if lace != 0:
                return _refuse(d, BAD_HEADER)
            if not (1 <= d.width <= 32767 and 1 <= d.height <= 32767):
                return _refuse(d, SIZE)
        elif typ == b"PLTE":
            if seen_idat or d.plte is not None or ln == 0 or ln % 3 or ln > 768:
                return _refuse(d, BAD_HEADER)
            d.plte = body
        elif typ == b"tRNS":
            if seen_idat or d.trns is not None or (d.colour_type == 3 and d.plte is None) or d.colour_type in (4, 6):
                return _refuse(d, BAD_HEADER)
            d.trns = body
        elif typ == b"acTL":
            return _refuse(d, APNG)
        elif typ == b"IDAT":
            if idat_closed:
                return _refuse(d, BAD_HEADER)
            seen_idat = True
            if ln:
                d.idat.append((pos + 8, pos + 8 + ln))
        elif typ == b"IEND":
            seen_end = True
            break
        if seen_idat and typ != b"IDAT":
            idat_closed = True
        pos += 12 + ln
    if first or not seen_end:
        return _refuse(d, BAD_HEADER)
    if d.colour_type == 3 and d.plte is None:
        return _refuse(d, NO_PLTE)
    if not d.idat:
        return _refuse(d, NO_IDAT)
    return d


class PngBatch(StreamBatch):
    """pack_pngs' result: everything msml_png_decode reads, on the host (pinned when a GPU is present).  streams uint8
    [bytes]: each image's IDAT payloads back to back (ONE zlib stream per image) at 4-byte-aligned offsets; desc int32
    [N, 16]; palettes uint8 [np, 256, 4], each distinct palette once; descriptors; ws_bytes."""

    FIELDS = ("streams", "desc", "palettes")
    STATUS_WORD = PD_STATUS

    def __init__(self, streams, desc, palettes, descriptors, ws_bytes):
        self.streams, self.desc, self.palettes = streams, desc, palettes
        self.descriptors, self.ws_bytes = descriptors, ws_bytes
        self._dev = None


def pack_pngs(streams):
    """A list of PNG byte strings -> PngBatch.  Streams the parser refuses keep their place with their status."""
    if not isinstance(streams, (list, tuple)) or len(streams) == 0:
        raise ValueError("pack_pngs: needs a non-empty list of byte strings")
    n = len(streams)
    descs = [parse_png(s) for s in streams]
    pidx, pals = {}, []
    desc = pinned((n, DESC_WORDS), torch.int32)
    dn = desc.numpy()
    dn[...] = 0
    lengths = [sum(b - a for a, b in d.idat) if d.status == 0 else 0 for d in descs]
    buf, offs = pack_streams(lengths, "pack_pngs")
    for i, (off, zl, d) in enumerate(zip(offs, lengths, descs)):
        dn[i, PD_STATUS] = d.status
        dn[i, PD_PAL] = -1
        if d.status:
            continue
        dn[i, PD_BASE], dn[i, PD_END] = off // 4, zl
        dn[i, PD_H], dn[i, PD_W], dn[i, PD_DEPTH], dn[i, PD_CTYPE] = d.height, d.width, d.depth, d.colour_type
        if d.colour_type == 3:
            p = d.palette()
            k = p.tobytes()
            if k not in pidx:
                pidx[k] = len(pals)
                pals.append(p)
            dn[i, PD_PAL] = pidx[k]
        key = d.key()
        if key is not None:
            dn[i, PD_KEY] = 1
            dn[i, PD_KEY0:PD_KEY0 + len(key)] = key
    flat = buf.numpy()
    for d, o in zip(descs, offs):
        if d.status == 0:
            for a, b in d.idat:
                flat[o:o + b - a] = np.frombuffer(d.data, np.uint8, b - a, a)
                o += b - a
    pal = pinned((max(len(pals), 1), 256, 4), torch.uint8)
    pal.numpy()[...] = np.stack(pals) if pals else 0
    ws_bytes = 0
    if any(d.status == 0 for d in descs):
        ws_bytes = value("msml_png_workspace", desc.data_ptr(), n)
        if ws_bytes <= 0:
            raise RuntimeError("msml_png_workspace refused the descriptors")
    return PngBatch(buf, desc, pal, descs, ws_bytes)


@torch.no_grad()
def decode_into(batch, dst, meta, channels=3, order="rgb", ws=None, status=None):
    """msml_png_decode of a PngBatch into the caller's buffers, on the current stream: dst a uint8 tensor on the device,
    meta int64 [N][4] = byte offset in dst, H, W, pitch -- numpy (uploaded here) or a tensor already on the device (the
    device checks every row against its stream and against dst.numel(): a row that does not fit gives status 11 and
    writes nothing).  ws: uint8 on the device, at least batch.ws_bytes (allocated when None); status: int32 [N] on the
    device (allocated when None), returned."""
    n = len(batch)
    device = dst.device
    meta_dev = packed.meta_on_device(meta, n, device, "decode_into")
    streams, desc, palettes = batch.to_device(device)
    if ws is None:
        ws = torch.empty(max(batch.ws_bytes, 16), dtype=torch.uint8, device=device)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=device)
    call("msml_png_decode", streams, streams.numel(), desc, batch.desc.data_ptr(), palettes, palettes.numel(), dst,
         dst.numel(), meta_dev, channels, 1 if order == "bgr" else 0, status, ws, ws.numel(), n)
    return status


@torch.no_grad()
def decode_batch(batch, size=None, order="rgb", strict=True, channels=3, device="cuda"):
    """Decode a PngBatch (or a list of byte strings) on the device, on the current stream: the pixels of Pillow's
    Image.open(f).convert("L" / "RGB" / "RGBA") for channels 1 / 3 / 4.

    size=(H, W): uint8 [N, H, W, channels] ([N, H, W] for channels=1); an image of another size is a ValueError.
    size=None: (buf, meta) in the packed form of ijb.pack_images (meta int64 numpy [N][4] = byte offset, H, W, pitch).
    order: "rgb" or "bgr" (alpha stays last).  channels=1 takes gray and gray + alpha streams only.
    strict=True: ValueError naming the first failing image and why (this reads the statuses back: a synchronisation);
    strict=False: the int32 status tensor [N] comes back as the last element instead, failing images hold unspecified
    pixels.  A batch with no supported stream launches nothing."""
    return _codec.decode_batch(_CODEC, batch, size, order, strict, channels, device)


_CODEC = _codec.Codec(pack_pngs, PngBatch, (1, 3, 4),
                      lambda d: None if d.colour_type in (0, 4) else "colour type %d" % d.colour_type, decode_into, STATUS)


# ---------------------------------------------------------------------------------------------------------- encoding
# PNG files from pixels on the device (csrc/png_enc.hip, csrc/png_enc_core.h): what PIL.Image.save writes for the .png
# names of eval/align_dataset.py:52-75 and the '.png' payloads of datasets/3d_tools/cvt_casia_webface.py:35 -- files
# Pillow, zlib and msml_png_decode read back to exactly the source pixels.  The bytes are NOT Pillow's (PNG is lossless,
# and zlib's lazy matcher is sequential): 8-bit samples, colour type 0 / 4 / 2 / 6 for 1 / 2 / 3 / 4 channels, no
# interlace, one IDAT chunk, no ancillary chunks.  tests/png_enc_cases.py restates the filter pass and the container.
ENC_DESC_WORDS = 4
(PE_H, PE_W, PE_WS) = 0, 1, 2
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
COLOUR_TYPE_OF = {1: 0, 2: 4, 3: 2, 4: 6}
ENCODE_STATUS = {0: "ok", 1: "the meta row is not this image inside the source buffer",
                 2: "the slot is outside the output buffer or too small for the file",
                 3: "unsupported geometry (a size outside 1..32767, or more than 2^30 - 1 filtered bytes)"}


def encode_bound(height, width, channels):
    """msml_png_encode_bound: the all-stored worst case, which no file exceeds (0 for an unsupported geometry)."""
    return value("msml_png_encode_bound", int(height), int(width), int(channels))


class PngEncodePlan:
    """What msml_png_encode reads besides the pixels: desc int32 [N, 4] (pinned) = H, W, workspace offset; bounds int64
    [N] = msml_png_encode_bound of every image rounded up to 4; ws_bytes.  The twin of jpeg.EncodePlan."""

    STATUS = ENCODE_STATUS

    def __init__(self, sizes, channels):
        n = len(sizes)
        if n == 0:
            raise ValueError("encode: needs at least one image")
        self.n, self.sizes, self.channels = n, [(int(h), int(w)) for h, w in sizes], int(channels)
        self.desc = pinned((n, ENC_DESC_WORDS), torch.int32)
        dn = self.desc.numpy()
        dn[...] = 0
        self.bounds = np.zeros(n, np.int64)
        for i, (h, w) in enumerate(self.sizes):
            if not (1 <= h <= 32767 and 1 <= w <= 32767):
                raise ValueError("encode: image %d is %d x %d, sizes must be 1..32767" % (i, h, w))
            b = encode_bound(h, w, channels)
            if b <= 0:
                raise ValueError("encode: image %d (%d x %d x %d) holds more than 2^30 - 1 filtered bytes" % (i, h, w, channels))
            dn[i, PE_H], dn[i, PE_W] = h, w
            self.bounds[i] = (b + 3) & ~3
        self.ws_bytes = value("msml_png_encode_ws_bytes", self.desc.data_ptr(), self.channels, n)
        if self.ws_bytes <= 0:
            raise RuntimeError("msml_png_encode_ws_bytes refused the descriptors")
        self._dev = None

    def to_device(self, device="cuda"):
        if self._dev is None or self._dev.device != torch.device(device):
            self._dev = self.desc.to(device, non_blocking=True)
        return self._dev


_PLANS = {}


def _plan(sizes, channels):
    if len(set(sizes)) == 1:
        key = (len(sizes), sizes[0], channels)
        if key not in _PLANS:
            if len(_PLANS) >= 16:
                _PLANS.clear()
            _PLANS[key] = PngEncodePlan(sizes, channels)
        return _PLANS[key]
    return PngEncodePlan(sizes, channels)


def _check_options(channels, order, filter, who):
    if channels not in (1, 2, 3, 4):
        raise ValueError("%s: channels must be 1..4, got %r" % (who, channels))
    if order not in ("rgb", "bgr"):
        raise ValueError("%s: order must be 'rgb' or 'bgr'" % who)
    if order == "bgr" and channels < 3:
        raise ValueError("%s: order 'bgr' needs 3 or 4 channels, got %d" % (who, channels))
    if filter not in FILTERS:
        raise ValueError("%s: filter must be one of %s, got %r" % (who, sorted(FILTERS), filter))


def _source(images, channels):
    """-> (src uint8 tensor, meta int64 numpy [N][4] or None for a contiguous tensor, sizes, channels), nothing moved."""
    if isinstance(images, (tuple, list)) and len(images) == 2 and isinstance(images[0], torch.Tensor) and images[0].dim() == 1:
        buf, meta = images
        meta = np.ascontiguousarray(meta.cpu().numpy() if isinstance(meta, torch.Tensor) else meta, dtype=np.int64)
        if buf.dtype != torch.uint8 or meta.ndim != 2 or meta.shape[1] != 4:
            raise ValueError("encode: the packed form is (uint8 buffer, int64 meta [N][4])")
        return buf, meta, [(int(h), int(w)) for h, w in meta[:, 1:3]], channels
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() not in (3, 4):
        raise ValueError("encode: images must be a uint8 [N, H, W] or [N, H, W, C] tensor, or the packed (buf, meta)")
    c = int(images.shape[3]) if images.dim() == 4 else 1
    if images.dim() == 4 and not 2 <= c <= 4:
        raise ValueError("encode: [N, H, W, C] takes C in 2..4, got %d" % c)
    return images, None, [(int(images.shape[1]), int(images.shape[2]))] * images.shape[0], c


@torch.no_grad()
def encode_into(src, meta, dst, slots, channels=3, order="rgb", filter="adaptive", length=None, status=None, ws=None,
                plan=None):
    """msml_png_encode with the caller's buffers, on the current stream.  src: uint8 on the device; meta: int64 [N][4] on
    the device = byte offset, H, W, pitch of each source, or the same in numpy (uploaded here); dst: uint8 on the device;
    slots: int64 [N][2] on the device = byte offset and capacity of each image's slot.  length / status int32 [N] and ws
    are allocated when None.  plan: a PngEncodePlan of the sizes (needed when meta is on the device only, where the host
    cannot read the sizes).  -> (length, status).  The device checks every meta row against src and every slot against
    dst: an image that does not fit gets a status (ENCODE_STATUS) and length 0 and writes nothing outside its slot."""
    _check_options(channels, order, filter, "encode_into")
    device = dst.device
    if plan is None:
        if isinstance(meta, torch.Tensor):
            raise ValueError("encode_into: a meta tensor on the device needs plan= (the host lays out the workspace)")
        meta = np.ascontiguousarray(meta, dtype=np.int64)
        plan = _plan([(int(h), int(w)) for h, w in meta[:, 1:3]], channels)
    n = plan.n
    if plan.channels != channels:
        raise ValueError("encode_into: the plan is for %d channels, not %d" % (plan.channels, channels))
    meta = packed.meta_on_device(meta, n, device, "encode_into")
    if not isinstance(slots, torch.Tensor) or slots.dtype != torch.int64 or tuple(slots.shape) != (n, 2) or \
            slots.device != device or not slots.is_contiguous():
        raise ValueError("encode_into: slots must be a contiguous int64 [%d, 2] tensor on %s" % (n, device))
    desc = plan.to_device(device)
    if length is None:
        length = torch.empty(n, dtype=torch.int32, device=device)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=device)
    if ws is None:
        ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=device)
    call("msml_png_encode", src, src.numel(), meta, channels, 1 if order == "bgr" else 0, FILTERS[filter], desc,
         plan.desc.data_ptr(), dst, dst.numel(), slots, length, status, ws, ws.numel(), n)
    return length, status


@torch.no_grad()
def encode_batch(images, order="rgb", filter="adaptive", device="cuda", channels=3, slot_bytes=None):
    """Encode N images on the device to PNG files -> jpeg.EncodedBatch (to_bytes, write_faces and imageio.save_images
    take it as they take a JPEG one; its plan is a PngEncodePlan).  No synchronisation.

    images: uint8 [N, H, W] (gray), [N, H, W, C] with C 2 (gray + alpha), 3 (RGB) or 4 (RGBA), or the packed (buf, meta)
    of ijb.pack_images / decode_batch with `channels` bytes per pixel.  order "bgr": the sources are B, G, R(, A).
    filter: "adaptive" (per row the filter with the smallest sum of abs((int8) byte), ties to the lowest number: the
    libpng / Pillow heuristic) or one of "none", "sub", "up", "average", "paeth" for every row.  slot_bytes: the capacity
    of every slot; the default is msml_png_encode_bound, the all-stored worst case no file exceeds (photographs take
    about 0.65 of it), so a caller that knows its data may pass less (an image that does not fit gets status 2)."""
    from .jpeg import EncodedBatch
    src, meta, sizes, channels = _source(images, channels)
    _check_options(channels, order, filter, "encode")
    plan = _plan(sizes, channels)
    n = plan.n
    src = src.to(device).contiguous()
    if meta is None:
        h, w = sizes[0]
        meta_dev = packed.uniform_meta(n, h, w, channels, src.device)
    else:
        meta_dev = torch.from_numpy(meta).to(src.device)
    caps = plan.bounds if slot_bytes is None else np.full(n, (int(slot_bytes) + 3) & ~3, np.int64)
    slots = np.empty((n, 2), np.int64)
    slots[:, 1] = caps
    slots[:, 0] = np.cumsum(caps) - caps
    dst = torch.empty(int(caps.sum()), dtype=torch.uint8, device=src.device)
    slots_dev = torch.from_numpy(slots).to(src.device)
    length, status = encode_into(src.reshape(-1), meta_dev, dst, slots_dev, channels, order, filter, plan=plan)
    return EncodedBatch(dst, slots_dev, slots, length, status, plan)
