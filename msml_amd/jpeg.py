"""Baseline JPEG decoding on the device, bit-exact with libjpeg (csrc/jpeg.hip), and the MXNet RecordIO reader in
front of it: what mx.image.imdecode / cv2.imread do for every input path of the reference (datasets/load_dataset.py,
eval/verification.py:202-236).

The host parses headers only (parse_jpeg never walks the entropy-coded bytes); the compressed bytes go to the device
and msml_jpeg_decode writes the uint8 pixels libjpeg writes with its defaults (JDCT_ISLOW, fancy upsampling), either as
one [N, H, W, 3] tensor (the DeviceLoaderX / data.augment input) or in the packed (buf, meta) form ijb.align_faces,
mtcnn_align and detect.Detector take.  tests/jpeg_cases.py restates the arithmetic in numpy.
"""
import os
import struct
import threading

import numpy as np
import torch

from ._lib import call, value

DESC_WORDS = 32
HUFF_WORDS = 832
(JD_BASE, JD_BEGIN, JD_END, JD_H, JD_W, JD_NCOMP, JD_HMAX, JD_VMAX, JD_QT, JD_DC, JD_AC, JD_RI, JD_STATUS, JD_MCUX,
 JD_MCUY, JD_WS) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 14, 17, 18, 19, 20, 21

# status[n] of a decode: 1-6 from the device (csrc/jpeg_core.h), 16.. from the parser
STATUS = {
    0: "ok", 1: "a Huffman code that is in no table", 2: "a coefficient index past 63",
    3: "a DC category above 11 or an AC category above 10", 4: "a restart marker missing or out of sequence",
    5: "the data ends before the last MCU", 6: "the output rectangle does not match the image",
    16: "not a JPEG stream, or a malformed header", 17: "progressive JPEG is unsupported",
    18: "arithmetic coding is unsupported", 19: "only 8-bit samples are supported",
    20: "only 1 or 3 components are supported", 21: "unsupported sampling factors (gray, 4:4:4, 4:2:2, 4:2:0 only)",
    22: "only one scan over all components is supported", 23: "a table the scan selects is missing or invalid",
    24: "image size outside 1..32767", 25: "unsupported frame type (extended, lossless or hierarchical)",
    26: "the components are RGB, not YCbCr (Adobe transform 0, or ids 'R' 'G' 'B' without JFIF): unsupported",
}
(BAD_HEADER, PROGRESSIVE, ARITHMETIC, PRECISION, COMPONENTS, SAMPLING, SCAN, TABLES, SIZE, FRAME, COLORSPACE) = \
    range(16, 27)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegDescriptor:
    """What parse_jpeg read from the header.  status 0: a supported stream, every field is set; otherwise `reason`
    says why not and the fields read up to that point are set."""

    def __init__(self):
        self.status = 0
        self.begin = self.end = 0           # byte range of the entropy-coded segment (to the end of the buffer)
        self.height = self.width = 0
        self.components = 0
        self.sampling = ()                  # ((h, v), ...) per component
        self.qsel = self.dcsel = self.acsel = ()
        self.restart_interval = 0
        self.qtables = {}                   # id -> int32 [64], natural order
        self.huffman = {}                   # (class, id) -> (counts [16], symbols)

    @property
    def reason(self):
        return STATUS[self.status]


def _refuse(d, status):
    d.status = status
    return d


def parse_jpeg(data):
    """Walk the marker segments in front of the scan (SOI, APPn / COM, DQT, SOF0, DHT, DRI, SOS) -> JpegDescriptor.
    Never reads the entropy-coded bytes and never guesses: anything but 8-bit baseline Huffman with one interleaved
    scan in gray / 4:4:4 / 4:2:2 / 4:2:0 comes back with a nonzero status.  Three components are YCbCr as libjpeg
    decides it (jdapimin.c default_decompress_parms): a JFIF marker says so; without one, an Adobe APP14 segment with
    transform 0, or the component ids 'R' 'G' 'B', mean RGB stored as it is, which is refused."""
    data = bytes(data)
    d = JpegDescriptor()
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return _refuse(d, BAD_HEADER)
    pos = 2
    frame = None
    jfif, adobe = False, None              # adobe: the transform byte of an APP14 "Adobe" segment
    while True:
        if pos + 2 > n or data[pos] != 0xFF:
            return _refuse(d, BAD_HEADER)
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return _refuse(d, BAD_HEADER)
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9, 0x00) or pos + 2 > n:
            return _refuse(d, BAD_HEADER)
        ln = (data[pos] << 8) | data[pos + 1]
        if ln < 2 or pos + ln > n:
            return _refuse(d, BAD_HEADER)
        seg = data[pos + 2:pos + ln]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                size = 64 * (2 if pq else 1)
                if pq > 1 or tq > 3 or i + 1 + size > len(seg):
                    return _refuse(d, BAD_HEADER)
                raw = np.frombuffer(seg, dtype=">u2" if pq else np.uint8, count=64, offset=i + 1).astype(np.int32)
                q = np.zeros(64, np.int32)
                q[ZIGZAG] = raw
                d.qtables[tq] = q
                i += 1 + size
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    return _refuse(d, BAD_HEADER)
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or i + 17 + total > len(seg):
                    return _refuse(d, BAD_HEADER)
                d.huffman[(tc, th)] = (counts, bytes(seg[i + 17:i + 17 + total]))
                i += 17 + total
        elif m == 0xE0 and seg[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDD:
            if len(seg) != 2:
                return _refuse(d, BAD_HEADER)
            d.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xC0:
            if frame is not None or len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                return _refuse(d, BAD_HEADER)
            frame = seg
            d.height, d.width, d.components = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            d.sampling = tuple((seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15) for c in range(seg[5]))
            d.qsel = tuple(seg[8 + 3 * c] for c in range(seg[5]))
        elif m == 0xC2:
            return _refuse(d, PROGRESSIVE)
        elif m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            return _refuse(d, ARITHMETIC)
        elif m in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7, 0xDE):
            return _refuse(d, FRAME)
        elif m == 0xDA:
            if frame is None or len(seg) < 1:
                return _refuse(d, BAD_HEADER)
            if frame[0] != 8:
                return _refuse(d, PRECISION)
            if d.components not in (1, 3):
                return _refuse(d, COMPONENTS)
            if not (1 <= d.height <= 32767 and 1 <= d.width <= 32767):
                return _refuse(d, SIZE)
            if d.sampling not in (((1, 1),), ((1, 1),) * 3, ((2, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1))):
                return _refuse(d, SAMPLING)
            ns = seg[0]
            if len(seg) != 4 + 2 * ns:
                return _refuse(d, BAD_HEADER)
            ids = [frame[6 + 3 * c] for c in range(d.components)]
            if d.components == 3 and not jfif and (adobe == 0 or (adobe is None and ids == [0x52, 0x47, 0x42])):
                return _refuse(d, COLORSPACE)
            if ns != d.components or [seg[1 + 2 * c] for c in range(ns)] != ids:
                return _refuse(d, SCAN)
            if (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]) != (0, 63, 0):
                return _refuse(d, SCAN)
            d.dcsel = tuple(seg[2 + 2 * c] >> 4 for c in range(ns))
            d.acsel = tuple(seg[2 + 2 * c] & 15 for c in range(ns))
            for c in range(ns):
                if d.qsel[c] not in d.qtables or (0, d.dcsel[c]) not in d.huffman or (1, d.acsel[c]) not in d.huffman:
                    return _refuse(d, TABLES)
                if huffman_lookup(*d.huffman[(0, d.dcsel[c])]) is None or \
                        huffman_lookup(*d.huffman[(1, d.acsel[c])]) is None:
                    return _refuse(d, TABLES)
            d.begin, d.end = pos + ln, n
            return d
        # APPn, COM and everything else with a length: skipped
        pos += ln


class HeaderCache:
    """parse_jpeg, remembering whole headers (SOI .. end of SOS): the records of one dataset carry the same header byte
    for byte (same size, same tables), so all but the first cost one slice and one dictionary lookup per distinct
    header length.  Holds at most `capacity` headers; past that it parses without remembering (`full` counts those).
    The descriptors it hands out share their table dictionaries: they are read, never written.  Owned by whoever
    packs many batches (RecordFaceSource has one); pack_jpegs without one parses every header."""

    def __init__(self, capacity=256):
        self.capacity, self.full = capacity, 0
        self.headers = {}
        self.lengths = []

    def parse(self, data):
        import copy
        data = bytes(data)
        for ln in self.lengths:
            d = self.headers.get(data[:ln])
            if d is not None:
                d = copy.copy(d)
                d.end = len(data)
                return d
        d = parse_jpeg(data)
        if d.status == 0:
            if len(self.headers) < self.capacity:
                self.headers[data[:d.begin]] = d
                if d.begin not in self.lengths:
                    self.lengths.append(d.begin)
            else:
                self.full += 1
        return d


_LOOKUPS = {}


def huffman_lookup(counts, symbols):
    """The lookup form csrc/jpeg_core.h reads: int32 [832] = 9-bit lookahead (length << 8 | symbol), maxcode[18],
    valoff[17], huffval[256].  None for counts that do not form a prefix code."""
    key = (bytes(counts), bytes(symbols))
    if key in _LOOKUPS:
        return _LOOKUPS[key]
    t = np.zeros(HUFF_WORDS, np.int32)
    t[512:530] = -1
    code, p, ok = 0, 0, True
    for ln in range(1, 17):
        cnt = counts[ln - 1]
        if code + cnt > (1 << ln):
            ok = False
            break
        if cnt:
            t[530 + ln] = p - code
            for k in range(cnt):
                if ln <= 9:
                    lo = (code + k) << (9 - ln)
                    t[lo:lo + (1 << (9 - ln))] = (ln << 8) | symbols[p + k]
            t[512 + ln] = code + cnt - 1
            p += cnt
            code += cnt
        code <<= 1
    if ok:
        t[547:547 + len(symbols)] = np.frombuffer(bytes(symbols), np.uint8)
    _LOOKUPS[key] = t if ok else None
    return _LOOKUPS[key]


class JpegBatch:
    """pack_jpegs' result: everything msml_jpeg_decode reads, on the host (pinned when a GPU is present).
    streams uint8 [bytes]: the byte strings back to back at 4-byte-aligned offsets; desc int32 [N, 32]; qtabs int32
    [nq, 64] (natural order) and htabs int32 [nh, 832] (lookup form), each distinct table once; descriptors: the
    JpegDescriptor of every stream; ws_bytes: the workspace the decode needs."""

    def __init__(self, streams, desc, qtabs, htabs, descriptors, ws_bytes):
        self.streams, self.desc, self.qtabs, self.htabs = streams, desc, qtabs, htabs
        self.descriptors, self.ws_bytes = descriptors, ws_bytes
        self._dev = None

    def __len__(self):
        return self.desc.shape[0]

    @property
    def status(self):
        return self.desc[:, JD_STATUS].numpy()

    @property
    def sizes(self):
        return [(d.height, d.width) for d in self.descriptors]

    def to_device(self, device="cuda"):
        """(streams, desc, qtabs, htabs) on the device, copied once (non_blocking, on the current stream)."""
        if self._dev is None or self._dev[0].device != torch.device(device):
            self._dev = tuple(t.to(device, non_blocking=True) for t in (self.streams, self.desc, self.qtabs, self.htabs))
        return self._dev


def _pinned(shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=torch.cuda.is_available())


def pack_jpegs(streams, cache=None):
    """A list of JPEG byte strings -> JpegBatch.  Streams the parser refuses keep their place with their status.
    cache: a HeaderCache, for callers that pack batch after batch of one dataset."""
    if not isinstance(streams, (list, tuple)) or len(streams) == 0:
        raise ValueError("pack_jpegs: needs a non-empty list of byte strings")
    n = len(streams)
    parse = cache.parse if cache is not None else parse_jpeg
    descs = [parse(s) for s in streams]
    qidx, hidx, qtabs, htabs = {}, {}, [], []

    def q_index(q):
        k = q.tobytes()
        if k not in qidx:
            qidx[k] = len(qtabs)
            qtabs.append(q)
        return qidx[k]

    def h_index(ch):
        k = (bytes(ch[0]), bytes(ch[1]))
        if k not in hidx:
            hidx[k] = len(htabs)
            htabs.append(huffman_lookup(*ch))
        return hidx[k]

    desc = _pinned((n, DESC_WORDS), torch.int32)
    dn = desc.numpy()
    dn[...] = 0
    off = 0
    offs = []
    for i, (s, d) in enumerate(zip(streams, descs)):
        offs.append(off)
        dn[i, JD_STATUS] = d.status
        if d.status:
            continue
        hm, vm = d.sampling[0]
        dn[i, JD_BASE], dn[i, JD_BEGIN], dn[i, JD_END] = off // 4, d.begin, d.end
        dn[i, JD_H], dn[i, JD_W], dn[i, JD_NCOMP], dn[i, JD_HMAX], dn[i, JD_VMAX] = d.height, d.width, d.components, hm, vm
        for c in range(d.components):
            dn[i, JD_QT + c] = q_index(d.qtables[d.qsel[c]])
            dn[i, JD_DC + c] = h_index(d.huffman[(0, d.dcsel[c])])
            dn[i, JD_AC + c] = h_index(d.huffman[(1, d.acsel[c])])
        dn[i, JD_RI] = d.restart_interval
        dn[i, JD_MCUX], dn[i, JD_MCUY] = -(-d.width // (8 * hm)), -(-d.height // (8 * vm))
        off += (len(s) + 3) & ~3
        if off >= 2 ** 33:
            raise ValueError("pack_jpegs: more than 8 GiB of streams in one batch")
    buf = _pinned(max(off, 4), torch.uint8)
    flat = buf.numpy()
    for s, d, o in zip(streams, descs, offs):
        if d.status == 0:
            flat[o:o + len(s)] = np.frombuffer(bytes(s), np.uint8)
            flat[o + len(s):(o + len(s) + 3) & ~3] = 0
    qt = _pinned((max(len(qtabs), 1), 64), torch.int32)
    ht = _pinned((max(len(htabs), 1), HUFF_WORDS), torch.int32)
    qt.numpy()[...] = np.stack(qtabs) if qtabs else 1
    ht.numpy()[...] = np.stack(htabs) if htabs else 0
    ws_bytes = 0
    if any(d.status == 0 for d in descs):
        ws_bytes = value("msml_jpeg_workspace", desc.data_ptr(), n)
        if ws_bytes <= 0:
            raise RuntimeError("msml_jpeg_workspace refused the descriptors")
    return JpegBatch(buf, desc, qt, ht, descs, ws_bytes)


def _raise_first(status, what):
    bad = np.flatnonzero(status)
    if bad.size:
        i = int(bad[0])
        raise ValueError("%s: image %d: %s (status %d)" % (what, i, STATUS.get(int(status[i]), "?"), int(status[i])))


@torch.no_grad()
def decode_into(batch, dst, meta, channels=3, order="rgb", ws=None, status=None):
    """msml_jpeg_decode of a JpegBatch into the caller's buffers, on the current stream: dst a uint8 tensor on the
    device, meta int64 [N][4] = byte offset in dst, H, W, pitch -- numpy (uploaded here: a copy from pageable memory,
    for which the host waits) or a tensor already on the device (the device checks every row against its stream and
    against dst.numel(): a row that does not fit gives status 6 and writes nothing).  ws: uint8 on the device, at
    least batch.ws_bytes (allocated when None); status: int32 [N] on the device (allocated when None), returned."""
    n = len(batch)
    device = dst.device
    if isinstance(meta, torch.Tensor):
        if meta.dtype != torch.int64 or tuple(meta.shape) != (n, 4) or meta.device != device or not meta.is_contiguous():
            raise ValueError("decode_into: a meta tensor must be contiguous int64 [%d][4] on %s" % (n, device))
        meta_dev = meta
    else:
        meta = np.ascontiguousarray(meta, dtype=np.int64)
        if meta.shape != (n, 4):
            raise ValueError("decode_into: meta must be [%d][4]" % n)
        meta_dev = torch.from_numpy(meta).to(device)
    streams, desc, qtabs, htabs = batch.to_device(device)
    if ws is None:
        ws = torch.empty(max(batch.ws_bytes, 16), dtype=torch.uint8, device=device)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=device)
    call("msml_jpeg_decode", streams, streams.numel(), desc, batch.desc.data_ptr(), qtabs, qtabs.shape[0], htabs,
         htabs.shape[0], dst, dst.numel(), meta_dev, channels, 1 if order == "bgr" else 0, status, ws, ws.numel(), n)
    return status


_UNIFORM_META = {}       # (n, h, w, channels, device) -> meta of a contiguous [n, h, w, channels] tensor, on the device


def _uniform_meta(n, h, w, channels, device):
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


@torch.no_grad()
def decode_batch(batch, size=None, order="rgb", strict=True, channels=3, device="cuda"):
    """Decode a JpegBatch (or a list of byte strings) on the device, on the current stream.

    size=(H, W): uint8 [N, H, W, 3] ([N, H, W] for channels=1); an image of another size is a ValueError.
    size=None: (buf, meta) in the packed form of ijb.pack_images (meta int64 numpy [N][4] = byte offset, H, W, pitch).
    order: "rgb" (imdecode) or "bgr" (cv2.imread); a gray stream replicates Y.  channels=1 takes gray streams only.
    strict=True: ValueError naming the first failing image and why (this reads the statuses back: a synchronisation);
    strict=False: the int32 status tensor [N] comes back as the last element instead, failing images hold unspecified
    pixels.  A batch with no supported stream launches nothing."""
    if order not in ("rgb", "bgr"):
        raise ValueError("decode_batch: order must be 'rgb' or 'bgr'")
    if channels not in (1, 3):
        raise ValueError("decode_batch: channels must be 1 or 3")
    if not isinstance(batch, JpegBatch):
        batch = pack_jpegs(batch)
    n = len(batch)
    host = batch.status
    if strict:
        _raise_first(host, "decode_batch")
    ok = host == 0
    hw = np.array([(d.height, d.width) if o else (1, 1) for d, o in zip(batch.descriptors, ok)], np.int64)
    if channels == 1:
        for i in np.flatnonzero(ok):
            if batch.descriptors[i].components != 1:
                raise ValueError("decode_batch: channels=1 takes gray streams; image %d has 3 components" % i)
    meta = np.empty((n, 4), np.int64)
    if size is not None:
        h, w = int(size[0]), int(size[1])
        for i in np.flatnonzero(ok):
            if tuple(hw[i]) != (h, w):
                raise ValueError("decode_batch: image %d is %d x %d, not %d x %d" % (i, hw[i, 0], hw[i, 1], h, w))
        out = torch.empty((n, h, w, 3) if channels == 3 else (n, h, w), dtype=torch.uint8, device=device)
        dst = out
        meta = _uniform_meta(n, h, w, channels, out.device)      # on the device, uploaded once per shape
    else:
        pitch = (hw[:, 1] * channels + 3) & ~3
        ends = np.cumsum(hw[:, 0] * pitch)
        meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3] = ends - hw[:, 0] * pitch, hw[:, 0], hw[:, 1], pitch
        dst = torch.empty(int(ends[-1]), dtype=torch.uint8, device=device)
        out = (dst, meta)
    if ok.any():
        status = decode_into(batch, dst, meta, channels, order)
    else:
        status = torch.from_numpy(host.astype(np.int32)).to(device)
    if strict:
        _raise_first(status.cpu().numpy(), "decode_batch")
        return out
    return (out, status) if size is not None else out + (status,)


# ---------------------------------------------------------------------------------------------------- RecordIO
RECORD_MAGIC = 0xCED7230A


class RecordFile:
    """MXNet indexed RecordIO (mx.recordio.MXIndexedRecordIO + unpack) without mxnet.  A record is uint32 magic
    0xced7230a, uint32 whose low 29 bits are the payload length (a nonzero continuation flag in the upper 3 bits is
    unsupported), the payload padded to 4 bytes.  The payload is IRHeader `<IfQQ` (flag, label, id, id2), then `flag`
    float32 labels when flag > 0, then the image bytes.  The .idx file holds `key\\toffset` lines."""

    def __init__(self, rec_path, idx_path):
        self.rec_path = rec_path
        self.index = {}
        self.keys = []
        with open(idx_path) as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                k, o = line.split("\t")
                self.index[int(k)] = int(o)
                self.keys.append(int(k))
        self._f = open(rec_path, "rb")
        self._lock = threading.Lock()        # seek + read of one record: readers on several threads share the handle
        self.header0 = None
        self.img_idx = np.array(self.keys, dtype=np.int64)
        if 0 in self.index:                                  # load_dataset.py:51-57
            header, _ = self.read_idx(0)
            if header[0] > 0:
                label = header[1]
                self.header0 = (int(label[0]), int(label[1]))
                self.img_idx = np.arange(1, int(label[0]), dtype=np.int64)

    def close(self):
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def read_idx(self, i):
        """-> ((flag, label, id, id2), image bytes); label is a float, or a float32 array of `flag` values."""
        if i not in self.index:
            raise KeyError("record %d is not in the index" % i)
        with self._lock:
            self._f.seek(self.index[i])
            head = self._f.read(8)
            if len(head) != 8:
                raise ValueError("record %d: the file ends inside the record header" % i)
            magic, lrec = struct.unpack("<II", head)
            if magic != RECORD_MAGIC:
                raise ValueError("record %d: bad magic 0x%08x" % (i, magic))
            if lrec >> 29:
                raise ValueError("record %d: continued (multi-part) records are unsupported" % i)
            length = lrec & ((1 << 29) - 1)
            payload = self._f.read(length)
        if len(payload) != length or length < 24:
            raise ValueError("record %d: truncated payload" % i)
        flag, label, id1, id2 = struct.unpack("<IfQQ", payload[:24])
        body = payload[24:]
        if flag > 0:
            if len(body) < 4 * flag:
                raise ValueError("record %d: %d labels do not fit the payload" % (i, flag))
            label = np.frombuffer(body[:4 * flag], dtype="<f4").copy()
            body = body[4 * flag:]
        return (flag, label, id1, id2), body


class RecordFaceSource:
    """The record reader SynthFaceSource stands in for: yields (JpegBatch, labels int64 [B]) from root/train.rec, in
    index order (shuffle=False) or in a seeded permutation per pass.  masks=True (p_mask > 0): yields (JpegBatch of the
    faces, JpegBatch of the mask_out records, JpegBatch of the mask records, rows int32 [B], labels) with the renders
    of the samples data.mask_flags(seed, k * B, B, p_mask) selects only, rows[n] = the render of face n or -1 -- the
    flags DeviceLoaderX(seed=seed, p_mask=p_mask) draws for batch k of the pass.  close() (or `with`) closes the
    record files."""

    def __init__(self, root, batch, steps=None, shuffle=False, seed=1, masks=False, p_mask=0.2):
        self.rec = RecordFile(os.path.join(root, "train.rec"), os.path.join(root, "train.idx"))
        self.batch, self.steps, self.shuffle, self.seed = batch, steps, shuffle, seed
        self.masks, self.p_mask = masks, p_mask
        if masks:
            self.mask_out = RecordFile(os.path.join(root, "mask_out.rec"), os.path.join(root, "mask_out.idx"))
            self.mask = RecordFile(os.path.join(root, "mask.rec"), os.path.join(root, "mask.idx"))
        self.headers = HeaderCache()         # the records of one dataset share their headers
        if len(self.rec.img_idx) < batch:
            self.close()
            raise ValueError("RecordFaceSource: %d records, fewer than one batch of %d" % (len(self.rec.img_idx), batch))

    def close(self):
        for f in (self.rec, getattr(self, "mask_out", None), getattr(self, "mask", None)):
            if f is not None:
                f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self.rec.img_idx) // self.batch

    def __iter__(self):
        from . import data
        order = self.rec.img_idx
        if self.shuffle:
            order = order[np.random.RandomState(self.seed).permutation(len(order))]
        k = 0
        while self.steps is None or k < self.steps:
            j = k % len(self)
            idx = order[j * self.batch:(j + 1) * self.batch]
            streams, labels = [], []
            for i in idx:
                (_, label, _, _), body = self.rec.read_idx(int(i))
                streams.append(body)
                labels.append(int(label if np.isscalar(label) else label[0]))
            item = (pack_jpegs(streams, self.headers), torch.tensor(labels, dtype=torch.int64))
            if self.masks:
                flags = data.mask_flags(self.seed, k * self.batch, self.batch, self.p_mask)
                rows = np.full(self.batch, -1, np.int32)
                rows[flags] = np.arange(int(flags.sum()), dtype=np.int32)
                sel = [int(i) for i in idx[flags]]
                mo = pack_jpegs([self.mask_out.read_idx(i)[1] for i in sel], self.headers) if sel else None
                mk = pack_jpegs([self.mask.read_idx(i)[1] for i in sel], self.headers) if sel else None
                item = (item[0], mo, mk, torch.from_numpy(rows), item[1])
            if torch.cuda.is_available():
                item = tuple(t.pin_memory() if isinstance(t, torch.Tensor) else t for t in item)
            yield item
            k += 1


@torch.no_grad()
def decode_renders(mask_out, mask, size, device="cuda"):
    """The mask_out / mask records of RecordFaceSource as data.apply takes them: masked uint8 [M, H, W, 3] (RGB),
    mask uint8 [M, H, W] = Image.fromarray(imdecode(mask)).convert('L') (load_dataset.py:167-177): Y of a gray
    stream, (19595 R + 38470 G + 7471 B + 32768) >> 16 of a colour one -- and status int32 [M] on the device: 0, or
    the status of render m's mask_out record, else of its mask record.  A record the parser refused is a ValueError
    naming it.  None (no render in this batch) gives one render that no row points at, so that the shapes data.apply
    checks hold."""
    h, w = size
    if mask_out is None:
        return (torch.zeros(1, h, w, 3, dtype=torch.uint8, device=device),
                torch.full((1, h, w), 255, dtype=torch.uint8, device=device),
                torch.zeros(1, dtype=torch.int32, device=device))
    _raise_first(mask_out.status, "decode_renders: mask_out")
    _raise_first(mask.status, "decode_renders: mask")
    masked, st = decode_batch(mask_out, size=size, strict=False, device=device)
    if all(d.components == 1 for d in mask.descriptors):
        m, st2 = decode_batch(mask, size=size, strict=False, channels=1, device=device)
    else:
        rgb, st2 = decode_batch(mask, size=size, strict=False, device=device)
        rgb = rgb.to(torch.int32)
        m = ((rgb[..., 0] * 19595 + rgb[..., 1] * 38470 + rgb[..., 2] * 7471 + 32768) >> 16).to(torch.uint8)
    return masked, m, torch.where(st != 0, st, st2)
