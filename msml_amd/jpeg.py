"""Baseline JPEG decoding on the device, bit-exact with libjpeg (csrc/jpeg.hip), progressive JPEG behind the keyword
progressive=True (csrc/jpeg_prog.hip), and the MXNet RecordIO reader in front of them: what mx.image.imdecode /
cv2.imread do for every input path of the reference (datasets/load_dataset.py, eval/verification.py:202-236).

The host parses headers only (parse_jpeg never walks the entropy-coded bytes; for a progressive file it looks for the
marker that ends each scan); the compressed bytes go to the device and msml_jpeg_decode / msml_jpeg_decode_scans write
the uint8 pixels libjpeg writes with its defaults (JDCT_ISLOW, fancy upsampling), either as one [N, H, W, 3] tensor
(the DeviceLoaderX / data.augment input) or in the packed (buf, meta) form ijb.align_faces, mtcnn_align and
detect.Detector take.  tests/jpeg_cases.py restates the arithmetic in numpy, tests/jpeg_prog_cases.py the progressive
scans.
"""
import os
import struct
import threading

import numpy as np
import torch

from . import _codec, packed
from ._codec import StreamBatch, pack_streams, pinned, raise_first
from ._lib import call, value

DESC_WORDS = 32
HUFF_WORDS = 832
(JD_BASE, JD_BEGIN, JD_END, JD_H, JD_W, JD_NCOMP, JD_HMAX, JD_VMAX, JD_QT, JD_DC, JD_AC, JD_RI, JD_STATUS, JD_MCUX,
 JD_MCUY, JD_WS, JD_NSCAN, JD_SCAN0) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 14, 17, 18, 19, 20, 21, 22, 23
SCAN_WORDS = 16      # one record of the scan table (csrc/jpeg_prog_core.h)
(JS_BEGIN, JS_END, JS_NCOMP, JS_COMP, JS_TAB, JS_SS, JS_SE, JS_AH, JS_AL, JS_RI) = 0, 1, 2, 3, 6, 9, 10, 11, 12, 13

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
    27: "a progressive scan libjpeg rejects or warns about (parameters, order of the scans, or its components)",
    28: "an incomplete progression: not every coefficient reaches bit 0 before the file ends",
}
(BAD_HEADER, PROGRESSIVE, ARITHMETIC, PRECISION, COMPONENTS, SAMPLING, SCAN, TABLES, SIZE, FRAME, COLORSPACE,
 PROGRESSION, INCOMPLETE) = range(16, 29)

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
        self.progressive = False            # an SOF2 frame, read with parse_jpeg(progressive=True)
        self.scans = []                     # its JpegScans in file order; empty for a baseline stream
        self.coef_bits = None               # [component][64]: the Al each coefficient was last left at, -1 = never sent

    @property
    def reason(self):
        return STATUS[self.status]


class JpegScan:
    """One scan of a progressive stream: components (frame indices), dcsel / acsel (the SOS's selectors), ss, se, ah,
    al, restart_interval (as DRI stood at this SOS), begin / end (byte range of the entropy-coded segment) and tables:
    per component the (counts, symbols) the scan decodes with as DHT stood at this SOS -- the DC table of a first DC
    scan, the AC table of an AC scan, None for a DC refinement, which reads plain bits."""

    def __init__(self, components, dcsel, acsel, ss, se, ah, al, restart_interval, begin, end, tables):
        self.components, self.dcsel, self.acsel = components, dcsel, acsel
        self.ss, self.se, self.ah, self.al = ss, se, ah, al
        self.restart_interval, self.begin, self.end, self.tables = restart_interval, begin, end, tables


def _refuse(d, status):
    d.status = status
    return d


def _bad(d, n):
    """A header that cannot be read: BAD_HEADER in front of the first scan; behind one the file counts as ending there."""
    return _finish(d, n) if d.scans else _refuse(d, BAD_HEADER)


def _finish(d, n):
    """EOI, or the end of what can be read, of a progressive stream: supported when every coefficient reached bit 0
    (jdcoefct.c smoothing_ok then keeps libjpeg's inter-block smoothing off)."""
    d.begin, d.end = d.scans[0].begin, n
    if any(b != 0 for comp in d.coef_bits for b in comp):
        return _refuse(d, INCOMPLETE)
    return d


def _segment_end(data, pos):
    """The first marker at or behind pos that is neither FF 00 nor RSTn: where an entropy-coded segment ends."""
    n = len(data)
    while True:
        pos = data.find(b"\xff", pos)
        if pos < 0 or pos + 1 >= n:
            return n
        m = data[pos + 1]
        if m == 0 or 0xD0 <= m <= 0xD7:
            pos += 2
        elif m == 0xFF:
            pos += 1                        # a fill byte: the marker code follows
        else:
            return pos


def _progressive_scan(d, data, seg, ids, begin):
    """SOS of a progressive stream, by jdmarker.c get_sos and jdphuff.c start_pass_phuff_decoder: the scan is taken
    only with parameters libjpeg accepts without a warning.  -> status (0: appended to d.scans)."""
    ns = seg[0]
    if len(seg) != 4 + 2 * ns:
        return BAD_HEADER
    if not 1 <= ns <= d.components:
        return PROGRESSION
    comps = [ids.index(seg[1 + 2 * c]) if seg[1 + 2 * c] in ids else -1 for c in range(ns)]
    if any(c < 0 for c in comps) or any(b <= a for a, b in zip(comps, comps[1:])):
        return PROGRESSION                  # not of the frame, repeated, or out of frame order
    ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
    if ss > se or se > 63 or (ss == 0 and se != 0) or (ss != 0 and ns != 1) or al > 13 or (ah != 0 and al != ah - 1):
        return PROGRESSION
    for c in comps:
        bits = d.coef_bits[c]
        if ss != 0 and bits[0] < 0:
            return PROGRESSION              # AC before the component's DC
        if bits[ss:se + 1].count(ah if ah else -1) != se + 1 - ss:
            return PROGRESSION              # a refinement without its first scan, a repeated or a skipped pass
    dcsel = tuple(seg[2 + 2 * c] >> 4 for c in range(ns))
    acsel = tuple(seg[2 + 2 * c] & 15 for c in range(ns))
    tables = []
    for i in range(ns):
        if ss == 0 and ah != 0:
            tables.append(None)
            continue
        key = (0, dcsel[i]) if ss == 0 else (1, acsel[i])
        if key not in d.huffman or huffman_lookup(*d.huffman[key]) is None:
            return TABLES
        tables.append(d.huffman[key])
    for c in comps:
        d.coef_bits[c][ss:se + 1] = [al] * (se + 1 - ss)
    d.scans.append(JpegScan(tuple(comps), dcsel, acsel, ss, se, ah, al, d.restart_interval, begin,
                            _segment_end(data, begin), tables))
    return 0


def parse_jpeg(data, progressive=False):
    """Walk the marker segments in front of the scan (SOI, APPn / COM, DQT, SOF0, DHT, DRI, SOS) -> JpegDescriptor.
    Never reads the entropy-coded bytes and never guesses: anything but 8-bit baseline Huffman with one interleaved
    scan in gray / 4:4:4 / 4:2:2 / 4:2:0 comes back with a nonzero status.  Three components are YCbCr as libjpeg
    decides it (jdapimin.c default_decompress_parms): a JFIF marker says so; without one, an Adobe APP14 segment with
    transform 0, or the component ids 'R' 'G' 'B', mean RGB stored as it is, which is refused.

    progressive=True: an SOF2 frame is read like SOF0 and every scan is walked to EOI: `scans` holds each SOS with the
    tables and the restart interval as they stood there, and the byte range of its entropy-coded segment (found by
    looking for the next marker, never by decoding).  Supported when every scan is one libjpeg takes without a warning
    (else PROGRESSION) and every coefficient of every component has reached bit 0 by the end (else INCOMPLETE: libjpeg
    would smooth such a file, differently from version to version)."""
    data = bytes(data)
    d = JpegDescriptor()
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return _refuse(d, BAD_HEADER)
    pos = 2
    frame = None
    jfif, adobe = False, None              # adobe: the transform byte of an APP14 "Adobe" segment
    while True:
        if d.scans and pos + 2 <= n and data[pos] == 0xFF and data[pos + 1] == 0xD9:
            return _finish(d, n)
        if pos + 2 > n or data[pos] != 0xFF:
            return _bad(d, n)
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return _bad(d, n)
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD8, 0xD9, 0x00) or pos + 2 > n:
            return _bad(d, n)
        ln = (data[pos] << 8) | data[pos + 1]
        if ln < 2 or pos + ln > n:
            return _bad(d, n)
        seg = data[pos + 2:pos + ln]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                size = 64 * (2 if pq else 1)
                if pq > 1 or tq > 3 or i + 1 + size > len(seg):
                    return _bad(d, n)
                raw = np.frombuffer(seg, dtype=">u2" if pq else np.uint8, count=64, offset=i + 1).astype(np.int32)
                q = np.zeros(64, np.int32)
                q[ZIGZAG] = raw
                d.qtables[tq] = q
                i += 1 + size
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    return _bad(d, n)
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or i + 17 + total > len(seg):
                    return _bad(d, n)
                d.huffman[(tc, th)] = (counts, bytes(seg[i + 17:i + 17 + total]))
                i += 17 + total
        elif m == 0xE0 and seg[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDD:
            if len(seg) != 2:
                return _bad(d, n)
            d.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xC0 or (m == 0xC2 and progressive):
            if frame is not None or len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                return _bad(d, n)
            frame = seg
            d.progressive = m == 0xC2
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
                return _bad(d, n)
            if frame[0] != 8:
                return _refuse(d, PRECISION)
            if d.components not in (1, 3):
                return _refuse(d, COMPONENTS)
            if not (1 <= d.height <= 32767 and 1 <= d.width <= 32767):
                return _refuse(d, SIZE)
            if d.sampling not in (((1, 1),), ((1, 1),) * 3, ((2, 1), (1, 1), (1, 1)), ((2, 2), (1, 1), (1, 1))):
                return _refuse(d, SAMPLING)
            ns = seg[0]
            ids = [frame[6 + 3 * c] for c in range(d.components)]
            if d.components == 3 and not jfif and (adobe == 0 or (adobe is None and ids == [0x52, 0x47, 0x42])):
                return _refuse(d, COLORSPACE)
            if d.progressive:
                if d.coef_bits is None:
                    if any(q not in d.qtables for q in d.qsel):
                        return _refuse(d, TABLES)
                    d.coef_bits = [[-1] * 64 for _ in range(d.components)]
                st = _progressive_scan(d, data, seg, ids, pos + ln)
                if st:
                    return _bad(d, n) if st == BAD_HEADER else _refuse(d, st)
                pos = d.scans[-1].end
                continue
            if len(seg) != 4 + 2 * ns:
                return _bad(d, n)
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
    packs many batches (RecordFaceSource has one); pack_jpegs without one parses every header.  A progressive stream
    (progressive=True) passes through uncached: its headers run through the whole file."""

    def __init__(self, capacity=256):
        self.capacity, self.full = capacity, 0
        self.headers = {}
        self.lengths = []

    def parse(self, data, progressive=False):
        import copy
        data = bytes(data)
        for ln in self.lengths:
            d = self.headers.get(data[:ln])
            if d is not None:
                d = copy.copy(d)
                d.end = len(data)
                return d
        d = parse_jpeg(data, progressive)
        if d.status == 0 and not d.progressive:
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


class JpegBatch(StreamBatch):
    """pack_jpegs' result: everything msml_jpeg_decode reads, on the host (pinned when a GPU is present).
    streams uint8 [bytes]: the byte strings back to back at 4-byte-aligned offsets; desc int32 [N, 32]; qtabs int32
    [nq, 64] (natural order) and htabs int32 [nh, 832] (lookup form), each distinct table once; descriptors: the
    JpegDescriptor of every stream; ws_bytes: the workspace the decode needs.  scans int32 [ns, 16]: the scan table
    of the progressive streams (pack_jpegs(progressive=True) found some), else None."""

    FIELDS = ("streams", "desc", "qtabs", "htabs")
    STATUS_WORD = JD_STATUS

    def __init__(self, streams, desc, qtabs, htabs, descriptors, ws_bytes, scans=None):
        self.streams, self.desc, self.qtabs, self.htabs = streams, desc, qtabs, htabs
        self.descriptors, self.ws_bytes, self.scans = descriptors, ws_bytes, scans
        if scans is not None:
            self.FIELDS = JpegBatch.FIELDS + ("scans",)
        self._dev = None


def pack_jpegs(streams, cache=None, progressive=False):
    """A list of JPEG byte strings -> JpegBatch.  Streams the parser refuses keep their place with their status.
    cache: a HeaderCache, for callers that pack batch after batch of one dataset.  progressive=True: progressive
    streams are taken too (parse_jpeg), baseline and progressive in any mix; their scans go into one table beside
    `desc`, one record per scan, with table selectors as indices into the deduplicated htabs."""
    if not isinstance(streams, (list, tuple)) or len(streams) == 0:
        raise ValueError("pack_jpegs: needs a non-empty list of byte strings")
    n = len(streams)
    parse = cache.parse if cache is not None else parse_jpeg
    descs = [parse(s, progressive) for s in streams] if progressive else [parse(s) for s in streams]
    records = []
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

    desc = pinned((n, DESC_WORDS), torch.int32)
    dn = desc.numpy()
    dn[...] = 0
    buf, offs = pack_streams([len(s) if d.status == 0 else 0 for s, d in zip(streams, descs)], "pack_jpegs")
    for i, (off, d) in enumerate(zip(offs, descs)):
        dn[i, JD_STATUS] = d.status
        if d.status:
            continue
        hm, vm = d.sampling[0]
        dn[i, JD_BASE], dn[i, JD_BEGIN], dn[i, JD_END] = off // 4, d.begin, d.end
        dn[i, JD_H], dn[i, JD_W], dn[i, JD_NCOMP], dn[i, JD_HMAX], dn[i, JD_VMAX] = d.height, d.width, d.components, hm, vm
        for c in range(d.components):
            dn[i, JD_QT + c] = q_index(d.qtables[d.qsel[c]])
            if not d.scans:
                dn[i, JD_DC + c] = h_index(d.huffman[(0, d.dcsel[c])])
                dn[i, JD_AC + c] = h_index(d.huffman[(1, d.acsel[c])])
        if d.scans:
            dn[i, JD_NSCAN], dn[i, JD_SCAN0] = len(d.scans), len(records)
            for sc in d.scans:
                r = [0] * SCAN_WORDS
                r[JS_BEGIN], r[JS_END], r[JS_NCOMP] = sc.begin, sc.end, len(sc.components)
                for c, (comp, t) in enumerate(zip(sc.components, sc.tables)):
                    r[JS_COMP + c], r[JS_TAB + c] = comp, (h_index(t) if t is not None else 0)
                r[JS_SS], r[JS_SE], r[JS_AH], r[JS_AL], r[JS_RI] = sc.ss, sc.se, sc.ah, sc.al, sc.restart_interval
                records.append(r)
        dn[i, JD_RI] = d.restart_interval
        dn[i, JD_MCUX], dn[i, JD_MCUY] = -(-d.width // (8 * hm)), -(-d.height // (8 * vm))
    flat = buf.numpy()
    for s, d, o in zip(streams, descs, offs):
        if d.status == 0:
            flat[o:o + len(s)] = np.frombuffer(bytes(s), np.uint8)
    qt = pinned((max(len(qtabs), 1), 64), torch.int32)
    ht = pinned((max(len(htabs), 1), HUFF_WORDS), torch.int32)
    qt.numpy()[...] = np.stack(qtabs) if qtabs else 1
    ht.numpy()[...] = np.stack(htabs) if htabs else 0
    ws_bytes = 0
    if any(d.status == 0 for d in descs):
        ws_bytes = value("msml_jpeg_workspace", desc.data_ptr(), n)
        if ws_bytes <= 0:
            raise RuntimeError("msml_jpeg_workspace refused the descriptors")
    scans = None
    if records:
        scans = pinned((len(records), SCAN_WORDS), torch.int32)
        scans.numpy()[...] = np.array(records, np.int32)
    return JpegBatch(buf, desc, qt, ht, descs, ws_bytes, scans)


@torch.no_grad()
def decode_into(batch, dst, meta, channels=3, order="rgb", ws=None, status=None, progressive=False):
    """msml_jpeg_decode (msml_jpeg_decode_scans when the batch carries a scan table, which only a batch packed with
    progressive=True does; the keyword itself changes nothing for a packed batch) of a JpegBatch into the caller's buffers, on the current stream: dst a uint8 tensor on the
    device, meta int64 [N][4] = byte offset in dst, H, W, pitch -- numpy (uploaded here: a copy from pageable memory,
    for which the host waits) or a tensor already on the device (the device checks every row against its stream and
    against dst.numel(): a row that does not fit gives status 6 and writes nothing).  ws: uint8 on the device, at
    least batch.ws_bytes (allocated when None); status: int32 [N] on the device (allocated when None), returned."""
    n = len(batch)
    device = dst.device
    meta_dev = packed.meta_on_device(meta, n, device, "decode_into")
    streams, desc, qtabs, htabs = batch.to_device(device)[:4]
    if ws is None:
        ws = torch.empty(max(batch.ws_bytes, 16), dtype=torch.uint8, device=device)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=device)
    if batch.scans is not None:
        call("msml_jpeg_decode_scans", streams, streams.numel(), desc, batch.desc.data_ptr(), batch.to_device(device)[4],
             batch.scans.data_ptr(), batch.scans.shape[0], qtabs, qtabs.shape[0], htabs, htabs.shape[0], dst, dst.numel(),
             meta_dev, channels, 1 if order == "bgr" else 0, status, ws, ws.numel(), n)
        return status
    call("msml_jpeg_decode", streams, streams.numel(), desc, batch.desc.data_ptr(), qtabs, qtabs.shape[0], htabs,
         htabs.shape[0], dst, dst.numel(), meta_dev, channels, 1 if order == "bgr" else 0, status, ws, ws.numel(), n)
    return status


@torch.no_grad()
def decode_batch(batch, size=None, order="rgb", strict=True, channels=3, device="cuda", progressive=False):
    """Decode a JpegBatch (or a list of byte strings) on the device, on the current stream.

    size=(H, W): uint8 [N, H, W, 3] ([N, H, W] for channels=1); an image of another size is a ValueError.
    size=None: (buf, meta) in the packed form of ijb.pack_images (meta int64 numpy [N][4] = byte offset, H, W, pitch).
    order: "rgb" (imdecode) or "bgr" (cv2.imread); a gray stream replicates Y.  channels=1 takes gray streams only.
    strict=True: ValueError naming the first failing image and why (this reads the statuses back: a synchronisation);
    strict=False: the int32 status tensor [N] comes back as the last element instead, failing images hold unspecified
    pixels.  A batch with no supported stream launches nothing.  progressive=True: a list of byte strings is packed
    with pack_jpegs(progressive=True), so progressive streams decode too, in any mix with baseline ones."""
    if progressive and not isinstance(batch, JpegBatch):
        batch = pack_jpegs(batch, progressive=True)
    return _codec.decode_batch(_CODEC, batch, size, order, strict, channels, device)


_CODEC = _codec.Codec(pack_jpegs, JpegBatch, (1, 3), lambda d: None if d.components == 1 else "3 components",
                      decode_into, STATUS)


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
    record files.  raw=True: yields (list of byte strings, labels) instead, for records whose payloads are PNG files
    (png.encode_batch through write_faces) or a mix: imageio.decode_images reads those."""

    def __init__(self, root, batch, steps=None, shuffle=False, seed=1, masks=False, p_mask=0.2, progressive=False,
                 raw=False):
        self.progressive = progressive       # records may be progressive JPEG (pack_jpegs)
        self.raw = raw                       # yield the payloads as byte strings (PNG or mixed records: imageio.decode_images)
        if raw and masks:
            raise ValueError("RecordFaceSource: raw=True yields the face payloads only (no masks)")
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
            if self.raw:
                yield streams, torch.tensor(labels, dtype=torch.int64)
                k += 1
                continue
            item = (pack_jpegs(streams, self.headers, self.progressive), torch.tensor(labels, dtype=torch.int64))
            if self.masks:
                flags = data.mask_flags(self.seed, k * self.batch, self.batch, self.p_mask)
                rows = np.full(self.batch, -1, np.int32)
                rows[flags] = np.arange(int(flags.sum()), dtype=np.int32)
                sel = [int(i) for i in idx[flags]]
                mo = pack_jpegs([self.mask_out.read_idx(i)[1] for i in sel], self.headers, self.progressive) if sel else None
                mk = pack_jpegs([self.mask.read_idx(i)[1] for i in sel], self.headers, self.progressive) if sel else None
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
    raise_first(mask_out.status, "decode_renders: mask_out", STATUS)
    raise_first(mask.status, "decode_renders: mask", STATUS)
    masked, st = decode_batch(mask_out, size=size, strict=False, device=device)
    if all(d.components == 1 for d in mask.descriptors):
        m, st2 = decode_batch(mask, size=size, strict=False, channels=1, device=device)
    else:
        rgb, st2 = decode_batch(mask, size=size, strict=False, device=device)
        rgb = rgb.to(torch.int32)
        m = ((rgb[..., 0] * 19595 + rgb[..., 1] * 38470 + rgb[..., 2] * 7471 + 32768) >> 16).to(torch.uint8)
    return masked, m, torch.where(st != 0, st, st2)


# ---------------------------------------------------------------------------------------------------- encoding
# Baseline JPEG encoding on the device, byte for byte what libjpeg writes with Pillow's save() options (csrc/jpeg_enc.hip,
# csrc/jpeg_enc_core.h): PIL.Image.save of eval/align_dataset.py:52-75 and iterate_pku.py, and the entropy-coded data of
# mx.recordio.pack_img in datasets/3d_tools/cvt_casia_webface.py:57 and cvt_casia_webface_masked.py:108-114.  pack_img
# goes through cv2.imencode: the same library with the same defaults, so its scan should equal Pillow's at the same
# quality and sampling, but its header bytes were never compared -- byte equality is claimed with Pillow only.
ENC_DESC_WORDS = 12
(JE_SAMP, JE_H, JE_W, JE_QT, JE_RI, JE_HOFF, JE_HLEN, JE_WS) = 0, 1, 2, 3, 5, 6, 7, 8
SAMPLINGS = {"gray": 0, "444": 1, "422": 2, "420": 3}
ENCODE_STATUS = {0: "ok", 1: "the meta row is not this image inside the source buffer",
                 2: "the slot is outside the output buffer or too small for the stream"}

# Annex K.1 / K.2, natural order
_BASE_Q = (np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17,
                     22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78,
                     87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64),
           np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66,
                     99, 99, 99, 99, 99, 99] + [99] * 32, np.int64))
# Annex K.3 - K.6: (class, id) -> (counts [16], symbols)
_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839"
    "3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
    "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
STD_HUFFMAN = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bytes(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], bytes(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC_LUMA),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC_CHROMA),
}


def quant_tables(quality):
    """libjpeg's jpeg_set_quality(quality, force_baseline=TRUE): (luma, chroma) int32 [64] in natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be 1..100, got %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * scale + 50) // 100, 1, 255).astype(np.int32) for b in _BASE_Q)


def _segment(marker, body):
    return bytes((0xFF, marker)) + struct.pack(">H", len(body) + 2) + body


def build_header(height, width, sampling, qtabs, restart=0):
    """SOI .. SOS as libjpeg writes them for Pillow (jcmarker.c): APP0 JFIF 1.01 with density 1 x 1 and no unit, one DQT
    per table, SOF0, one DHT per standard table (DC 0, AC 0, DC 1, AC 1; a gray stream has the first two), DRI when a
    restart interval is set, SOS.  sampling: a key of SAMPLINGS; qtabs: (luma, chroma) in natural order."""
    s = SAMPLINGS[sampling] if isinstance(sampling, str) else int(sampling)
    nc = 1 if s == 0 else 3
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if nc == 3 else 1):
        out += _segment(0xDB, bytes((t,)) + bytes(int(v) for v in np.asarray(qtabs[t])[ZIGZAG]))
    comps = [(1, (0x11, 0x11, 0x21, 0x22)[s], 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if nc == 3 else [])
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, nc) + b"".join(bytes(c) for c in comps))
    for th in range(2 if nc == 3 else 1):
        for tc in (0, 1):
            counts, symbols = STD_HUFFMAN[(tc, th)]
            out += _segment(0xC4, bytes(((tc << 4) | th,)) + bytes(counts) + symbols)
    if restart:
        out += _segment(0xDD, struct.pack(">H", restart))
    scan = bytes((nc,)) + b"".join(bytes((c[0], 0x11 * c[2])) for c in comps) + b"\x00\x3f\x00"
    return out + _segment(0xDA, scan)


class EncodePlan:
    """Everything msml_jpeg_encode reads besides the pixels, built on the host from sizes and options: desc int32
    [N, 12] (pinned), qtabs int32 [nq, 64] (each distinct table once), headers uint8 (each distinct header once),
    bounds int64 [N] = msml_jpeg_encode_bound of every image rounded up to 4, ws_bytes, and what the decoder needs to read
    the streams back (recompress)."""

    def __init__(self, sizes, quality=75, sampling="420", restart=0):
        n = len(sizes)
        if n == 0:
            raise ValueError("encode: needs at least one image")

        def per_image(v, name):
            if isinstance(v, (str, int, np.integer)):
                return [v] * n
            v = list(v)
            if len(v) != n:
                raise ValueError("encode: %s has %d values for %d images" % (name, len(v), n))
            return v

        quality, sampling, restart = per_image(quality, "quality"), per_image(sampling, "sampling"), per_image(restart, "restart")
        self.n, self.sizes = n, [(int(h), int(w)) for h, w in sizes]
        self.desc = pinned((n, ENC_DESC_WORDS), torch.int32)
        dn = self.desc.numpy()
        dn[...] = 0
        qidx, qtabs, hidx, headers, hoff = {}, [], {}, [], 0
        self.bounds = np.zeros(n, np.int64)
        for i, ((h, w), q, s, r) in enumerate(zip(self.sizes, quality, sampling, restart)):
            if s not in SAMPLINGS:
                raise ValueError("encode: sampling must be one of %s, got %r" % (sorted(SAMPLINGS), s))
            q, r = int(q), int(r)
            if not (1 <= h <= 32767 and 1 <= w <= 32767):
                raise ValueError("encode: image %d is %d x %d, sizes must be 1..32767" % (i, h, w))
            if not 0 <= r <= 65535:
                raise ValueError("encode: restart must be 0..65535 MCUs, got %d" % r)
            if q not in qidx:
                qidx[q] = len(qtabs)
                qtabs.extend(quant_tables(q))
            key = (h, w, s, q, r)
            if key not in hidx:
                hb = build_header(h, w, s, quant_tables(q), r)
                hidx[key] = (hoff, len(hb))
                headers.append(hb)
                hoff += len(hb)
            dn[i, JE_SAMP], dn[i, JE_H], dn[i, JE_W], dn[i, JE_RI] = SAMPLINGS[s], h, w, r
            dn[i, JE_QT], dn[i, JE_QT + 1] = qidx[q], qidx[q] + 1
            dn[i, JE_HOFF], dn[i, JE_HLEN] = hidx[key]
            self.bounds[i] = (value("msml_jpeg_encode_bound", h, w, SAMPLINGS[s], r, hidx[key][1]) + 3) & ~3
        self.qtabs = pinned((len(qtabs), 64), torch.int32)
        self.qtabs.numpy()[...] = np.stack(qtabs)
        hb = b"".join(headers)
        self.headers = pinned((len(hb) + 3) & ~3, torch.uint8)
        self.headers.numpy()[:len(hb)] = np.frombuffer(hb, np.uint8)
        self.headers.numpy()[len(hb):] = 0
        self.ws_bytes = value("msml_jpeg_encode_workspace", self.desc.data_ptr(), n)
        if self.ws_bytes <= 0:
            raise RuntimeError("msml_jpeg_encode_workspace refused the descriptors")
        self._dev = None
        self._decode = {}

    def to_device(self, device="cuda"):
        if self._dev is None or self._dev[0].device != torch.device(device):
            self._dev = tuple(t.to(device, non_blocking=True) for t in (self.desc, self.qtabs, self.headers))
        return self._dev

    def decode_batch_of(self, buf, slots):
        """The JpegBatch that decodes the streams this plan's encode wrote into `buf` at `slots` (numpy [N][2], offsets
        multiples of 4), built without reading anything back: the header length is known, and the end of the stream is
        given as the end of the slot, which msml_jpeg_decode allows (it stops at the EOI marker after the last MCU)."""
        key = slots.tobytes()
        if key not in self._decode:
            n = self.n
            en = self.desc.numpy()
            desc = pinned((n, DESC_WORDS), torch.int32)
            dn = desc.numpy()
            dn[...] = 0
            lookups = [huffman_lookup(*STD_HUFFMAN[k]) for k in ((0, 0), (1, 0), (0, 1), (1, 1))]
            for i in range(n):
                s = int(en[i, JE_SAMP])
                hm, vm = (2 if s >= 2 else 1), (2 if s == 3 else 1)
                h, w = self.sizes[i]
                dn[i, JD_BASE], dn[i, JD_BEGIN], dn[i, JD_END] = slots[i, 0] // 4, en[i, JE_HLEN], slots[i, 1]
                dn[i, JD_H], dn[i, JD_W], dn[i, JD_NCOMP], dn[i, JD_HMAX], dn[i, JD_VMAX] = h, w, 1 if s == 0 else 3, hm, vm
                dn[i, JD_QT:JD_QT + 3] = en[i, JE_QT], en[i, JE_QT + 1], en[i, JE_QT + 1]
                dn[i, JD_DC:JD_DC + 3] = 0, 2, 2
                dn[i, JD_AC:JD_AC + 3] = 1, 3, 3
                dn[i, JD_RI] = en[i, JE_RI]
                dn[i, JD_MCUX], dn[i, JD_MCUY] = -(-w // (8 * hm)), -(-h // (8 * vm))
            ht = pinned((4, HUFF_WORDS), torch.int32)
            ht.numpy()[...] = np.stack(lookups)
            ws_bytes = value("msml_jpeg_workspace", desc.data_ptr(), n)
            if ws_bytes <= 0:
                raise RuntimeError("msml_jpeg_workspace refused the descriptors")
            if len(self._decode) >= 4:
                self._decode.clear()
            self._decode[key] = (desc, ht, ws_bytes)
        desc, ht, ws_bytes = self._decode[key]
        return JpegBatch(buf, desc, self.qtabs, ht, None, ws_bytes)


_PLANS = {}


def _plan(sizes, quality, sampling, restart):
    """EncodePlan, remembered for a uniform batch with scalar options (what a loop over batches of crops asks for)."""
    scalar = all(isinstance(v, (str, int, np.integer)) for v in (quality, sampling, restart))
    if scalar and len(set(sizes)) == 1:
        key = (len(sizes), sizes[0], int(quality), sampling, int(restart))
        if key not in _PLANS:
            if len(_PLANS) >= 16:
                _PLANS.clear()
            _PLANS[key] = EncodePlan(sizes, quality, sampling, restart)
        return _PLANS[key]
    return EncodePlan(sizes, quality, sampling, restart)


class EncodedBatch:
    """encode_batch's result, all on the device: buf uint8 (the slots), slots int64 [N][2] = byte offset and capacity of
    each image's slot (slots_host: the same in numpy), length int32 [N] (0 for an image that failed), status int32 [N]
    (ENCODE_STATUS).  Image n is buf[slots[n, 0] : slots[n, 0] + length[n]]."""

    def __init__(self, buf, slots, slots_host, length, status, plan):
        self.buf, self.slots, self.slots_host, self.length, self.status, self.plan = buf, slots, slots_host, length, status, plan

    def __len__(self):
        return self.length.shape[0]

    def to_bytes(self, strict=True):
        """-> a list of N byte strings.  One device-to-host copy (the slots, the lengths and the statuses together) for
        which the host waits.  strict: ValueError naming the first image whose status is not 0; otherwise that image's
        string is empty."""
        n = len(self)
        tail = torch.stack([self.length, self.status]).view(torch.uint8).reshape(-1)
        host = torch.cat([self.buf.reshape(-1), tail]).cpu().numpy()
        ls = host[self.buf.numel():].view(np.int32).reshape(2, n)
        if strict:
            bad = np.flatnonzero(ls[1])
            if bad.size:
                i = int(bad[0])
                table = getattr(self.plan, "STATUS", ENCODE_STATUS)       # a PNG plan brings its own reasons
                raise ValueError("encode: image %d: %s (status %d)" % (i, table.get(int(ls[1, i]), "?"), ls[1, i]))
        return [host[o:o + l].tobytes() for o, l in zip(self.slots_host[:, 0], ls[0])]


def _source(images, channels, device):
    """-> (src uint8 flat on the device, meta int64 numpy [N][4] or None for a contiguous tensor, sizes, channels)."""
    if isinstance(images, (tuple, list)) and len(images) == 2 and isinstance(images[0], torch.Tensor) and images[0].dim() == 1:
        buf, meta = images
        meta = np.ascontiguousarray(meta.cpu().numpy() if isinstance(meta, torch.Tensor) else meta, dtype=np.int64)
        if buf.dtype != torch.uint8 or meta.ndim != 2 or meta.shape[1] != 4:
            raise ValueError("encode: the packed form is (uint8 buffer, int64 meta [N][4])")
        return buf.to(device).contiguous(), meta, [(int(h), int(w)) for h, w in meta[:, 1:3]], channels
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() not in (3, 4) or \
            (images.dim() == 4 and images.shape[3] != 3):
        raise ValueError("encode: images must be a uint8 [N, H, W, 3] or [N, H, W] tensor, or the packed (buf, meta)")
    images = images.to(device).contiguous()
    return images, None, [(int(images.shape[1]), int(images.shape[2]))] * images.shape[0], 3 if images.dim() == 4 else 1


@torch.no_grad()
def encode_into(plan, src, meta, dst, slots, channels=3, order="rgb", length=None, status=None, ws=None):
    """msml_jpeg_encode with the caller's buffers, on the current stream.  plan: an EncodePlan; src: uint8 on the
    device; meta: int64 [N][4] on the device = byte offset, H, W, pitch of each source; dst: uint8 on the device; slots:
    int64 [N][2] on the device = byte offset and capacity of each image's slot.  length / status int32 [N] and ws (at
    least plan.ws_bytes) are allocated when None.  -> (length, status).  The device checks every meta row against src
    and every slot against dst: an image that does not fit gets a status and length 0 and writes nothing outside its slot."""
    n = plan.n
    device = dst.device
    for t, shape, name in ((meta, (n, 4), "meta"), (slots, (n, 2), "slots")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or tuple(t.shape) != shape or t.device != device or \
                not t.is_contiguous():
            raise ValueError("encode_into: %s must be a contiguous int64 %s tensor on %s" % (name, list(shape), device))
    if order not in ("rgb", "bgr"):
        raise ValueError("encode_into: order must be 'rgb' or 'bgr'")
    desc, qtabs, headers = plan.to_device(device)
    if length is None:
        length = torch.empty(n, dtype=torch.int32, device=device)
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=device)
    if ws is None:
        ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=device)
    call("msml_jpeg_encode", src, src.numel(), meta, channels, 1 if order == "bgr" else 0, desc, plan.desc.data_ptr(),
         qtabs, qtabs.shape[0], headers, headers.numel(), dst, dst.numel(), slots, length, status, ws, ws.numel(), n)
    return length, status


@torch.no_grad()
def encode_batch(images, quality=75, sampling="420", restart=0, order="rgb", device="cuda", channels=3, slot_bytes=None):
    """Encode N images on the device to baseline JPEG, the bytes PIL.Image.save(quality=, subsampling=,
    restart_marker_blocks=) writes; the defaults are those of a bare save().  -> EncodedBatch.  No synchronisation.

    images: uint8 [N, H, W, 3], or [N, H, W] (one channel; sampling becomes "gray" unless given per image), or the packed
    (buf, meta) of ijb.pack_images / decode_batch with `channels` bytes per pixel.  quality (1..100), sampling ("420",
    "422", "444", "gray") and restart (MCUs per restart interval, 0 = none) are scalars or one value per image.  order
    "bgr": the sources are B, G, R (cv2).  A 3-channel source with sampling "gray" stores libjpeg's Y, which is what
    convert("L") gives.  slot_bytes: the capacity of every slot; the default is msml_jpeg_encode_bound, which no stream
    can exceed and which is 20-40 times what a photograph takes, so a caller that knows its data may pass less (an image
    that does not fit gets status 2)."""
    src, meta, sizes, channels = _source(images, channels, device)
    if channels == 1 and isinstance(sampling, str):
        sampling = "gray"
    plan = _plan(sizes, quality, sampling, restart)
    n = plan.n
    if channels == 1 and (plan.desc.numpy()[:, JE_SAMP] != 0).any():
        raise ValueError("encode: one-channel sources take sampling 'gray' only")
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
    length, status = encode_into(plan, src.reshape(-1), meta_dev, dst, slots_dev, channels, order)
    return EncodedBatch(dst, slots_dev, slots, length, status, plan)


@torch.no_grad()
def recompress(images, quality=75, sampling="420", order="rgb", device="cuda"):
    """Encode, then decode, on the device: the pixels Image.open(path) gives after Image.save(path, quality=,
    subsampling=) -- what eval/qeval_folder.py reads after eval/align_dataset.py:52-75 saved the crops.  images: uint8
    [N, H, W, 3] or [N, H, W]; the same shape comes back, channels in the order they came in.

    Nothing is read back and the host does not wait: the decoder's descriptors are known on the host except for the end
    of each stream, and msml_jpeg_decode's contract allows trailing bytes (it stops at the marker after the last MCU),
    so the end of the slot is passed instead of `length`."""
    if not isinstance(images, torch.Tensor) or images.dim() not in (3, 4):
        raise ValueError("recompress: images must be a uint8 [N, H, W, 3] or [N, H, W] tensor")
    enc = encode_batch(images, quality, sampling, 0, order, device)
    batch = enc.plan.decode_batch_of(enc.buf, enc.slots_host)
    n, h, w = images.shape[:3]
    channels = 3 if images.dim() == 4 else 1
    out = torch.empty(tuple(images.shape), dtype=torch.uint8, device=enc.buf.device)
    decode_into(batch, out, packed.uniform_meta(n, h, w, channels, out.device), channels, order)
    return out


class RecordWriter:
    """The writing twin of RecordFile: MXNet indexed RecordIO (mx.recordio.MXIndexedRecordIO(idx, rec, 'w') + pack)
    without mxnet.  A record is uint32 magic, uint32 length, the payload padded with zeros to 4 bytes; the index holds
    `key\\toffset` lines.  dmlc's writer splits a payload that holds the magic word at a 4-byte-aligned offset into
    continued parts, which RecordFile does not read (and no mxnet was at hand to check a split against): such a payload is
    a ValueError naming the key, and nothing is written for it."""

    def __init__(self, rec_path, idx_path):
        self._f = open(rec_path, "wb")
        self._idx = open(idx_path, "w")
        self.keys = []

    @staticmethod
    def pack(header, payload):
        """header (flag, label, id, id2) as mx.recordio.IRHeader: a number as label gives flag 0; a sequence of labels gives
        flag = their count, label 0 and the float32 labels in front of the payload."""
        flag, label, id1, id2 = header
        if isinstance(label, (int, float, np.integer, np.floating)):
            return struct.pack("<IfQQ", 0, float(label), int(id1), int(id2)) + bytes(payload)
        label = np.asarray(label, dtype="<f4").reshape(-1)
        return struct.pack("<IfQQ", label.size, 0.0, int(id1), int(id2)) + label.tobytes() + bytes(payload)

    def write_idx(self, key, header, payload=None):
        """Write record `key`: pack(header, payload), or `header` itself when payload is None (already packed)."""
        data = bytes(header) if payload is None else self.pack(header, payload)
        if len(data) >= 1 << 29:
            raise ValueError("record %d: %d bytes do not fit one RecordIO record" % (key, len(data)))
        words = np.frombuffer(data[:len(data) & ~3], dtype="<u4")
        if (words == RECORD_MAGIC).any():
            raise ValueError("record %d: the payload holds the RecordIO magic word at a 4-byte-aligned offset; it would be "
                             "written as a continued record, which is unsupported" % key)
        self._idx.write("%d\t%d\n" % (key, self._f.tell()))
        self._f.write(struct.pack("<II", RECORD_MAGIC, len(data)) + data + b"\x00" * (-len(data) % 4))
        self.keys.append(int(key))

    def close(self):
        self._f.close()
        self._idx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def write_faces(writer, encoded, labels, first_key=1, header0=None):
    """What datasets/3d_tools/cvt_casia_webface.py:40-60 does with a batch: record first_key + n holds IRHeader(0,
    labels[n], 0, 0) and the JPEG stream of image n (one synchronising copy, EncodedBatch.to_bytes), or the PNG file when
    `encoded` comes from png.encode_batch (that script's img_fmt='.png', line 35).  header0 = (count,
    classes): also write record 0 as that script's lines 31-37 do, with the labels (count + 1, classes) and id 1, which is
    what load_dataset.py:51-57 (and RecordFile) read the number of samples from; its image (a PNG of zeros there, never
    decoded) is left empty.  -> the next free key."""
    streams = encoded.to_bytes() if isinstance(encoded, EncodedBatch) else list(encoded)
    labels = [int(v) for v in (labels.tolist() if isinstance(labels, (torch.Tensor, np.ndarray)) else labels)]
    if len(labels) != len(streams):
        raise ValueError("write_faces: %d labels for %d images" % (len(labels), len(streams)))
    if header0 is not None:
        writer.write_idx(0, (0, [header0[0] + 1, header0[1]], 1, 0), b"")
    for k, (s, label) in enumerate(zip(streams, labels)):
        writer.write_idx(first_key + k, (0, label, 0, 0), s)
    return first_key + len(streams)
