"""The progressive entropy decode of csrc/jpeg_prog_core.h restated in Python, scan kind by scan kind as jdphuff.c does
it (DC first, DC refinement, AC first, AC refinement), producing coefficients; everything behind the coefficients is
tests/jpeg_cases.py.  Also a scan splitter (a progressive stream as its scans, reassembled in any subset or order) and
a small progressive writer (quantised coefficients + any valid scan script -> a stream, by jcphuff.c), which gives the
cases Pillow never writes: one-component DC scans, spectral selection alone, deeper Al chains, reordered scans, tables
with codes longer than 9 bits.  The restatement counts the events that make the hard paths (EVENTS)."""
import collections
import heapq
import os
import struct

import numpy as np

from msml_amd import jpeg
from tests import hostcheck
from tests import jpeg_cases as J

Z = [int(v) for v in jpeg.ZIGZAG]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_jpeg_prog.npz")
CORRUPT = os.path.join(os.path.dirname(GOLDEN), "g18_jpeg_prog_corrupt.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SRC = os.path.join(ROOT, "tools", "jpeg_prog_hostcheck.cpp")
HOSTCHECK_SEED = 1818
EVENTS = ["eob%d" % n for n in range(15)] + ["zrl_refine", "correction_in_eobrun", "ac_restart", "stuffed_ff", "long_code"]


def load_golden():
    """-> list of dicts {name, data, pixels (uint8 [H,W,3] or [H,W]), base (the baseline stream of the same
    coefficients, b"" where none is recorded)} and the version strings."""
    z = np.load(GOLDEN, allow_pickle=False)
    offs, poffs, boffs = z["stream_offsets"], z["pixel_offsets"], z["base_offsets"]
    out = []
    for i, name in enumerate(z["names"]):
        shape = tuple(int(v) for v in z["shapes"][i] if v > 0)
        out.append({"name": str(name), "data": z["streams"][offs[i]:offs[i + 1]].tobytes(),
                    "pixels": z["pixels"][poffs[i]:poffs[i + 1]].reshape(shape),
                    "base": z["bases"][boffs[i]:boffs[i + 1]].tobytes()})
    return out, {"pillow": str(z["pillow_version"]), "libjpeg_turbo": str(z["libjpeg_turbo_version"])}


# ------------------------------------------------------------------------------------------------ the restatement
def own_blocks(d, c):
    """(blocks per column, blocks per row) of component c's own size: what a one-component scan covers."""
    hm, vm = d.sampling[0]
    h, v = d.sampling[c]
    return -(-(-(-d.height * v // vm)) // 8), -(-(-(-d.width * h // hm)) // 8)


def _symbol(b, table, ev):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | b.bit()
        if (ln, code) in table:
            if ln > 9:
                ev["long_code"] += 1
            return table[(ln, code)]
    raise J.Corrupt(1)


def entropy_decode(data, d, events=None):
    """data, parse_jpeg(data, progressive=True) -> per component an int array [blocks_y, blocks_x, 64] (the
    MCU-padded planes, natural order).  events: a Counter of EVENTS."""
    ev = events if events is not None else collections.Counter()
    hm, vm = d.sampling[0]
    mcux, mcuy = -(-d.width // (8 * hm)), -(-d.height // (8 * vm))
    coefs = [np.zeros((mcuy * v, mcux * h, 64), np.int64) for h, v in d.sampling]
    for sc in d.scans:
        b = J._Bits(data, sc.begin, sc.end)
        if b"\xff\x00" in data[sc.begin:sc.end]:
            ev["stuffed_ff"] += 1
        tabs = [J._codes(*t) if t is not None else None for t in sc.tables]
        ri, p1 = sc.restart_interval, 1 << sc.al
        state = {"left": ri, "rst": 0}

        def restart_due():
            if not ri:
                return False
            due = state["left"] == 0
            if due:
                b.restart(state["rst"])
                state["rst"] += 1
                state["left"] = ri
            state["left"] -= 1
            return due

        if sc.ss == 0:
            inter = len(sc.components) > 1
            rows, cols = (mcuy, mcux) if inter else own_blocks(d, sc.components[0])
            pred = [0] * len(sc.components)
            for my in range(rows):
                for mx in range(cols):
                    if restart_due():
                        pred = [0] * len(sc.components)
                    for i, c in enumerate(sc.components):
                        h, v = d.sampling[c] if inter else (1, 1)
                        for yy in range(v):
                            for xx in range(h):
                                blk = coefs[c][my * v + yy, mx * h + xx]
                                if sc.ah == 0:
                                    s = _symbol(b, tabs[i], ev)
                                    if s > 11:
                                        raise J.Corrupt(3)
                                    if s:
                                        pred[i] += J.extend(b.receive(s), s)
                                    blk[0] = pred[i] << sc.al
                                elif b.bit():
                                    blk[0] |= p1
                    if b.fake:
                        raise J.Corrupt(5)
            continue
        c = sc.components[0]
        rows, cols = own_blocks(d, c)
        eobrun, tab = 0, tabs[0]
        for by in range(rows):
            for bx in range(cols):
                if restart_due():
                    eobrun = 0
                    ev["ac_restart"] += 1
                blk = coefs[c][by, bx]
                if sc.ah == 0:
                    if eobrun > 0:
                        eobrun -= 1
                        continue
                    k = sc.ss
                    while k <= sc.se:
                        rs = _symbol(b, tab, ev)
                        r, s = rs >> 4, rs & 15
                        if s:
                            if s > 10:
                                raise J.Corrupt(3)
                            k += r
                            if k > sc.se:
                                raise J.Corrupt(2)
                            blk[Z[k]] = J.extend(b.receive(s), s) << sc.al
                            k += 1
                        elif r == 15:
                            k += 16
                            if k > sc.se + 1:
                                raise J.Corrupt(2)
                        else:
                            eobrun = (1 << r) - 1 + (b.receive(r) if r else 0)
                            ev["eob%d" % r] += 1
                            break
                else:
                    k = sc.ss
                    if eobrun == 0:
                        while k <= sc.se:
                            rs = _symbol(b, tab, ev)
                            r, s = rs >> 4, rs & 15
                            if s:
                                if s != 1:
                                    raise J.Corrupt(3)
                                s = p1 if b.bit() else -p1
                            elif r != 15:
                                eobrun = (1 << r) + (b.receive(r) if r else 0)
                                ev["eob%d" % r] += 1
                                break
                            else:
                                ev["zrl_refine"] += 1
                            while k <= sc.se:
                                z = Z[k]
                                if blk[z] != 0:
                                    if b.bit() and (int(blk[z]) & p1) == 0:
                                        blk[z] += p1 if blk[z] >= 0 else -p1
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            if s:
                                if k > sc.se:
                                    raise J.Corrupt(2)
                                blk[Z[k]] = s
                            k += 1
                    if eobrun > 0:
                        while k <= sc.se:
                            z = Z[k]
                            if blk[z] != 0:
                                ev["correction_in_eobrun"] += 1
                                if b.bit() and (int(blk[z]) & p1) == 0:
                                    blk[z] += p1 if blk[z] >= 0 else -p1
                            k += 1
                        eobrun -= 1
                if b.fake:
                    raise J.Corrupt(5)
    return coefs


def pixels_of(coefs, d):
    """The coefficients of entropy_decode (or J.entropy_decode) -> uint8 [H, W, 3], or [H, W] for a gray stream."""
    planes = [J.idct_blocks(coefs[c], d.qtables[d.qsel[c]]) for c in range(d.components)]
    h, w = d.height, d.width
    if d.components == 1:
        return planes[0][:h, :w]
    hm, vm = d.sampling[0]
    dw, dh = -(-w // hm), -(-h // vm)
    chroma = []
    for p in planes[1:]:
        p = p[:dh, :dw]
        if (hm, vm) == (2, 1):
            p = J.upsample_h2v1(p)
        elif (hm, vm) == (2, 2):
            p = J.upsample_h2v2(p)
        chroma.append(p[:h, :w])
    return J.ycc_to_rgb(planes[0][:h, :w], chroma[0], chroma[1])


def decode(data, events=None):
    """Progressive (or baseline) JPEG bytes -> pixels.  Raises J.Corrupt(status) / ValueError (refused)."""
    d = jpeg.parse_jpeg(data, progressive=True)
    if d.status:
        raise ValueError(d.reason)
    if not d.scans:
        return J.decode(data)
    return pixels_of(entropy_decode(data, d, events), d)


def coefficients(data):
    """The quantised coefficients of a supported stream of either kind -> (coefs, descriptor)."""
    d = jpeg.parse_jpeg(data, progressive=True)
    if d.status:
        raise ValueError(d.reason)
    return (entropy_decode(data, d) if d.scans else J.entropy_decode(data, d)), d


# ------------------------------------------------------------------------------------------------ the scan splitter
def _dri(ri):
    return b"\xff\xdd\x00\x04" + struct.pack(">H", ri)


def split_scans(data):
    """A progressive stream -> (head, [scan chunks]): head runs through the frame header; a chunk is the scan's table
    segments, its SOS and its entropy-coded bytes, with the restart interval it was written under stated in front, so
    that join_scans(head, any subset in any order) is a stream whose scans still decode as they were written."""
    d = jpeg.parse_jpeg(data, progressive=True)
    if not d.scans:
        raise ValueError("split_scans: not a progressive stream the parser walks (status %d)" % d.status)
    sof = data.index(b"\xff\xc2")
    at = sof + 2 + ((data[sof + 2] << 8) | data[sof + 3])
    head, chunks = data[:at], []
    any_ri = any(s.restart_interval for s in d.scans)
    for s in d.scans:
        chunks.append((_dri(s.restart_interval) if any_ri else b"") + data[at:s.end])
        at = s.end
    return head, chunks


def join_scans(head, chunks):
    return head + b"".join(chunks) + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------ the writer
PILLOW_SCRIPT_3 = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1),
                   ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0),
                   ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def _nbits(v):
    return int(v).bit_length()


def huffman_from_counts(freq, skew=False):
    """Annex K.2 (jpeg_gen_optimal_table): {symbol: count} -> (counts [16], symbols) of a prefix code of at most 16
    bits that leaves the all-ones code unused.  skew: the counts are replaced by Fibonacci numbers in their order,
    which makes the longest codes a table of that many symbols can have."""
    syms = sorted(freq, key=lambda s: (-freq[s], s))
    if skew:
        fib = [1, 2]
        while len(fib) < len(syms):
            fib.append(fib[-1] + fib[-2])
        freq = {s: fib[len(syms) - 1 - i] for i, s in enumerate(syms)}
    heap = [(f, s, (s,)) for s, f in freq.items()] + [(0.5, 256, (256,))]     # 256: the reserved code point
    size = collections.Counter()
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            size[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    bits = [0] * 300
    for s, n in size.items():
        bits[n] += 1
    for i in range(299, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                              # the reserved code point goes
    order = sorted((s for s in size if s != 256), key=lambda s: (size[s], s))
    return bits[1:17], bytes(order)


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _extra(v, n):
    return (v if v >= 0 else v - 1) & ((1 << n) - 1)


class _Tokens:
    """One scan as tokens: ("s", table slot, symbol), ("b", value, count), ("r", index)."""

    def __init__(self):
        self.t, self.eobrun, self.be = [], 0, []

    def sym(self, slot, s):
        self.t.append(("s", slot, s))

    def bits(self, v, n):
        if n:
            self.t.append(("b", v, n))

    def flush_eobrun(self):
        if self.eobrun:
            n = _nbits(self.eobrun) - 1
            self.sym(0, n << 4)
            self.bits(self.eobrun & ((1 << n) - 1), n)
            self.eobrun = 0
        for v in self.be:
            self.bits(v, 1)
        self.be = []


def _scan_tokens(coefs, d, script_row, ri):
    comps, ss, se, ah, al = script_row
    tk = _Tokens()
    hm, vm = d.sampling[0]
    mcux, mcuy = -(-d.width // (8 * hm)), -(-d.height // (8 * vm))
    left, rst = ri, 0
    if ss == 0:
        inter = len(comps) > 1
        rows, cols = (mcuy, mcux) if inter else own_blocks(d, comps[0])
        pred = [0] * len(comps)
        for my in range(rows):
            for mx in range(cols):
                if ri:
                    if left == 0:
                        tk.t.append(("r", rst))
                        rst += 1
                        pred = [0] * len(comps)
                        left = ri
                    left -= 1
                for i, c in enumerate(comps):
                    h, v = d.sampling[c] if inter else (1, 1)
                    for yy in range(v):
                        for xx in range(h):
                            dc = int(coefs[c][my * v + yy, mx * h + xx, 0])
                            if ah:
                                tk.bits((dc >> al) & 1, 1)
                                continue
                            diff = (dc >> al) - pred[i]
                            pred[i] = dc >> al
                            n = _nbits(abs(diff))
                            tk.sym(i, n)
                            tk.bits(_extra(diff, n), n)
        return tk.t
    c = comps[0]
    rows, cols = own_blocks(d, c)
    for by in range(rows):
        for bx in range(cols):
            if ri:
                if left == 0:
                    tk.flush_eobrun()
                    tk.t.append(("r", rst))
                    rst += 1
                    left = ri
                left -= 1
            blk = coefs[c][by, bx]
            mag = [abs(int(blk[Z[k]])) >> al for k in range(64)]
            r = 0
            if ah == 0:
                for k in range(ss, se + 1):
                    if mag[k] == 0:
                        r += 1
                        continue
                    tk.flush_eobrun()
                    while r > 15:
                        tk.sym(0, 0xF0)
                        r -= 16
                    n = _nbits(mag[k])
                    tk.sym(0, (r << 4) | n)
                    tk.bits(_extra(mag[k] if blk[Z[k]] > 0 else -mag[k], n), n)
                    r = 0
                if r > 0:
                    tk.eobrun += 1
                    if tk.eobrun == 0x7FFF:
                        tk.flush_eobrun()
                continue
            eob = max([k for k in range(ss, se + 1) if mag[k] == 1], default=0)
            br = []
            for k in range(ss, se + 1):
                if mag[k] == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    tk.flush_eobrun()
                    tk.sym(0, 0xF0)
                    r -= 16
                    for v in br:
                        tk.bits(v, 1)
                    br = []
                if mag[k] > 1:
                    br.append(mag[k] & 1)
                    continue
                tk.flush_eobrun()
                tk.sym(0, (r << 4) | 1)
                tk.bits(0 if blk[Z[k]] < 0 else 1, 1)
                for v in br:
                    tk.bits(v, 1)
                br, r = [], 0
            if r > 0 or br:
                tk.eobrun += 1
                tk.be += br
                if tk.eobrun == 0x7FFF or len(tk.be) > 937:
                    tk.flush_eobrun()
    tk.flush_eobrun()
    return tk.t


def _emit(tokens, tables):
    codes = []
    for counts, symbols in tables:
        codes.append({s: (code, ln) for (ln, code), s in J._codes(counts, symbols).items()})
    w = _BitWriter()
    for t in tokens:
        if t[0] == "s":
            code, ln = codes[t[1]][t[2]]
            w.put(code, ln)
        elif t[0] == "b":
            w.put(t[1], t[2])
        else:
            w.flush()
            w.out += bytes((0xFF, 0xD0 + (t[1] & 7)))
    w.flush()
    return bytes(w.out)


def _tables_for(tokens, nslots, skew):
    tabs = []
    for slot in range(nslots):
        freq = collections.Counter(t[2] for t in tokens if t[0] == "s" and t[1] == slot)
        if not freq:
            freq[0] = 1
        tabs.append(huffman_from_counts(freq, skew))
    return tabs


def _frame(d, marker):
    out = b"\xff\xd8" + jpeg._segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in sorted(set(d.qsel)):
        out += jpeg._segment(0xDB, bytes((t,)) + bytes(int(v) for v in d.qtables[t][jpeg.ZIGZAG]))
    comps = b"".join(bytes((c + 1, (h << 4) | v, d.qsel[c])) for c, (h, v) in enumerate(d.sampling))
    return out + jpeg._segment(marker, struct.pack(">BHHB", 8, d.height, d.width, d.components) + comps)


def write_progressive(coefs, d, script, restart=0, skew=False):
    """coefs / d: as coefficients() gives them (d supplies size, sampling and quantisation tables); script: rows of
    (components, Ss, Se, Ah, Al); restart: one interval for every scan, or one per scan (MCUs, blocks for a
    one-component scan).  Every scan brings its own optimal tables under ids 0.. (skew: with the longest codes)."""
    out, last_ri = _frame(d, 0xC2), 0
    for i, row in enumerate(script):
        comps, ss, se, ah, al = row
        ri = restart[i] if isinstance(restart, (list, tuple)) else restart
        tokens = _scan_tokens(coefs, d, row, ri)
        dc = ss == 0
        tabs = [] if (dc and ah) else _tables_for(tokens, len(comps) if dc else 1, skew)
        for slot, (counts, symbols) in enumerate(tabs):
            out += jpeg._segment(0xC4, bytes(((0 if dc else 0x10) | slot,)) + bytes(counts) + symbols)
        if ri != last_ri:
            out += _dri(ri)
            last_ri = ri
        sel = b"".join(bytes((c + 1, (k << 4) if dc else 0)) for k, c in enumerate(comps))
        out += jpeg._segment(0xDA, bytes((len(comps),)) + sel + bytes((ss, se, (ah << 4) | al)))
        out += _emit(tokens, tabs)
    return out + b"\xff\xd9"


def write_baseline(coefs, d, restart=0):
    """The same coefficients as one baseline scan with optimal tables (one DC and one AC table per component)."""
    tk = _Tokens()
    hm, vm = d.sampling[0]
    mcux, mcuy = -(-d.width // (8 * hm)), -(-d.height // (8 * vm))
    pred, left, rst = [0] * d.components, restart, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if restart:
                if left == 0:
                    tk.t.append(("r", rst))
                    rst += 1
                    pred = [0] * d.components
                    left = restart
                left -= 1
            for c, (h, v) in enumerate(d.sampling):
                for yy in range(v):
                    for xx in range(h):
                        blk = coefs[c][my * v + yy, mx * h + xx]
                        diff = int(blk[0]) - pred[c]
                        pred[c] = int(blk[0])
                        n = _nbits(abs(diff))
                        tk.sym(2 * c, n)
                        tk.bits(_extra(diff, n), n)
                        r = 0
                        for k in range(1, 64):
                            v_ = int(blk[Z[k]])
                            if v_ == 0:
                                r += 1
                                continue
                            while r > 15:
                                tk.sym(2 * c + 1, 0xF0)
                                r -= 16
                            n = _nbits(abs(v_))
                            tk.sym(2 * c + 1, (r << 4) | n)
                            tk.bits(_extra(v_, n), n)
                            r = 0
                        if r:
                            tk.sym(2 * c + 1, 0)
    tabs = _tables_for(tk.t, 2 * d.components, False)
    out = _frame(d, 0xC0)
    for slot, (counts, symbols) in enumerate(tabs):
        out += jpeg._segment(0xC4, bytes((((slot & 1) << 4) | (slot >> 1),)) + bytes(counts) + symbols)
    if restart:
        out += _dri(restart)
    sel = b"".join(bytes((c + 1, (c << 4) | c)) for c in range(d.components))
    out += jpeg._segment(0xDA, bytes((d.components,)) + sel + b"\x00\x3f\x00")
    return out + _emit(tk.t, tabs) + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------ the host check
def build_hostcheck(out, sanitize=True):
    """Compile tools/jpeg_prog_hostcheck.cpp with the host compiler (and the sanitizers) -> out."""
    return hostcheck.build_hostcheck(HOSTCHECK_SRC, out, sanitize)


def write_hostcheck_input(path, cases):
    """The input file of tools/jpeg_prog_hostcheck.cpp: header, descriptors, scan table, tables, streams and the
    expected RGB pixels of every supported stream."""
    batch = jpeg.pack_jpegs([c["data"] for c in cases], progressive=True)
    head = np.array([0x4A504831, len(cases), batch.qtabs.shape[0], batch.htabs.shape[0], batch.streams.numel(),
                     batch.scans.shape[0], HOSTCHECK_SEED, 0], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(batch.desc.numpy().tobytes())
        f.write(batch.scans.numpy().tobytes())
        f.write(batch.qtabs.numpy().tobytes())
        f.write(batch.htabs.numpy().tobytes())
        f.write(batch.streams.numpy().tobytes())
        for c, d in zip(cases, batch.descriptors):
            if d.status == 0:
                f.write(np.ascontiguousarray(J.as_rgb(c["pixels"])).tobytes())
    return batch


def run_hostcheck(exe, input_path):
    """-> (returncode, stderr, clean [(image, status, match)], mutations [(kind, image, a, b, status)],
    dumped [(kind, image, a, b, status, stream bytes, scan records as bytes)])."""
    import subprocess
    r = subprocess.run([exe, input_path], capture_output=True, text=True)
    clean, muts, dumped = [], [], []
    for line in r.stdout.splitlines():
        t = line.split(" ")
        if t[0] == "C":
            clean.append((int(t[1]), int(t[2]), int(t[3])))
        elif t[0] == "M":
            muts.append((t[1], int(t[2]), int(t[3]), int(t[4]), int(t[5])))
        elif t[0] == "D":
            rec = np.array([int(t[7][i:i + 8], 16) for i in range(0, len(t[7]), 8)], np.uint32).astype(np.int32)
            dumped.append((t[1], int(t[2]), int(t[3]), int(t[4]), int(t[5]), bytes.fromhex(t[6]), rec.tobytes()))
    return r.returncode, r.stderr, clean, muts, dumped


def load_corrupt():
    """The mutations tools/make_golden_jpeg_prog.py recorded from the host check, with the statuses it printed: list
    of (kind, image, a, b, status, stream bytes, scan records as bytes)."""
    z = np.load(CORRUPT, allow_pickle=False)
    offs, roffs = z["offsets"], z["record_offsets"]
    return [(str(k), int(r[0]), int(r[1]), int(r[2]), int(r[3]), z["streams"][offs[i]:offs[i + 1]].tobytes(),
             z["records"][roffs[i]:roffs[i + 1]].tobytes()) for i, (k, r) in enumerate(zip(z["kinds"], z["rows"]))]


def save_corrupt(dumped):
    offs = np.cumsum([0] + [len(d[5]) for d in dumped]).astype(np.int64)
    roffs = np.cumsum([0] + [len(d[6]) // 4 for d in dumped]).astype(np.int64)
    np.savez_compressed(CORRUPT, kinds=np.array([d[0] for d in dumped]),
                        rows=np.array([d[1:5] for d in dumped], np.int64), offsets=offs, record_offsets=roffs,
                        streams=np.frombuffer(b"".join(d[5] for d in dumped), np.uint8),
                        records=np.frombuffer(b"".join(d[6] for d in dumped), np.int32))


def corrupt_batch(clean, patches):
    """A packed batch of the clean streams in which, for every (image, stream, records) of `patches`, that image is a
    mutation the host check decoded: its bytes (no longer than the clean stream's) and its scan records (no more than
    the clean stream's) put in place of the parsed ones, exactly what the host check handed its decoder."""
    batch = jpeg.pack_jpegs(clean, progressive=True)
    dn, sn, flat = batch.desc.numpy(), batch.scans.numpy(), batch.streams.numpy()
    for victim, stream, records in patches:
        rec = np.frombuffer(records, np.int32).reshape(-1, jpeg.SCAN_WORDS)
        off, s0 = int(dn[victim, jpeg.JD_BASE]) * 4, int(dn[victim, jpeg.JD_SCAN0])
        assert len(stream) <= dn[victim, jpeg.JD_END] and 0 < len(rec) <= dn[victim, jpeg.JD_NSCAN]
        flat[off:off + int(dn[victim, jpeg.JD_END])] = 0
        flat[off:off + len(stream)] = np.frombuffer(stream, np.uint8)
        sn[s0:s0 + len(rec)] = rec
        dn[victim, jpeg.JD_END], dn[victim, jpeg.JD_NSCAN] = len(stream), len(rec)
        dn[victim, jpeg.JD_BEGIN] = min(int(dn[victim, jpeg.JD_BEGIN]), len(stream))
    return batch
