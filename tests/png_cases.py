"""The PNG decoder of csrc/png_core.h restated with numpy and zlib (decode_png: inflate by zlib, the filters and the
sample expansion in numpy, Pillow's convert rules), the PNG *writer* the fixtures need (chosen row filters, IDAT split
points and zlib.compressobj arguments), a token-level DEFLATE writer (chosen (length, distance) tokens and chosen
dynamic-block headers: what zlib's own encoder never emits), and an inflate in plain Python that reports what a stream
exercises.  tests/test_png_cpu.py pins the restatement to the arrays Pillow gave (tests/golden/g17_png.npz) and to
the installed Pillow; the GPU and host-check tests compare with the fixture."""
import os
import struct
import zlib

import numpy as np

from msml_amd import png
from tests import hostcheck
from tests.hostcheck import host_compiler, sanitizers_link  # noqa: F401 (the tests reach them through this module)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g17_png.npz")
CORRUPT = os.path.join(HERE, "golden", "g17_png_corrupt.npz")
HOSTCHECK_SRC = os.path.join(os.path.dirname(HERE), "tools", "png_hostcheck.cpp")
HOSTCHECK_SEED = 20260117
MODES = {1: "L", 3: "RGB", 4: "RGBA"}


# ------------------------------------------------------------------------------------------------ the PNG writer
def chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(rows, filters, bpp):
    """rows uint8 [H][rowbytes] (packed samples) -> the filtered bytes, row y with filter filters[y % len]."""
    rows = np.asarray(rows, np.uint8)
    h, rb = rows.shape
    out = bytearray()
    prior = np.zeros(rb, np.int32)
    for y in range(h):
        ft = filters[y % len(filters)]
        cur = rows[y].astype(np.int32)
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        if rb <= bpp:
            left = np.zeros(rb, np.int32)
        ul = np.concatenate([np.zeros(bpp, np.int32), prior[:-bpp]]) if rb > bpp else np.zeros(rb, np.int32)
        if ft == 0:
            pred = np.zeros(rb, np.int32)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prior
        elif ft == 3:
            pred = (left + prior) >> 1
        else:
            pred = np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, prior, ul)], np.int32)
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prior = cur
    return bytes(out)


def pack_samples(samples, depth):
    """samples uint8 [H][W * spp] -> packed rows uint8 [H][ceil(W * spp * depth / 8)] (MSB first)."""
    samples = np.asarray(samples, np.uint8)
    if depth == 8:
        return samples
    h, n = samples.shape
    per = 8 // depth
    pad = (-n) % per
    s = np.concatenate([samples, np.zeros((h, pad), np.uint8)], axis=1).reshape(h, -1, per).astype(np.int32)
    shifts = np.array([8 - depth * (k + 1) for k in range(per)], np.int32)
    return (s << shifts).sum(axis=2).astype(np.uint8)


def split_idat(z, splits):
    """splits: None (one IDAT), an int (pieces of that size) or a list of cut offsets."""
    if splits is None:
        return [z]
    if isinstance(splits, int):
        return [z[i:i + splits] for i in range(0, len(z), splits)]
    cuts = [0] + list(splits) + [len(z)]
    return [z[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def write_png(width, height, depth, colour_type, samples=None, filters=(0,), plte=None, trns=None, splits=None,
              zargs=None, zstream=None, filtered=None, extra=(), interlace=0):
    """-> the bytes of a PNG file.  samples [H][W * spp]; filters: the row filters, cycled; zargs: dict of
    zlib.compressobj arguments (level, strategy ...); zstream: a ready zlib stream instead (the token-level writer's);
    filtered: ready filtered bytes instead of samples; extra: [(type, body)] chunks in front of IDAT."""
    spp = png.CHANNELS_OF[colour_type]
    bpp = max(1, spp * depth // 8)
    if zstream is None:
        if filtered is None:
            filtered = filter_rows(pack_samples(samples, depth), filters, bpp)
        c = zlib.compressobj(**(zargs or {}))
        zstream = c.compress(filtered) + c.flush()
    out = png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour_type, 0, 0, interlace))
    if plte is not None:
        out += chunk(b"PLTE", bytes(plte))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    for t, body in extra:
        out += chunk(t, body)
    for piece in split_idat(zstream, splits):
        out += chunk(b"IDAT", piece)
    return out + chunk(b"IEND", b"")


# ------------------------------------------------------------------------------------- the token-level DEFLATE writer
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def flat_lengths(used, n):
    """A complete code over the symbols `used` (at least 2): lengths [n], as equal as the Kraft sum allows."""
    used = sorted(used)
    k = len(used)
    assert k >= 2
    top = (k - 1).bit_length()
    short = (1 << top) - k
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = top - 1 if i < short else top
    return lens


def length_symbol(length):
    for s in range(28, -1, -1):
        if length >= LBASE[s]:
            if s == 28 and length != 258:
                continue
            return s
    raise ValueError(length)


def distance_symbol(dist):
    for s in range(29, -1, -1):
        if dist >= DBASE[s]:
            return s
    raise ValueError(dist)


class Deflate:
    """An LSB-first bit writer with the three block kinds.  Tokens: an int is a literal, (length, distance) a match."""

    def __init__(self, cmf=0x78, flg=0x01):
        self.out = bytearray([cmf, flg])
        self.acc = self.n = 0

    def bits(self, v, k):
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        v, k = c
        for i in range(k - 1, -1, -1):
            self.bits((v >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def stored(self, data, final=False):
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.align()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xffff) + bytes(data)

    def tokens(self, toks, lit, dist):
        for t in toks:
            if isinstance(t, tuple):
                ln, d = t
                s = length_symbol(ln)
                self.code(lit[257 + s])
                self.bits(ln - LBASE[s], LEXT[s])
                s = distance_symbol(d)
                self.code(dist[s])
                self.bits(d - DBASE[s], DEXT[s])
            else:
                self.code(lit[t])
        self.code(lit[256])

    def fixed(self, toks, final=False):
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        self.tokens(toks, canonical(FIXED_LIT), canonical(FIXED_DIST))

    def dynamic(self, toks, lit_lens, dist_lens, final=False, cl_syms=None):
        """lit_lens [257..286], dist_lens [1..30]: the code lengths.  The header run-length codes the two lists as ONE
        sequence (so a repeat may run from the one into the other); cl_syms overrides that coding with explicit
        (symbol, extra) pairs."""
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        seq = list(lit_lens) + list(dist_lens)
        if cl_syms is None:
            cl_syms, i = [], 0
            while i < len(seq):
                v, run = seq[i], 1
                while i + run < len(seq) and seq[i + run] == v:
                    run += 1
                if v == 0 and run >= 3:
                    r = min(run, 138)
                    cl_syms.append((17, r - 3) if r <= 10 else (18, r - 11))
                    i += r
                elif v != 0 and run >= 4:
                    r = min(run - 1, 6)
                    cl_syms += [(v, None), (16, r - 3)]
                    i += 1 + r
                else:
                    cl_syms.append((v, None))
                    i += 1
        used = sorted({s for s, _ in cl_syms})
        if len(used) < 2:
            used = sorted(set(used) | {0, 18})[:2] if used != [0] else [0, 18]
        cl_lens = flat_lengths(used, 19)
        hclen = max(i for i, s in enumerate(CLORDER) if cl_lens[s]) + 1
        hclen = max(hclen, 4)
        self.bits(len(lit_lens) - 257, 5)
        self.bits(len(dist_lens) - 1, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CLORDER[i]], 3)
        cl = canonical(cl_lens)
        for s, ex in cl_syms:
            self.code(cl[s])
            if s == 16:
                self.bits(ex, 2)
            elif s == 17:
                self.bits(ex, 3)
            elif s == 18:
                self.bits(ex, 7)
        self.tokens(toks, canonical(lit_lens), canonical(dist_lens))

    def finish(self, data=None, adler=None):
        """The Adler-32 trailer of `data` (the bytes the tokens stand for)."""
        self.align()
        self.out += struct.pack(">I", zlib.adler32(data) if adler is None else adler)
        return bytes(self.out)


def expand_tokens(toks, start=b""):
    out = bytearray(start)
    for t in toks:
        if isinstance(t, tuple):
            ln, d = t
            for _ in range(ln):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out[len(start):])


# ------------------------------------------------------------------------------------------- inflate in plain Python
class Corrupt(Exception):
    def __init__(self, status):
        super().__init__(png.STATUS[status])
        self.status = status


def trace_inflate(z):
    """RFC 1951 walked bit by bit -> (bytes, facts): facts records what the stream exercises (block kinds, the longest
    code, match extremes, header repeats that cross from the literal/length into the distance lengths ...)."""
    pos = [16]

    def bit():
        p = pos[0]
        if p >> 3 >= len(z):
            raise Corrupt(7)
        pos[0] = p + 1
        return (z[p >> 3] >> (p & 7)) & 1

    def bits(k):
        return sum(bit() << i for i in range(k))

    def decoder(lens):
        table = {(l, c): s for s, (c, l) in canonical(lens).items()}

        def sym():
            c = 0
            for l in range(1, 16):
                c = (c << 1) | bit()
                if (l, c) in table:
                    return table[(l, c)]
            raise Corrupt(5)
        return sym

    facts = {"blocks": [], "max_code": 0, "max_dist": 0, "d1_l258": False, "repeat_spans": False,
             "one_bit_dist": False, "empty_stored": False, "final_empty_fixed": False, "matches": []}
    out = bytearray()
    if len(z) < 2 or ((z[0] << 8) | z[1]) % 31 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or z[1] & 32:
        raise Corrupt(1)
    while True:
        final, typ = bit(), bits(2)
        facts["blocks"].append(typ)
        before = len(out)
        if typ == 0:
            pos[0] = (pos[0] + 7) & ~7
            ln, nl = bits(16), bits(16)
            if ln ^ 0xffff != nl:
                raise Corrupt(3)
            p = pos[0] >> 3
            if p + ln > len(z):
                raise Corrupt(7)
            out += z[p:p + ln]
            pos[0] += 8 * ln
            if ln == 0:
                facts["empty_stored"] = True
        elif typ == 3:
            raise Corrupt(2)
        else:
            if typ == 1:
                ll, dl = FIXED_LIT, FIXED_DIST
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CLORDER[i]] = bits(3)
                sym = decoder(cl)
                seq = []
                while len(seq) < hlit + hdist:
                    s = sym()
                    at = len(seq)
                    if s < 16:
                        seq.append(s)
                    else:
                        if s == 16 and not seq:
                            raise Corrupt(4)
                        v, r = (seq[-1], 3 + bits(2)) if s == 16 else ((0, 3 + bits(3)) if s == 17 else (0, 11 + bits(7)))
                        seq += [v] * r
                        if at < hlit < len(seq):
                            facts["repeat_spans"] = True
                    if len(seq) > hlit + hdist:
                        raise Corrupt(4)
                ll, dl = seq[:hlit], seq[hlit:]
                facts["max_code"] = max(facts["max_code"], max(ll), max(dl))
                if sum(1 for v in dl if v) == 1 and max(dl) == 1:
                    facts["one_bit_dist"] = True
            lsym, dsym = decoder(ll), decoder(dl)
            while True:
                s = lsym()
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise Corrupt(5)
                    ln = LBASE[s - 257] + bits(LEXT[s - 257])
                    s = dsym()
                    if s > 29:
                        raise Corrupt(5)
                    d = DBASE[s] + bits(DEXT[s])
                    if d > len(out):
                        raise Corrupt(6)
                    facts["max_dist"] = max(facts["max_dist"], d)
                    facts["d1_l258"] |= d == 1 and ln == 258
                    facts["matches"].append((len(out), ln, d))
                    for _ in range(ln):
                        out.append(out[-d])
            if typ == 1 and final and len(out) == before:
                facts["final_empty_fixed"] = True
        if final:
            break
    pos[0] = (pos[0] + 7) & ~7
    if bits(32) != struct.unpack("<I", struct.pack(">I", zlib.adler32(bytes(out))))[0]:
        raise Corrupt(9)
    return bytes(out), facts


def zlib_accepts(z, expected):
    """The acceptance rule of msml_amd/png.py, evaluated with the installed zlib."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(z)
    except zlib.error:
        return False
    return d.eof and len(out) == expected


# ----------------------------------------------------------------------------------------------- the restatement
def unfilter(raw, h, rb, bpp):
    """raw: h rows of 1 + rb bytes -> uint8 [h][rb]; Corrupt(10) for a filter byte above 4."""
    rows = np.zeros((h, rb), np.uint8)
    prior = [0] * rb
    for y in range(h):
        ft = raw[y * (rb + 1)]
        if ft > 4:
            raise Corrupt(10)
        line = list(raw[y * (rb + 1) + 1:(y + 1) * (rb + 1)])
        for i in range(rb):
            a = line[i - bpp] if i >= bpp else 0
            b = prior[i]
            c = prior[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]
            line[i] = (line[i] + pred) & 255
        rows[y] = line
        prior = line
    return rows


def decode_png(data, channels=3):
    """-> uint8 [H][W] / [H][W][3] / [H][W][4]: Pillow's Image.open(data).convert("L" / "RGB" / "RGBA").  Corrupt with
    the status for a stream the parser or the acceptance rule refuses."""
    d = png.parse_png(data)
    if d.status:
        raise Corrupt(d.status)
    z = d.zlib_stream()
    if not zlib_accepts(z, d.expected):
        raise Corrupt(7)
    rows = unfilter(zlib.decompressobj().decompress(z), d.height, d.row_bytes, max(1, d.bits_per_pixel // 8))
    h, w, dp, ct = d.height, d.width, d.depth, d.colour_type
    spp = png.CHANNELS_OF[ct]
    if dp == 8:
        s = rows.reshape(h, w, spp).astype(np.int32)
    else:
        per = 8 // dp
        shifts = np.array([8 - dp * (k + 1) for k in range(per)], np.int32)
        s = ((rows.astype(np.int32)[:, :, None] >> shifts) & ((1 << dp) - 1)).reshape(h, -1)[:, :w * spp].reshape(h, w, spp)
    rgba = np.empty((h, w, 4), np.int32)
    rgba[..., 3] = 255
    key = d.key()
    if ct == 3:
        rgba = d.palette().astype(np.int32)[s[..., 0]]
    elif ct == 0:
        rgba[..., :3] = s * (255 // ((1 << dp) - 1))
        if key is not None:
            rgba[..., 3] = np.where(s[..., 0] == key[0], 0, 255)
    elif ct == 4:
        rgba[..., :3] = s[..., :1]
        rgba[..., 3] = s[..., 1]
    elif ct == 2:
        rgba[..., :3] = s
        if key is not None:
            rgba[..., 3] = np.where((s == np.array(key)).all(axis=2), 0, 255)
    else:
        rgba = s
    rgba = rgba.astype(np.uint8)
    if channels == 4:
        return rgba
    if channels == 3:
        return np.ascontiguousarray(rgba[..., :3])
    if ct not in (0, 4):
        raise ValueError("channels=1 takes gray streams")
    return np.ascontiguousarray(rgba[..., 0])


# ---------------------------------------------------------------------------------------------------- the fixture
def load_golden():
    """-> list of dicts {name, data (bytes), supported, status (the parser's), L / RGB / RGBA (uint8 arrays as Pillow
    gave them; L only for gray streams; none for an unsupported stream)} and the version strings."""
    z = np.load(GOLDEN, allow_pickle=False)
    offs, poffs = z["stream_offsets"], z["pixel_offsets"]
    out = []
    for i, name in enumerate(str(s) for s in z["names"]):
        c = {"name": name, "data": z["streams"][offs[i]:offs[i + 1]].tobytes(), "supported": bool(z["supported"][i]),
             "status": int(z["status"][i])}
        h, w = int(z["shapes"][i][0]), int(z["shapes"][i][1])
        for k, (mode, ch) in enumerate((("L", 1), ("RGB", 3), ("RGBA", 4))):
            a, b = int(poffs[i][k]), int(poffs[i][k + 1])
            if b > a:
                c[mode] = z["pixels"][a:b].reshape((h, w) if ch == 1 else (h, w, ch))
        out.append(c)
    return out, {"pillow": str(z["pillow_version"]), "zlib": str(z["zlib_version"])}


def save_golden(cases, versions):
    streams = b"".join(c["data"] for c in cases)
    offs = np.cumsum([0] + [len(c["data"]) for c in cases]).astype(np.int64)
    px, poffs, shapes, p = [], [], [], 0
    for c in cases:
        row = [p]
        for mode in ("L", "RGB", "RGBA"):
            if mode in c:
                px.append(np.ascontiguousarray(c[mode]).reshape(-1))
                p += px[-1].size
            row.append(p)
        poffs.append(row)
        shapes.append(c["RGB"].shape[:2] if "RGB" in c else (0, 0))
    np.savez_compressed(GOLDEN, names=np.array([c["name"] for c in cases]), streams=np.frombuffer(streams, np.uint8),
                        stream_offsets=offs, pixels=np.concatenate(px), pixel_offsets=np.array(poffs, np.int64),
                        shapes=np.array(shapes, np.int64), supported=np.array([c["supported"] for c in cases]),
                        status=np.array([c["status"] for c in cases], np.int32),
                        pillow_version=np.array(versions["pillow"]), zlib_version=np.array(versions["zlib"]))


def load_corrupt():
    """The mutated zlib streams tools/make_golden_png.py recorded from the host check, with the statuses it printed:
    list of (kind, image, a, b, status, zlib stream bytes); `image` indexes the supported cases of the fixture."""
    z = np.load(CORRUPT, allow_pickle=False)
    offs = z["offsets"]
    return [(str(k), int(r[0]), int(r[1]), int(r[2]), int(r[3]), z["streams"][offs[i]:offs[i + 1]].tobytes())
            for i, (k, r) in enumerate(zip(z["kinds"], z["rows"]))]


def save_corrupt(dumped):
    offs = np.cumsum([0] + [len(d[5]) for d in dumped]).astype(np.int64)
    np.savez_compressed(CORRUPT, kinds=np.array([d[0] for d in dumped]),
                        rows=np.array([d[1:5] for d in dumped], np.int64), offsets=offs,
                        streams=np.frombuffer(b"".join(d[5] for d in dumped), np.uint8))


def with_zlib_stream(data, z):
    """The PNG file `data` with its IDAT chunks replaced by ONE IDAT holding z (how a recorded mutation becomes a
    file again)."""
    d = png.parse_png(data)
    assert d.status == 0
    head = data[:d.idat[0][0] - 8]
    return head + chunk(b"IDAT", z) + chunk(b"IEND", b"")


# ------------------------------------------------------------------------------------------------ the host check
def build_hostcheck(out, sanitize=True):
    return hostcheck.build_hostcheck(HOSTCHECK_SRC, out, sanitize)


def write_hostcheck_input(path, cases, muts=()):
    """The input file of tools/png_hostcheck.cpp from the fixture's SUPPORTED cases: header, descriptors, palettes,
    zlib streams, the expected RGBA pixels, and the mutated zlib streams of mutations().  -> the PngBatch."""
    batch = png.pack_pngs([c["data"] for c in cases])
    assert not batch.status.any()
    head = np.array([0x504E4731, len(cases), batch.palettes.shape[0], batch.streams.numel(), HOSTCHECK_SEED, len(muts),
                     0, 0], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(batch.desc.numpy().tobytes())
        f.write(batch.palettes.numpy().tobytes())
        f.write(batch.streams.numpy().tobytes())
        for c in cases:
            f.write(np.ascontiguousarray(c["RGBA"]).tobytes())
        for m in muts:
            f.write(struct.pack("<ii", m[1], len(m[4])) + m[4])
    return batch


def run_hostcheck(exe, input_path):
    """-> (returncode, stderr, clean [(image, status, match)], statuses of the mutations in the input's order)."""
    import subprocess
    r = subprocess.run([exe, input_path], capture_output=True, text=True)
    clean, muts = [], []
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "C":
            clean.append((int(t[1]), int(t[2]), int(t[3])))
        elif t[0] == "M":
            assert int(t[1]) == len(muts)
            muts.append(int(t[3]))
    return r.returncode, r.stderr, clean, muts


def _lcg(seed):
    state = [seed & 0xffffffff]

    def rnd():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xffffffff
        return state[0] >> 8
    return rnd


def mutations(streams):
    """The mutations the host check runs, generated HERE and written into its input: [(kind, image, a, b, bytes)].
    Kinds: trunc (cut at a), subst (byte a becomes b), hdrbit (bit b of byte a, inside the first block header, flipped),
    splice (bytes [a, b) cut out, or a piece of another place put in), trailer (one of the last 4 bytes changed, or the
    trailer cut)."""
    rnd = _lcg(HOSTCHECK_SEED)
    out = []
    small = sorted(range(len(streams)), key=lambda i: len(streams[i]))
    for i in small[:6]:                                      # truncations at every length of the smallest streams
        z = streams[i]
        for ln in range(len(z)):
            out.append(("trunc", i, ln, 0, z[:ln]))
    for i, z in enumerate(streams):
        n = len(z)
        big = n > 4096                                       # the large streams: fewer of each kind
        for _ in range(8 if big else 24):
            p, v = rnd() % n, rnd() & 255
            out.append(("subst", i, p, v, z[:p] + bytes([v]) + z[p + 1:]))
        for k in range(min(n, 4 if big else 12) * 8):                      # the zlib header, the block header and what follows it
            p, bit = k >> 3, k & 7
            out.append(("hdrbit", i, p, bit, z[:p] + bytes([z[p] ^ (1 << bit)]) + z[p + 1:]))
        for _ in range(6):
            a = rnd() % n
            b = min(n, a + 1 + rnd() % 9)
            out.append(("splice", i, a, b, z[:a] + z[b:]))
            c = rnd() % n
            out.append(("splice", i, a, -c - 1, z[:a] + z[c:c + 5] + z[a:]))
        for k in range(1, 5):
            out.append(("trailer", i, n - k, 1, z[:n - k] + bytes([z[n - k] ^ (1 << (rnd() & 7))]) + z[n - k + 1:]))
            out.append(("trailer", i, n - k, 0, z[:n - k]))
    return out
