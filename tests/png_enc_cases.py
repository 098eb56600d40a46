"""PNG encoding restated in numpy (msml_amd/csrc/png_enc_core.h): the filter pass with the adaptive rule bit for bit, the
container with its CRCs, the bound, a deterministic CPU encoder (all stored blocks: the simplest valid stream, NOT the
device's tokens), and the reference cost the size test uses: optimal 15-bit-limited Huffman code lengths (package-merge)
over the literal + end-of-block alphabet of a byte string.  Also the fixture (tests/golden/g19_png_enc.npz), the test
shapes, and the host check's file formats."""
import os
import struct
import subprocess
import zlib

import numpy as np

from tests import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g19_png_enc.npz")
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHUNK = 65535                       # filtered bytes per deflate block of the device encoder
HEADER_BITS_MAX = 17 + 19 * 3 + 316 * 7   # block bits, HLIT / HDIST / HCLEN, the code-length code, 316 lengths of 7 bits


def as_hwc(img):
    a = np.asarray(img, np.uint8)
    return a[:, :, None] if a.ndim == 2 else a


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, filter="adaptive", order="rgb"):
    """-> uint8 [H, 1 + W * C]: the filter byte and the filtered row, every row from the raw row above it."""
    a = as_hwc(img)
    h, w, c = a.shape
    if order == "bgr" and c >= 3:
        a = a[:, :, [2, 1, 0] + ([3] if c == 4 else [])]
    raw = a.reshape(h, w * c).astype(np.int64)
    out = np.zeros((h, 1 + w * c), np.uint8)
    zero = np.zeros(w * c, np.int64)
    for y in range(h):
        x = raw[y]
        up = raw[y - 1] if y else zero
        left = np.concatenate([zero[:c], x[:-c]]) if w * c > c else zero[:w * c].copy()
        ul = np.concatenate([zero[:c], up[:-c]]) if w * c > c else zero[:w * c].copy()
        cand = np.stack([x, x - left, x - up, x - ((left + up) >> 1), x - _paeth(left, up, ul)]) & 255
        if filter == "adaptive":
            sums = np.where(cand < 128, cand, 256 - cand).sum(axis=1)
            f = int(np.argmin(sums))                    # the first smallest: ties go to the lowest filter number
        else:
            f = FILTERS[filter]
        out[y, 0] = f
        out[y, 1:] = cand[f]
    return out


def filtered_bytes(img, filter="adaptive", order="rgb"):
    return filter_rows(img, filter, order).tobytes()


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def stored_stream(data):
    """zlib header, stored blocks of at most 65535 bytes, Adler-32."""
    out = [b"\x78\x01"]
    n = len(data)
    for o in range(0, n, 65535):
        part = data[o:o + 65535]
        out.append(bytes([1 if o + 65535 >= n else 0]) + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part)
    return b"".join(out) + struct.pack(">I", zlib.adler32(data))


def container(height, width, channels, stream):
    ihdr = struct.pack(">IIBBBBB", width, height, 8, COLOUR_TYPE[channels], 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


def encode(img, filter="adaptive", order="rgb"):
    """The deterministic CPU encoder: the filter pass, stored blocks, the container."""
    a = as_hwc(img)
    return container(a.shape[0], a.shape[1], a.shape[2], stored_stream(filtered_bytes(a, filter, order)))


def bound(height, width, channels):
    n = height * (width * channels + 1)
    return 8 + 25 + 12 + 2 + n + 5 * -(-n // 65535) + 4 + 12


def idat_of(data):
    """The IDAT payload of a file with one IDAT chunk (asserts the layout the encoder promises)."""
    assert data[:8] == SIGNATURE and data[12:16] == b"IHDR" and data[37:41] == b"IDAT"
    n = struct.unpack(">I", data[33:37])[0]
    assert data[41 + n + 4:] == chunk(b"IEND", b""), "one IDAT, then IEND"
    return data[41:41 + n]


def limited_lengths(counts, limit=15):
    """Optimal prefix-code lengths with no length above `limit` (package-merge) for the symbols with a count."""
    counts = np.asarray(counts, np.int64)
    syms = np.flatnonzero(counts)
    lens = np.zeros(len(counts), np.int64)
    n = len(syms)
    if n == 1:
        lens[syms[0]] = 1
        return lens
    order = syms[np.argsort(counts[syms], kind="stable")]
    leaves = [(int(counts[s]), np.eye(n, dtype=np.int64)[i]) for i, s in enumerate(order)]
    prev = list(leaves)
    for _ in range(limit - 1):
        packs = [(prev[i][0] + prev[i + 1][0], prev[i][1] + prev[i + 1][1]) for i in range(0, len(prev) - 1, 2)]
        prev = sorted(leaves + packs, key=lambda t: t[0])
    take = sum(t[1] for t in prev[:2 * n - 2])
    lens[order] = take
    assert (2.0 ** -lens[order]).sum() <= 1 + 1e-12 and lens.max() <= limit
    return lens


def literal_cost_bits(data, limit=15):
    """B: the bits of the bytes of `data` and one end-of-block under the optimal length-limited code of their counts."""
    counts = np.zeros(257, np.int64)
    counts[:256] = np.bincount(np.frombuffer(data, np.uint8), minlength=256)
    counts[256] = 1
    return int((counts * limited_lengths(counts, limit)).sum())


def size_limit(filtered):
    """What a file may take at most, from references that do not involve the code under test: every block of CHUNK bytes
    has "dynamic, literals only" among its candidates, whose header costs at most HEADER_BITS_MAX bits; coding every
    block with the whole string's optimal code costs B plus one more end-of-block (at most 15 bits) per extra block, and
    each block's own optimal code is no worse.  A block leaves as stored only where that is cheaper still."""
    blocks = -(-len(filtered) // CHUNK)
    bits = blocks * HEADER_BITS_MAX + literal_cost_bits(filtered) + 15 * (blocks - 1)
    return 8 + 25 + 12 + 12 + 2 + 4 + -(-bits // 8)


# ------------------------------------------------------------------------------------------------------------ cases
def synthetic():
    """name -> array: the shapes tests/test_gpu_png_enc.py lists."""
    r = np.random.RandomState(19)
    out = {}
    for c in (1, 2, 3, 4):
        for h, w in ((1, 1), (1, 300), (300, 1)):
            out["s%dx%dx%d" % (h, w, c)] = r.randint(0, 256, (h, w, c)).astype(np.uint8)
    out["rgba7x5"] = r.randint(0, 256, (7, 5, 4)).astype(np.uint8)
    out["flat"] = np.full((112, 112, 3), 97, np.uint8)
    out["noise"] = r.randint(0, 256, (200, 150, 3)).astype(np.uint8)
    out["rows"] = np.repeat(r.randint(0, 256, (1, 150, 3)).astype(np.uint8), 200, axis=0)
    return out


def tall(width, channels=1, seed=7):
    """3 rows x width, identical rows of noise: with filter "none" the row-to-row distance is width * channels + 1."""
    r = np.random.RandomState(seed)
    return np.repeat(r.randint(0, 256, (1, width, channels)).astype(np.uint8), 3, axis=0)


def load_golden():
    """name -> array of tests/golden/g19_png_enc.npz (faces, the decoded 8-bit PNG fixtures, the synthetic shapes)."""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------------- host check
def build_hostcheck(out):
    return hostcheck.build_hostcheck(os.path.join(ROOT, "tools", "png_enc_hostcheck.cpp"), out)


def write_hostcheck_input(path, cases):
    """cases: [(array [H, W, C], filter name, order)]."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for a, flt, order in cases:
            a = as_hwc(a)
            f.write(struct.pack("<5i", a.shape[0], a.shape[1], a.shape[2], FILTERS[flt], 1 if order == "bgr" else 0))
            f.write(np.ascontiguousarray(a).tobytes())


def run_hostcheck(exe, inp, out):
    r = subprocess.run([exe, inp, out], capture_output=True, text=True)
    files = []
    if r.returncode == 0:
        with open(out, "rb") as f:
            blob = f.read()
        o = 0
        while o < len(blob):
            n = struct.unpack("<i", blob[o:o + 4])[0]
            files.append(blob[o + 4:o + 4 + n])
            o += 4 + n
    return r.returncode, r.stderr, files


def random_cases(count, seed=5):
    """Random sizes, channel counts, filters and contents: flat, noise, periodic with periods around 1, 3, 258, 32767,
    32768, 32769 (gray images of 3 x 30000, long enough for two periods), small images of every kind."""
    r = np.random.RandomState(seed)
    names = list(FILTERS)
    cases = []
    for i in range(count):
        c = int(r.randint(1, 5))
        h, w = int(r.randint(1, 40)), int(r.randint(1, 40))
        kind = i % 4
        if kind == 0:
            a = np.full((h, w, c), r.randint(0, 256), np.uint8)
        elif kind == 1:
            a = r.randint(0, 256, (h, w, c)).astype(np.uint8)
        elif kind == 2:
            p = int(r.choice([1, 2, 3, 4, 5, 7]))
            a = np.resize(r.randint(0, 256, p).astype(np.uint8), (h, w, c))
        else:
            a = (r.randint(0, 4, (h, w, c)) * 60).astype(np.uint8)
        cases.append((a, names[int(r.randint(0, 6))], "bgr" if c >= 3 and r.randint(0, 2) else "rgb"))
    for p in (257, 258, 259, 32767, 32768, 32769):
        pat = r.randint(0, 256, p).astype(np.uint8)
        cases.append((np.resize(pat, (3, 30000, 1)), "none", "rgb"))
        if p > 1000:
            c = 1 if p <= 32768 else 2                 # filtered rows of p bytes (sizes end at 32767: two channels)
            cases.append((np.repeat(pat[None, :p - 1], 3, axis=0).reshape(3, (p - 1) // c, c), "none", "rgb"))
    return cases
