"""The baseline JPEG encoder of csrc/jpeg_enc_core.h restated in numpy, step by step as libjpeg does it for Pillow's
save(): colour conversion, edge expansion and downsampling, JDCT_ISLOW forward, quantisation, dummy blocks, Huffman
coding with the standard tables and restart intervals, byte stuffing, markers.  The GPU tests and the CPU tests compare
with this; tests/test_jpeg_enc_cpu.py pins it to the bytes Pillow (libjpeg-turbo) wrote into
tests/golden/g16_jpeg_enc.npz.  Only the tables and the header come from msml_amd.jpeg (quant_tables, STD_HUFFMAN,
build_header), each pinned to Pillow by a test of its own."""
import os
import subprocess

import numpy as np

from msml_amd import jpeg
from tests import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g16_jpeg_enc.npz")
HOSTCHECK_SRC = os.path.join(ROOT, "tools", "jpeg_enc_hostcheck.cpp")
MODES = ("gray", "444", "422", "420")
HOSTCHECK_RANDOM, HOSTCHECK_SEED = 3000, 1616


def load_golden():
    """-> list of dicts {name, source (uint8 [H, W, 3]), sampling, quality, restart, data (bytes)} and the versions."""
    z = np.load(GOLDEN, allow_pickle=False)
    so, po = z["stream_offsets"], z["source_offsets"]
    out = []
    for i, name in enumerate(z["names"]):
        h, w = (int(v) for v in z["shapes"][i])
        s, q, r = (int(v) for v in z["options"][i])
        out.append({"name": str(name), "source": z["sources"][po[i]:po[i + 1]].reshape(h, w, 3), "sampling": MODES[s],
                    "quality": q, "restart": r, "data": z["streams"][so[i]:so[i + 1]].tobytes()})
    return out, {"pillow": str(z["pillow_version"]), "libjpeg_turbo": str(z["libjpeg_turbo_version"])}


def pack_sources(cases):
    """The sources back to back as ijb.pack_images lays them out: (uint8 buffer, int64 meta [N][4] = offset, H, W, pitch)."""
    meta = np.zeros((len(cases), 4), np.int64)
    parts, off = [], 0
    for i, c in enumerate(cases):
        h, w = c["source"].shape[:2]
        pitch = (3 * w + 3) & ~3
        rows = np.zeros((h, pitch), np.uint8)
        rows[:, :3 * w] = c["source"].reshape(h, 3 * w)
        meta[i] = off, h, w, pitch
        parts.append(rows.reshape(-1))
        off += h * pitch
    return np.concatenate(parts), meta


# ------------------------------------------------------------------------------------------- the restatement
def rgb_to_ycc(a):
    r, g, b = (a[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _expand(p, rows, cols):
    """Replicate the last column out to `cols` and the last row down to `rows`."""
    h, w = p.shape
    p = np.concatenate([p, np.repeat(p[:, -1:], cols - w, 1)], 1) if cols > w else p
    return np.concatenate([p, np.repeat(p[-1:], rows - h, 0)], 0) if rows > h else p


def component_plane(p, hs, vs):
    """A full-resolution plane -> the component's plane of whole blocks (jcprepct.c, jcsample.c): columns replicated
    out to width_in_blocks * 8 * hs BEFORE the horizontal average; rows replicated only up to a multiple of vs, then
    downsampled, then the last DOWNSAMPLED row replicated down to height_in_blocks * 8."""
    h, w = p.shape
    cw, ch = -(-w // hs), -(-h // vs)
    wib, hib = -(-cw // 8), -(-ch // 8)
    p = _expand(p, ch * vs, wib * 8 * hs)
    if hs == 2:
        bias = np.arange(wib * 8) & 1
        if vs == 1:
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        else:
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + bias) >> 2
    return _expand(p, hib * 8, wib * 8)


def _fdct_pass(x, first):
    d = [x[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15

    def ds(v, k):
        return (v + (1 << (k - 1))) >> k
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else ds(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else ds(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = ds(z1 + t13 * 6270, n)
    o[6] = ds(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = ds(a4 + z1 + z3, n), ds(a5 + z2 + z4, n), ds(a6 + z2 + z3, n), ds(a7 + z1 + z4, n)
    return np.stack(o, -1)


def quantised_blocks(plane, q):
    """uint8-valued plane of whole blocks, q int [64] natural -> int64 [by, bx, 64] quantised coefficients, natural order."""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128      # [by, bx, row, column]
    x = _fdct_pass(x, True)                                                           # rows
    x = _fdct_pass(x.swapaxes(-1, -2), False).swapaxes(-1, -2)                        # columns
    c = x.reshape(by, bx, 64)
    div = 8 * q.astype(np.int64)
    return np.sign(c) * ((np.abs(c) + div // 2) // div)


def _code_table(counts, symbols):
    table, code, p = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            table[symbols[p]] = (code, ln)
            code += 1
            p += 1
        code <<= 1
    return table


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = self.n = 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value_bits(v):
    cat = int(abs(v)).bit_length()
    return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)


def encode_block(w, zz, pred, dct, act):
    cat, bits = _value_bits(int(zz[0]) - pred)
    w.put(*dct[cat])
    if cat:
        w.put(bits, cat)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            w.put(*act[0xF0])
            run -= 16
        cat, bits = _value_bits(v)
        w.put(*act[(run << 4) | cat])
        w.put(bits, cat)
        run = 0
    if run:
        w.put(*act[0])


def coefficients(src, sampling):
    """-> (per component the plane of whole blocks, (hs, vs)) of an RGB [H, W, 3] or gray [H, W] source."""
    hs, vs = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}[sampling]
    if src.ndim == 2:
        return [component_plane(src.astype(np.int64), 1, 1)], (hs, vs)
    y, cb, cr = rgb_to_ycc(src)
    if sampling == "gray":
        return [component_plane(y, 1, 1)], (hs, vs)
    return [component_plane(y, 1, 1), component_plane(cb, hs, vs), component_plane(cr, hs, vs)], (hs, vs)


def encode(src, sampling="420", quality=75, restart=0):
    """uint8 RGB [H, W, 3] (or gray [H, W] with sampling "gray") -> the JPEG bytes."""
    h, w = src.shape[:2]
    qt = jpeg.quant_tables(quality)
    planes, (hs, vs) = coefficients(src, sampling)
    coefs = [quantised_blocks(p, qt[1 if c else 0])[..., jpeg.ZIGZAG] for c, p in enumerate(planes)]
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    tables = [(_code_table(*jpeg.STD_HUFFMAN[(0, t)]), _code_table(*jpeg.STD_HUFFMAN[(1, t)])) for t in (0, 1)]
    out = bytearray(jpeg.build_header(h, w, sampling, qt, restart))
    bw = _BitWriter()
    pred = [0] * len(coefs)
    left, rst = restart, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if restart:
                if left == 0:
                    bw.flush()
                    bw.out += bytes((0xFF, 0xD0 + (rst & 7)))
                    rst += 1
                    pred = [0] * len(coefs)
                    left = restart
                left -= 1
            for c, cf in enumerate(coefs):
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                last_dc = None
                for yy in range(cv):
                    for xx in range(ch):
                        by, bx = my * cv + yy, mx * ch + xx
                        if by < cf.shape[0] and bx < cf.shape[1]:
                            zz = cf[by, bx]
                        else:                                # a dummy block: the DC of the previous block of the MCU
                            zz = np.zeros(64, np.int64)
                            zz[0] = last_dc
                        encode_block(bw, zz, pred[c], *tables[1 if c else 0])
                        pred[c] = last_dc = int(zz[0])
    bw.flush()
    return bytes(out + bw.out + b"\xff\xd9")


# ------------------------------------------------------------------------------------------- the host check
def build_hostcheck(out, sanitize=True):
    """Compile tools/jpeg_enc_hostcheck.cpp with the host compiler (and the sanitizers) -> out."""
    return hostcheck.build_hostcheck(HOSTCHECK_SRC, out, sanitize)


def write_hostcheck_input(path, cases, random_cases=HOSTCHECK_RANDOM):
    """The input file of tools/jpeg_enc_hostcheck.cpp: header, descriptors, meta, tables, headers and the packed sources."""
    src, meta = pack_sources(cases)
    plan = jpeg.EncodePlan([c["source"].shape[:2] for c in cases], [c["quality"] for c in cases],
                           [c["sampling"] for c in cases], [c["restart"] for c in cases])
    head = np.array([0x4A454331, len(cases), plan.qtabs.shape[0], plan.headers.numel(), src.size, random_cases,
                     HOSTCHECK_SEED, 0], np.int32)
    with open(path, "wb") as f:
        for part in (head, plan.desc.numpy(), meta, plan.qtabs.numpy(), plan.headers.numpy(), src):
            f.write(np.ascontiguousarray(part).tobytes())
    return plan


def run_hostcheck(exe, input_path, output_path, n):
    """-> (returncode, stdout, stderr, [(status, stream bytes)] of the n fixture cases)."""
    r = subprocess.run([exe, input_path, output_path], capture_output=True, text=True)
    streams = []
    if os.path.exists(output_path):
        raw = open(output_path, "rb").read()
        pos = 0
        while pos + 8 <= len(raw) and len(streams) < n:
            st, ln = np.frombuffer(raw, np.int32, 2, pos)
            streams.append((int(st), raw[pos + 8:pos + 8 + ln]))
            pos += 8 + int(ln)
    return r.returncode, r.stdout, r.stderr, streams
