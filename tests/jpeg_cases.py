"""The baseline JPEG decoder of csrc/jpeg_core.h restated in numpy, step by step as libjpeg does it with its defaults
(Huffman decoding with restarts, JDCT_ISLOW, fancy upsampling with its plain replication for planes of width <= 2, the
16-bit fixed-point YCbCr conversion).  The GPU and host-check tests compare with this; tests/test_jpeg_cpu.py pins it
to the bytes Pillow (libjpeg-turbo) wrote into tests/golden/g15_jpeg.npz.  Only the header comes from
msml_amd.jpeg.parse_jpeg; the entropy-coded bytes are walked here, bit by bit, with the canonical codes of DHT."""
import os
import struct

import numpy as np

from msml_amd import jpeg
from tests import hostcheck
from tests.hostcheck import host_compiler, sanitizers_link  # noqa: F401 (the tests reach them through this module)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_jpeg.npz")


class Corrupt(Exception):
    def __init__(self, status):
        super().__init__(jpeg.STATUS[status])
        self.status = status


def load_golden():
    """-> list of dicts {name, data (bytes), pixels (uint8 [H,W,3] or [H,W]), supported (bool)} and the version strings."""
    z = np.load(GOLDEN, allow_pickle=False)
    names = [str(s) for s in z["names"]]
    offs = z["stream_offsets"]
    poffs = z["pixel_offsets"]
    shapes = z["shapes"]
    out = []
    for i, name in enumerate(names):
        data = z["streams"][offs[i]:offs[i + 1]].tobytes()
        shape = tuple(int(v) for v in shapes[i] if v > 0)
        px = z["pixels"][poffs[i]:poffs[i + 1]].reshape(shape)
        out.append({"name": name, "data": data, "pixels": px, "supported": bool(z["supported"][i])})
    return out, {"pillow": str(z["pillow_version"]), "libjpeg_turbo": str(z["libjpeg_turbo_version"])}


def _codes(counts, symbols):
    table, code, p = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            table[(ln, code)] = symbols[p]
            code += 1
            p += 1
        code <<= 1
    return table


class _Bits:
    """libjpeg's bit source: FF 00 is a data byte FF, a marker (or the end) feeds zeros from there on."""

    def __init__(self, data, pos, end):
        self.d, self.pos, self.end = data, pos, end
        self.bits = []          # pending bits of the current byte
        self.fake = 0           # bits handed out that were never in the data

    def bit(self):
        if not self.bits:
            c = None
            if self.pos < self.end:
                c = self.d[self.pos]
                if c == 0xFF:
                    q = self.pos + 1
                    while q < self.end and self.d[q] == 0xFF:
                        q += 1
                    if q < self.end and self.d[q] == 0:
                        self.pos = q + 1
                    else:
                        c = None
                else:
                    self.pos += 1
            if c is None:
                self.fake += 1
                return 0
            self.bits = [(c >> (7 - i)) & 1 for i in range(8)]
        return self.bits.pop(0)

    def receive(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | self.bit()
            if (ln, code) in table:
                return table[(ln, code)]
        raise Corrupt(1)

    def restart(self, index):
        if self.fake:
            raise Corrupt(5)
        self.bits = []
        q = self.pos
        if q >= self.end or self.d[q] != 0xFF:
            raise Corrupt(4)
        while q < self.end and self.d[q] == 0xFF:
            q += 1
        if q >= self.end or self.d[q] != 0xD0 + (index & 7):
            raise Corrupt(4)
        self.pos = q + 1


def extend(v, k):
    return v if v >= (1 << (k - 1)) else v - (1 << k) + 1


def entropy_decode(data, d):
    """-> per component an int array [blocks_y, blocks_x, 64] of coefficients in natural order."""
    hm, vm = d.sampling[0]
    mcux, mcuy = -(-d.width // (8 * hm)), -(-d.height // (8 * vm))
    coefs = [np.zeros((mcuy * v, mcux * h, 64), np.int64) for h, v in d.sampling]
    dct = [_codes(*d.huffman[(0, s)]) for s in d.dcsel]
    act = [_codes(*d.huffman[(1, s)]) for s in d.acsel]
    b = _Bits(data, d.begin, d.end)
    pred = [0] * d.components
    left, rst = d.restart_interval, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if d.restart_interval:
                if left == 0:
                    b.restart(rst)
                    rst += 1
                    pred = [0] * d.components
                    left = d.restart_interval
                left -= 1
            for c, (h, v) in enumerate(d.sampling):
                for yy in range(v):
                    for xx in range(h):
                        blk = coefs[c][my * v + yy, mx * h + xx]
                        s = b.symbol(dct[c])
                        if s > 11:
                            raise Corrupt(3)
                        if s:
                            pred[c] += extend(b.receive(s), s)
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = b.symbol(act[c])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                if k > 64:
                                    raise Corrupt(2)
                                continue
                            if s > 10:
                                raise Corrupt(3)
                            k += r
                            if k > 63:
                                raise Corrupt(2)
                            blk[jpeg.ZIGZAG[k]] = extend(b.receive(s), s)
                            k += 1
            if b.fake:
                raise Corrupt(5)
    return coefs


def _idct_pass(x, n):
    """x [..., 8] along the last axis -> the 8 outputs, descaled by n bits (jidctint.c)."""
    i0, i1, i2, i3, i4, i5, i6, i7 = [x[..., k] for k in range(8)]
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)
    return (out + (1 << (n - 1))) >> n


def idct_blocks(coef, q):
    """coef int [by, bx, 64] natural order, q int [64] -> the uint8 plane [by * 8, bx * 8]."""
    by, bx, _ = coef.shape
    x = (coef * q.astype(np.int64)).reshape(by, bx, 8, 8)            # [row v][column u]
    x = _idct_pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)          # columns first
    x = _idct_pass(x, 18)                                            # then rows
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def upsample_h2v1(p):
    """p uint8 [dh, dw] (the cropped plane) -> [dh, 2 dw]."""
    p = p.astype(np.int64)
    dh, dw = p.shape
    if dw <= 2:
        return np.repeat(p, 2, axis=1)
    left = np.concatenate([p[:, :1], p[:, :-1]], 1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((dh, 2 * dw), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def upsample_h2v2(p):
    """p uint8 [dh, dw] -> [2 dh, 2 dw]."""
    p = p.astype(np.int64)
    dh, dw = p.shape
    if dw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up = np.concatenate([p[:1], p[:-1]], 0)
    down = np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for v, other in ((0, up), (1, down)):
        s = 3 * p + other
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        rows = np.empty((dh, 2 * dw), np.int64)
        rows[:, 0::2] = (3 * s + left + 8) >> 4
        rows[:, 1::2] = (3 * s + right + 7) >> 4
        rows[:, 0] = (4 * s[:, 0] + 8) >> 4
        rows[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[v::2] = rows
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """JPEG bytes -> uint8 [H, W, 3] RGB, or [H, W] for a gray stream.  Raises Corrupt(status) / ValueError (refused)."""
    d = jpeg.parse_jpeg(data)
    if d.status:
        raise ValueError(d.reason)
    coefs = entropy_decode(data, d)
    planes = [idct_blocks(coefs[c], d.qtables[d.qsel[c]]) for c in range(d.components)]
    h, w = d.height, d.width
    if d.components == 1:
        return planes[0][:h, :w]
    hm, vm = d.sampling[0]
    dw, dh = -(-w // hm), -(-h // vm)
    chroma = []
    for p in planes[1:]:
        p = p[:dh, :dw]
        if (hm, vm) == (2, 1):
            p = upsample_h2v1(p)
        elif (hm, vm) == (2, 2):
            p = upsample_h2v2(p)
        chroma.append(p[:h, :w])
    return ycc_to_rgb(planes[0][:h, :w], chroma[0], chroma[1])


def as_rgb(px):
    """a fixture / decode() result as [H, W, 3] (a gray image replicated)."""
    return px if px.ndim == 3 else np.repeat(px[:, :, None], 3, axis=2)


# ------------------------------------------------------------------------------------------- the host check
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SRC = os.path.join(ROOT, "tools", "jpeg_hostcheck.cpp")
CORRUPT = os.path.join(os.path.dirname(GOLDEN), "g15_jpeg_corrupt.npz")
HOSTCHECK_SEED = 1515


def build_hostcheck(out, sanitize=True):
    """Compile tools/jpeg_hostcheck.cpp with the host compiler (and the sanitizers) -> out."""
    return hostcheck.build_hostcheck(HOSTCHECK_SRC, out, sanitize)


def write_hostcheck_input(path, cases):
    """The input file of tools/jpeg_hostcheck.cpp from the fixture's cases: header, descriptors, tables, streams and
    the expected RGB pixels of every supported stream.  Truncations run on the two smallest 3-component streams, one
    without and one with restart markers."""
    batch = jpeg.pack_jpegs([c["data"] for c in cases])
    desc = batch.desc.numpy()

    def smallest(with_restart):
        best = -1
        for i, d in enumerate(batch.descriptors):
            if d.status == 0 and d.components == 3 and d.width >= 9 and bool(d.restart_interval) == with_restart:
                if best < 0 or len(cases[i]["data"]) < len(cases[best]["data"]):
                    best = i
        return best

    head = np.array([0x4A484331, len(cases), batch.qtabs.shape[0], batch.htabs.shape[0], batch.streams.numel(),
                     smallest(False), smallest(True), HOSTCHECK_SEED], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(desc.tobytes())
        f.write(batch.qtabs.numpy().tobytes())
        f.write(batch.htabs.numpy().tobytes())
        f.write(batch.streams.numpy().tobytes())
        for c, d in zip(cases, batch.descriptors):
            if d.status == 0:
                f.write(np.ascontiguousarray(as_rgb(c["pixels"])).tobytes())
    return batch


def run_hostcheck(exe, input_path):
    """-> (returncode, stderr, clean [(image, status, match)], mutations [(kind, image, a, b, status)],
    dumped [(kind, image, a, b, status, stream bytes)])."""
    import subprocess
    r = subprocess.run([exe, input_path], capture_output=True, text=True)
    clean, muts, dumped = [], [], []
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "C":
            clean.append((int(t[1]), int(t[2]), int(t[3])))
        elif t[0] == "M":
            muts.append((t[1], int(t[2]), int(t[3]), int(t[4]), int(t[5])))
        elif t[0] == "D":
            dumped.append((t[1], int(t[2]), int(t[3]), int(t[4]), int(t[5]), bytes.fromhex(t[6]) if len(t) > 6 else b""))
    return r.returncode, r.stderr, clean, muts, dumped


def load_corrupt():
    """The mutated streams tools/make_golden_jpeg.py recorded from the host check, with the statuses it printed:
    list of (kind, image, a, b, status, stream bytes)."""
    z = np.load(CORRUPT, allow_pickle=False)
    offs = z["offsets"]
    return [(str(k), int(r[0]), int(r[1]), int(r[2]), int(r[3]), z["streams"][offs[i]:offs[i + 1]].tobytes())
            for i, (k, r) in enumerate(zip(z["kinds"], z["rows"]))]


def save_corrupt(dumped):
    offs = np.cumsum([0] + [len(d[5]) for d in dumped]).astype(np.int64)
    np.savez_compressed(CORRUPT, kinds=np.array([d[0] for d in dumped]),
                        rows=np.array([d[1:5] for d in dumped], np.int64), offsets=offs,
                        streams=np.frombuffer(b"".join(d[5] for d in dumped), np.uint8))


def write_records(tmp_path, records, name="train"):
    """records: [(key, flag, labels, id, id2, body)] -> rec / idx paths.  The package only reads RecordIO; this writer is the tests' own."""
    rec, idx = tmp_path / (name + ".rec"), tmp_path / (name + ".idx")
    with open(rec, "wb") as f, open(idx, "w") as g:
        for key, flag, labels, id1, id2, body in records:
            g.write("%d\t%d\n" % (key, f.tell()))
            if flag > 0:
                payload = struct.pack("<IfQQ", flag, 0.0, id1, id2) + np.asarray(labels, "<f4").tobytes() + body
            else:
                payload = struct.pack("<IfQQ", 0, float(labels), id1, id2) + body
            f.write(struct.pack("<II", 0xCED7230A, len(payload)) + payload + b"\x00" * (-len(payload) % 4))
    return str(rec), str(idx)
