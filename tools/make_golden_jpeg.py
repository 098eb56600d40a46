"""Write tests/golden/g15_jpeg.npz: JPEG byte strings and the pixels Pillow (libjpeg-turbo) decodes them to.

Pillow only.  The images are a smooth random field plus +-12 noise, and one saturated red / blue checker that reaches
the clamps of the colour conversion.  Sizes 1x1 .. 3x40 in 4:4:4 / 4:2:2 / 4:2:0 / gray at qualities 30, 75, 95, 100,
every second stream with a restart interval of 3 blocks; four 112x112 images, one option set each (only these are
kept at full size, so that the file stays small); one stream with a restart interval of one MCU; one stream whose DQT
segments are rewritten with 16-bit entries (libjpeg itself writes such tables only into non-baseline frames); one
progressive and one 4:1:1 stream for the refusals.  Run from the repository root: python tools/make_golden_jpeg.py"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "g15_jpeg.npz")
SIZES = [(1, 1), (8, 8), (9, 1), (9, 2), (9, 3), (5, 2), (1, 7), (16, 16), (17, 23), (15, 33), (40, 3), (3, 40)]   # (W, H)
SUB = {"444": 0, "422": 1, "420": 2}


def smooth_image(rng, w, h):
    gw, gh = max(2, w // 8 + 2), max(2, h // 8 + 2)
    low = Image.fromarray(rng.randint(0, 256, (gh, gw, 3)).astype(np.uint8))
    a = np.asarray(low.resize((w, h), Image.BICUBIC)).astype(np.int64)
    a = a + rng.randint(-12, 13, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def checker(w, h):
    y, x = np.mgrid[:h, :w]
    a = np.zeros((h, w, 3), np.uint8)
    red = ((x // 2 + y // 2) & 1) == 0
    a[red] = (255, 0, 0)
    a[~red] = (0, 0, 255)
    return a


def encode(arr, mode, quality, restart=0, **kw):
    im = Image.fromarray(arr)
    if mode == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = SUB[mode]
    if restart:
        kw["restart_marker_blocks"] = restart
    f = io.BytesIO()
    im.save(f, "JPEG", quality=quality, **kw)
    return f.getvalue()


def dqt16(data):
    """The same stream with every DQT entry written as 16 bits (Pq = 1)."""
    out, pos = bytearray(data[:2]), 2
    while True:
        m = data[pos + 1]
        ln = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + ln]
        if m == 0xDB:
            body, i = bytearray(), 0
            while i < len(seg):
                assert seg[i] >> 4 == 0
                body.append(0x10 | (seg[i] & 15))
                for v in seg[i + 1:i + 65]:
                    body += bytes((0, v))
                i += 65
            out += bytes((0xFF, 0xDB, (len(body) + 2) >> 8, (len(body) + 2) & 255)) + body
        else:
            out += data[pos:pos + 2 + ln]
        pos += 2 + ln
        if m == 0xDA:
            return bytes(out + data[pos:])


def has_ff00(data):
    sos = data.index(b"\xff\xda")
    return b"\xff\x00" in data[sos:]


def main():
    rng = np.random.RandomState(15)
    cases = []                                   # (name, bytes, supported)
    k = 0
    for w, h in SIZES:
        src = smooth_image(rng, w, h)
        for mode in ("444", "422", "420", "gray"):
            for q in (30, 75, 95, 100):
                restart = 3 if k % 2 else 0
                cases.append(("%dx%d_%s_q%d_r%d" % (w, h, mode, q, restart), encode(src, mode, q, restart), True))
                k += 1
    for mode in ("444", "422", "420"):
        cases.append(("checker16x16_%s_q75_r0" % mode, encode(checker(16, 16), mode, 75), True))
    cases.append(("checker17x9_420_q95_r3", encode(checker(17, 9), "420", 95, 3), True))
    faces = [smooth_image(rng, 112, 112) for _ in range(4)]
    cases.append(("face0_112x112_420_q95_r3", encode(faces[0], "420", 95, 3), True))
    cases.append(("face1_112x112_444_q95_r0", encode(faces[1], "444", 95), True))
    cases.append(("face2_112x112_422_q75_r3", encode(faces[2], "422", 75, 3), True))
    cases.append(("face3_112x112_gray_q95_r0", encode(faces[3], "gray", 95), True))
    cases.append(("mcu1_17x23_420_q75_r1", encode(smooth_image(rng, 17, 23), "420", 75, 1), True))
    cases.append(("dqt16_17x23_422_q30_r0", dqt16(encode(smooth_image(rng, 17, 23), "422", 30)), True))
    cases.append(("progressive_16x16", encode(smooth_image(rng, 16, 16), "420", 75, progressive=True), False))
    # Pillow writes no 4:1:1 (its "4:1:1" is an old name of 4:2:0).  A 32x16 image is two MCUs of four Y blocks in
    # 4:2:0 (16x16 each) and in 4:1:1 (32x8 each), so the same scan under a patched SOF0 is a valid 4:1:1 stream.
    data = bytearray(encode(smooth_image(rng, 32, 16), "420", 75))
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == 0x22
    data[sof + 11] = 0x41
    cases.append(("s411_32x16", bytes(data), False))
    assert any(has_ff00(d) for _, d, s in cases if s), "no stream with a stuffed FF"

    streams, pixels, soff, poff, shapes = [], [], [0], [0], []
    for name, data, _ in cases:
        px = np.asarray(Image.open(io.BytesIO(data)))
        assert px.dtype == np.uint8
        streams.append(np.frombuffer(data, np.uint8))
        pixels.append(px.reshape(-1))
        soff.append(soff[-1] + len(data))
        poff.append(poff[-1] + px.size)
        shapes.append(tuple(px.shape) + (0,) * (3 - px.ndim))
    np.savez_compressed(
        OUT, names=np.array([c[0] for c in cases]), supported=np.array([c[2] for c in cases]),
        streams=np.concatenate(streams), stream_offsets=np.array(soff, np.int64), pixels=np.concatenate(pixels),
        pixel_offsets=np.array(poff, np.int64), shapes=np.array(shapes, np.int64),
        pillow_version=np.array(Image.__version__ if hasattr(Image, "__version__") else features.version("pil")),
        libjpeg_turbo_version=np.array(str(features.version_feature("libjpeg_turbo"))))
    print("%d streams, %d bytes -> %s (%d bytes)" % (len(cases), soff[-1], OUT, os.path.getsize(OUT)))
    corrupt()


def corrupt():
    """tests/golden/g15_jpeg_corrupt.npz: the mutated streams tools/jpeg_hostcheck.cpp dumps, with the statuses the
    host decoder gave them -- the only corrupt inputs the GPU tests use (needs a host C++ compiler)."""
    import tempfile
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import jpeg_cases
    cases, _ = jpeg_cases.load_golden()
    with tempfile.TemporaryDirectory() as tmp:
        exe = jpeg_cases.build_hostcheck(os.path.join(tmp, "hostcheck"))
        jpeg_cases.write_hostcheck_input(os.path.join(tmp, "in.bin"), cases)
        rc, err, clean, muts, dumped = jpeg_cases.run_hostcheck(exe, os.path.join(tmp, "in.bin"))
    assert rc == 0 and not err, (rc, err)
    assert all(st == 0 and m == 1 for (i, st, m) in clean if cases[i]["supported"]), "the host decoder misses the fixture"
    jpeg_cases.save_corrupt(dumped)
    print("%d mutations, %d recorded -> %s (%d bytes)" % (len(muts), len(dumped), jpeg_cases.CORRUPT,
                                                           os.path.getsize(jpeg_cases.CORRUPT)))


if __name__ == "__main__":
    sys.exit(main())
