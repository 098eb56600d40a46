"""Write tests/golden/g16_jpeg_enc.npz: source pixels, option sets and the JPEG bytes Pillow (libjpeg-turbo) writes for them.

Pillow only.  Every source is an RGB image; a gray stream is Pillow's save of convert("L"), whose luma is libjpeg's Y
bit for bit (asserted below), so the encoder takes the same RGB source with sampling "gray".  The images come from the
generator of tools/make_golden_jpeg.py.  Run from the repository root: python tools/make_golden_jpeg_enc.py"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_jpeg import checker, smooth_image  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g16_jpeg_enc.npz")
SIZES = [(1, 1), (8, 8), (5, 2), (9, 1), (1, 7), (16, 8), (17, 23), (3, 40), (40, 3), (33, 17)]      # (W, H)
MODES = ("gray", "444", "422", "420")                      # the sampling codes 0..3 of csrc/jpeg_enc_core.h
SUB = {"444": 0, "422": 1, "420": 2}


def encode(arr, mode, quality, restart=0, bare=False):
    im = Image.fromarray(arr)
    f = io.BytesIO()
    if bare:                                               # Pillow's defaults: quality 75, 4:2:0
        assert (mode, quality, restart) == ("420", 75, 0)
        im.save(f, "JPEG")
        return f.getvalue()
    kw = {}
    if mode == "gray":
        im = im.convert("L")
        a = arr.astype(np.int64)
        assert np.array_equal(np.asarray(im), (a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 32768) >> 16)
    else:
        kw["subsampling"] = SUB[mode]
    if restart:
        kw["restart_marker_blocks"] = restart
    im.save(f, "JPEG", quality=quality, **kw)
    return f.getvalue()


def columns(w, h, period):
    x = np.arange(w)
    row = np.where((x // period) & 1, 255, 0).astype(np.uint8)
    return np.repeat(np.repeat(row[None, :, None], h, 0), 3, 2)


def scan_of(data):
    sos = data.index(b"\xff\xda")
    ln = (data[sos + 2] << 8) | data[sos + 3]
    return data[sos + 2 + ln:]


def main():
    sys.path[:0] = [ROOT]
    from tests import jpeg_cases
    from msml_amd import jpeg
    rng = np.random.RandomState(16)
    cases = []                                             # (name, source, mode, quality, restart, bytes)

    def add(name, src, mode, q, restart=0, bare=False):
        cases.append(("%s_%s_q%d_r%d" % (name, mode, q, restart), src, mode, q, restart, encode(src, mode, q, restart, bare)))

    k = 0
    for w, h in SIZES:
        src = smooth_image(rng, w, h)
        for mode in ("444", "422", "420", "gray"):
            for q in (30, 75, 95, 100):
                add("%dx%d" % (w, h), src, mode, q, 3 if k % 2 else 0)
                k += 1
    for mode in ("444", "422", "420"):
        add("checker16x16", checker(16, 16), mode, 75)
    add("checker17x9", checker(17, 9), "420", 95, 3)
    add("columns1_24x16", columns(24, 16, 1), "gray", 100)
    add("columns1_24x16", columns(24, 16, 1), "444", 100)
    add("columns8_24x16", columns(24, 16, 8), "gray", 100)
    noise = rng.randint(0, 256, (24, 24, 3)).astype(np.uint8)
    add("noise24x24", noise, "444", 50)
    add("noise24x24", noise, "444", 100)
    add("mcu1_17x23", smooth_image(rng, 17, 23), "420", 75, 1)
    faces = [smooth_image(rng, 112, 112) for _ in range(9)]
    add("face0_112x112_bare", faces[0], "420", 75, bare=True)
    add("face1_112x112", faces[1], "420", 97)              # cvt_casia_webface.py:57
    add("face2_112x112", faces[2], "444", 95, 3)
    add("face3_112x112", faces[3], "422", 75, 3)
    add("face4_112x112", faces[4], "gray", 95)
    for i in range(5, 9):
        add("uniform%d_112x112" % (i - 5), faces[i], "420", 75)

    std = {(tc, th): (list(c), bytes(v)) for (tc, th), (c, v) in jpeg.STD_HUFFMAN.items()}
    n_ff = n_zrl = 0
    cat_ac = cat_dc = 0
    for name, src, mode, q, restart, data in cases:
        d = jpeg.parse_jpeg(data)
        assert d.status == 0 and (d.height, d.width) == src.shape[:2] and d.restart_interval == restart, name
        if mode != "gray":
            assert {k2: (list(c), bytes(v)) for k2, (c, v) in d.huffman.items()} == std, name
        n_ff += b"\xff\x00" in scan_of(data)
        coefs = jpeg_cases.entropy_decode(data, d)
        for c in coefs:
            zz = c.reshape(-1, 64)[:, jpeg.ZIGZAG]
            cat_ac = max(cat_ac, int(np.abs(zz[:, 1:]).max()).bit_length())
            for blk in zz:
                nz = np.flatnonzero(blk[1:])
                gaps = np.diff(np.concatenate([[-1], nz]))
                n_zrl_here = bool(nz.size and (gaps - 1).max() >= 16)
                if n_zrl_here:
                    n_zrl += 1
                    break
        dc = coefs[0][..., 0].reshape(-1)
        if not restart and len(coefs) == 1:
            cat_dc = max(cat_dc, int(np.abs(np.diff(np.concatenate([[0], dc]))).max()).bit_length())
    assert n_ff >= 1, "no stream with a stuffed FF"
    assert n_zrl >= 1, "no stream with a ZRL run"
    assert cat_ac == 10 and cat_dc == 11, (cat_ac, cat_dc)

    soff = np.cumsum([0] + [len(c[5]) for c in cases]).astype(np.int64)
    poff = np.cumsum([0] + [c[1].size for c in cases]).astype(np.int64)
    np.savez_compressed(
        OUT, names=np.array([c[0] for c in cases]),
        options=np.array([(MODES.index(c[2]), c[3], c[4]) for c in cases], np.int32),      # sampling, quality, restart
        shapes=np.array([c[1].shape[:2] for c in cases], np.int64),
        sources=np.concatenate([c[1].reshape(-1) for c in cases]), source_offsets=poff,
        streams=np.frombuffer(b"".join(c[5] for c in cases), np.uint8), stream_offsets=soff,
        pillow_version=np.array(Image.__version__), libjpeg_turbo_version=np.array(str(features.version_feature("libjpeg_turbo"))))
    print("%d streams (%d with FF 00, %d with ZRL), %d source + %d stream bytes -> %s (%d bytes)" % (
        len(cases), n_ff, n_zrl, poff[-1], soff[-1], OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < (1 << 20)


if __name__ == "__main__":
    sys.exit(main())
