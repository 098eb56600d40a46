"""Write tests/golden/g18_jpeg_prog.npz and g18_jpeg_prog_corrupt.npz: progressive JPEG byte strings with the pixels
Pillow (libjpeg-turbo) decodes them to, and the mutations of them the host check decoded with their statuses.

The Pillow-written streams: the edge sizes of the baseline fixture (1x1 .. 33x47) in 4:4:4 / 4:2:2 / 4:2:0 / gray at
qualities 30, 75, 95, restarts off, every 3 blocks, or every MCU row in turn, and four 112x112 faces.  Pillow only
ever writes one scan script, so the rest come from the writer of tests/jpeg_prog_cases.py, on the coefficients of
some of those streams: one-component DC scans, spectral selection alone, an Al chain from bit 3, Pillow's scans
reordered, tables skewed to codes longer than 9 bits under a restart interval in the AC scans -- each with the baseline
stream of the same coefficients -- and one 1024x1024 gray stream whose AC bands are laid out so that every end-of-band
category from EOB0 to EOB14 occurs.  Run from the repository root: python tools/make_golden_jpeg_prog.py"""
import io
import os
import sys
import tempfile

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from make_golden_jpeg import smooth_image, SUB          # noqa: E402
from msml_amd import jpeg                               # noqa: E402
from tests import jpeg_prog_cases as P                  # noqa: E402

SIZES = [(1, 1), (9, 1), (5, 2), (16, 16), (17, 23), (23, 17), (33, 47)]   # (W, H)


def encode(arr, mode, quality, restart):
    im = Image.fromarray(arr)
    kw = {}
    if mode == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = SUB[mode]
    if restart == 1:
        kw["restart_marker_blocks"] = 3
    elif restart == 2:
        kw["restart_marker_rows"] = 1
    f = io.BytesIO()
    im.save(f, "JPEG", quality=quality, progressive=True, **kw)
    return f.getvalue()


def scripts(nc):
    comps = range(nc)
    dc1 = [((c,), 0, 0, 0, 0) for c in comps] + [((c,), 1, 63, 0, 0) for c in comps]
    spectral = [(tuple(comps), 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in comps for a, b in ((1, 5), (6, 20), (21, 63))]
    deep = [(tuple(comps), 0, 0, 0, 3)] + [((c,), 1, 63, 0, 3) for c in comps]
    for al in (2, 1, 0):
        deep += [(tuple(comps), 0, 0, al + 1, al)] + [((c,), 1, 63, al + 1, al) for c in reversed(comps)]
    return {"dc1": dc1, "spectral": spectral, "deep": deep}


def eob_stream():
    """1024 x 1024 gray, 16384 blocks: band 1..5 is zero everywhere (one EOB14), band 6..20 has single coefficients
    behind runs of 1, 2, 4 .. 4096 zero blocks (EOB0 .. EOB12), band 21..63 one coefficient behind 8192 (EOB13)."""
    d = jpeg.JpegDescriptor()
    d.height = d.width = 1024
    d.components, d.sampling, d.qsel = 1, ((1, 1),), (0,)
    d.qtables = {0: jpeg.quant_tables(75)[0]}
    coef = np.zeros((128 * 128, 64), np.int64)
    coef[:, 0] = (np.arange(128 * 128) * 7 % 41) - 20
    at = 0
    for n in range(13):
        at += 1 << n
        coef[at, jpeg.ZIGZAG[6 + n]] = 3 if n & 1 else -2
        at += 1
    coef[8192, jpeg.ZIGZAG[30]] = -5
    coefs = [coef.reshape(128, 128, 64)]
    script = [((0,), 0, 0, 0, 0), ((0,), 1, 5, 0, 0), ((0,), 6, 20, 0, 0), ((0,), 21, 63, 0, 0)]
    return P.write_progressive(coefs, d, script), P.write_baseline(coefs, d)


def main():
    rng = np.random.RandomState(18)
    cases, k = [], 0                                   # (name, bytes, baseline stream of the same coefficients)
    for w, h in SIZES:
        src = smooth_image(rng, w, h)
        for mode in ("444", "422", "420", "gray"):
            q, r = (30, 75, 95)[k % 3], (k // 3 + k) % 3
            cases.append(("%dx%d_%s_q%d_r%d" % (w, h, mode, q, r), encode(src, mode, q, r), b""))
            k += 1
    faces = [smooth_image(rng, 112, 112) for _ in range(4)]
    cases.append(("face0_112x112_420_q95_r1", encode(faces[0], "420", 95, 1), b""))
    cases.append(("face1_112x112_444_q95_r0", encode(faces[1], "444", 95, 0), b""))
    cases.append(("face2_112x112_422_q75_r2", encode(faces[2], "422", 75, 2), b""))
    cases.append(("face3_112x112_gray_q95_r0", encode(faces[3], "gray", 95, 0), b""))
    by = {c[0]: c[1] for c in cases}
    for prefix in ("17x23_420_", "9x1_422_", "16x16_444_", "23x17_gray_", "33x47_420_"):
        name = next(n for n in by if n.startswith(prefix))
        coefs, d = P.coefficients(by[name])
        base = P.write_baseline(coefs, d)
        for sname, script in scripts(d.components).items():
            cases.append(("w_%s_%s" % (sname, name), P.write_progressive(coefs, d, script), base))
        pil = P.PILLOW_SCRIPT_3 if d.components == 3 else [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)]
        cases.append(("w_skew_%s" % name, P.write_progressive(coefs, d, pil, restart=2, skew=True), base))
        if d.components == 3:
            head, ch = P.split_scans(by[name])
            cases.append(("w_reorder_%s" % name, P.join_scans(head, [ch[i] for i in (0, 3, 2, 1, 4, 5, 6, 9, 8, 7)]), base))
    prog, base = eob_stream()
    cases.append(("w_eobs_1024x1024_gray", prog, base))

    streams, pixels, bases, soff, poff, boff, shapes = [], [], [], [0], [0], [0], []
    for name, data, base in cases:
        px = np.asarray(Image.open(io.BytesIO(data)))
        assert px.dtype == np.uint8 and jpeg.parse_jpeg(data, progressive=True).status == 0, name
        if base:
            assert np.array_equal(px, np.asarray(Image.open(io.BytesIO(base)))), name
        streams.append(np.frombuffer(data, np.uint8))
        bases.append(np.frombuffer(base, np.uint8))
        pixels.append(px.reshape(-1))
        soff.append(soff[-1] + len(data))
        boff.append(boff[-1] + len(base))
        poff.append(poff[-1] + px.size)
        shapes.append(tuple(px.shape) + (0,) * (3 - px.ndim))
    np.savez_compressed(
        P.GOLDEN, names=np.array([c[0] for c in cases]), streams=np.concatenate(streams),
        stream_offsets=np.array(soff, np.int64), bases=np.concatenate(bases), base_offsets=np.array(boff, np.int64),
        pixels=np.concatenate(pixels), pixel_offsets=np.array(poff, np.int64), shapes=np.array(shapes, np.int64),
        pillow_version=np.array(Image.__version__), libjpeg_turbo_version=np.array(str(features.version_feature("libjpeg_turbo"))))
    print("%d streams, %d bytes -> %s (%d bytes)" % (len(cases), soff[-1], P.GOLDEN, os.path.getsize(P.GOLDEN)))
    corrupt()


def corrupt():
    """g18_jpeg_prog_corrupt.npz: the mutations tools/jpeg_prog_hostcheck.cpp dumps, with the statuses the host decoder
    gave them -- the only corrupt inputs the GPU tests use (needs a host C++ compiler)."""
    cases, _ = P.load_golden()
    with tempfile.TemporaryDirectory() as tmp:
        exe = P.build_hostcheck(os.path.join(tmp, "hostcheck"))
        P.write_hostcheck_input(os.path.join(tmp, "in.bin"), cases)
        rc, err, clean, muts, dumped = P.run_hostcheck(exe, os.path.join(tmp, "in.bin"))
    assert rc == 0 and not err, (rc, err[-3000:])
    assert all(st == 0 and m == 1 for (i, st, m) in clean), "the host decoder misses the fixture"
    P.save_corrupt(dumped)
    print("%d mutations, %d recorded -> %s (%d bytes)" % (len(muts), len(dumped), P.CORRUPT, os.path.getsize(P.CORRUPT)))


if __name__ == "__main__":
    sys.exit(main())
