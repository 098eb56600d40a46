"""Writes tests/golden/g17_png.npz and g17_png_corrupt.npz: small PNG streams (tests/png_cases.py's writer and token-
level DEFLATE writer, plus two files Pillow wrote itself) with the L / RGB / RGBA arrays the installed Pillow gives for
them, and a selection of mutated zlib streams with the statuses tools/png_hostcheck.cpp printed.  Needs Pillow and a
host compiler; the tests need neither the tool nor a compiler to read the fixture.

    python tools/make_golden_png.py
"""
import io
import os
import sys
import tempfile
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import png_cases as pc  # noqa: E402
from msml_amd import png  # noqa: E402


def content(h, w, spp, depth, seed):
    """Smooth ramps with a little noise (so that every filter has something to predict and the fixture stays small)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [(x * (3 + k) + y * (5 - k) + rng.randint(0, 6, (h, w)) * (rng.randint(0, 8, (h, w)) == 0) + 40 * k) & 255
              for k in range(spp)]
    s = np.stack(planes, axis=2).astype(np.uint8)
    if depth < 8:
        s >>= 8 - depth
    return s.reshape(h, w * spp)


def token_image(name, blocks, row=16):
    """A gray 8-bit image whose filtered bytes are what `blocks(deflate)` emits: every literal is 0..4, so any byte may
    stand where a filter byte falls.  blocks returns the bytes its tokens stand for; a last fixed block pads to whole
    rows."""
    d = pc.Deflate()
    raw = blocks(d)
    pad = (-len(raw)) % row
    d.fixed([0] * pad, final=True)
    raw += bytes(pad)
    z = d.finish(raw)
    assert zlib.decompress(z) == raw
    return name, pc.write_png(row - 1, len(raw) // row, 8, 0, zstream=z)


def pattern(n, seed):
    rng = np.random.RandomState(seed)
    return [int(v) for v in rng.randint(0, 5, n)]


def build_cases():
    cases = []

    def add(name, data):
        cases.append((name, data))

    sizes = [(1, 1), (1, 7), (7, 1), (3, 5), (17, 13)]
    combos = [(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)]
    k = 0
    for ct, dp in combos:
        spp = png.CHANNELS_OF[ct]
        for h, w in sizes if (ct, dp) in ((0, 8), (2, 8), (6, 8)) else sizes[k % 5:k % 5 + 1] + [(17, 13)]:
            plte = bytes((7 + 5 * i) & 255 for i in range(3 * (1 << dp))) if ct == 3 else None
            add("ct%d_d%d_%dx%d_cycle" % (ct, dp, h, w),
                pc.write_png(w, h, dp, ct, content(h, w, spp, dp, k), filters=(0, 1, 2, 3, 4), plte=plte))
            k += 1
    for ct in (0, 4, 2, 6):                                   # every filter on every bpp, from the first row on
        spp = png.CHANNELS_OF[ct]
        for ft in range(5):
            add("bpp%d_filter%d_3x5" % (spp, ft), pc.write_png(5, 3, 8, ct, content(3, 5, spp, 8, 50 + ft), filters=(ft,)))
    for dp in (1, 2, 4):
        add("ct0_d%d_9x17_paeth_avg" % dp, pc.write_png(17, 9, dp, 0, content(9, 17, 1, dp, 70 + dp), filters=(4, 3, 1, 2)))
    ties = np.array([[10, 10, 20, 20, 10, 30, 30, 10], [10, 20, 20, 10, 10, 30, 10, 30]] * 4, np.uint8)
    add("paeth_ties_8x8", pc.write_png(8, 8, 8, 0, ties, filters=(4,)))
    # palette: tRNS shorter than PLTE, indices past PLTE's end
    pal = bytes([200, 10, 10, 10, 200, 10, 10, 10, 200, 90, 90, 90, 250, 250, 5])
    idx = np.array([[0, 1, 2, 3, 4, 5, 9, 15], [4, 3, 2, 1, 0, 15, 7, 6]] * 3, np.uint8)
    add("pal4_short_trns_past_end", pc.write_png(8, 6, 4, 3, idx, filters=(0, 1), plte=pal, trns=bytes([0, 128, 255])))
    idx8 = np.array([[0, 1, 2, 3, 4, 5, 200, 255]] * 4, np.uint8)
    add("pal8_trns_past_end", pc.write_png(8, 4, 8, 3, idx8, filters=(2,), plte=pal, trns=bytes([255, 0])))
    add("pal8_one_transparent", pc.write_png(8, 4, 8, 3, idx8 % 5, filters=(0,), plte=pal, trns=bytes([255, 255, 0])))
    # colour keys
    g = content(6, 9, 1, 8, 90)
    add("gray8_key", pc.write_png(9, 6, 8, 0, g, filters=(1,), trns=bytes([0, int(g[2, 3])])))
    g4 = content(6, 9, 1, 4, 91)
    add("gray4_key", pc.write_png(9, 6, 4, 0, g4, filters=(0,), trns=bytes([0, int(g4[1, 1])])))
    g1 = ((np.mgrid[0:6, 0:9][0] + np.mgrid[0:6, 0:9][1] // 2) & 1).astype(np.uint8)
    add("gray1_key", pc.write_png(9, 6, 1, 0, g1, filters=(0,), trns=bytes([0, 1])))
    c = content(6, 9, 3, 8, 93)
    add("rgb_key", pc.write_png(9, 6, 8, 2, c, filters=(4,), trns=bytes([0, int(c[2, 9]), 0, int(c[2, 10]), 0, int(c[2, 11])])))
    # sizes and compressor settings
    rgb64 = content(64, 64, 3, 8, 100)
    add("rgb_64x64_fixed", pc.write_png(64, 64, 8, 2, rgb64, filters=(1, 4), zargs=dict(level=6, strategy=zlib.Z_FIXED)))
    add("rgb_64x64_rle", pc.write_png(64, 64, 8, 2, rgb64, filters=(2, 3), zargs=dict(level=6, strategy=zlib.Z_RLE)))
    add("rgb_64x64_huffman_only", pc.write_png(64, 64, 8, 2, rgb64, filters=(4,),
                                               zargs=dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY)))
    add("rgb_64x64_level9", pc.write_png(64, 64, 8, 2, rgb64, filters=(0,), zargs=dict(level=9)))
    add("rgb_150x150_level0", pc.write_png(150, 150, 8, 2, content(150, 150, 3, 8, 101), filters=(0,), zargs=dict(level=0)))
    add("rgba_113x111_cycle", pc.write_png(111, 113, 8, 6, content(113, 111, 4, 8, 102), filters=(0, 1, 2, 3, 4)))
    small = content(17, 13, 3, 8, 103)
    add("rgb_17x13_idat1", pc.write_png(13, 17, 8, 2, small, filters=(4, 1), splits=1))
    add("rgb_17x13_idat7", pc.write_png(13, 17, 8, 2, small, filters=(3,), splits=7))
    from PIL import Image
    face = content(112, 112, 3, 8, 104).reshape(112, 112, 3)
    buf = io.BytesIO()
    Image.fromarray(face).save(buf, "PNG")
    add("rgb_112x112_pillow", buf.getvalue())
    add("rgb_112x112_idat4096", pc.write_png(112, 112, 8, 2, face.reshape(112, 336), filters=(4, 2, 1), splits=4096))
    occ = content(128, 128, 4, 8, 105).reshape(128, 128, 4)
    yy, xx = np.mgrid[0:128, 0:128]
    hole = (xx - 64) ** 2 + (yy - 70) ** 2 > 40 ** 2
    occ[hole] = 0
    buf = io.BytesIO()
    Image.fromarray(occ, "RGBA").save(buf, "PNG", compress_level=9)
    add("rgba_128x128_occluder", buf.getvalue())
    add("gray_la_112x112_pillow", pc.write_png(112, 112, 8, 4, content(112, 112, 2, 8, 106), filters=(1, 3)))

    # ---- token-level streams
    def t_blocks(d):
        a = pattern(40, 1)
        d.fixed(a + [(20, 7)])
        d.stored(b"")
        d.stored(bytes(pattern(20, 2)))
        return pc.expand_tokens(a + [(20, 7)]) + bytes(pattern(20, 2))
    add(*token_image("tok_empty_stored_final_empty_fixed", t_blocks))

    def t_d1(d):
        toks = [3, (258, 1), 1, 2, (258, 1), (3, 2)]
        d.fixed(toks)
        return pc.expand_tokens(toks)
    add(*token_image("tok_d1_l258", t_d1))

    def t_far(d):
        toks = pattern(300, 3)
        n = 300

        def fill(to):
            nonlocal n
            while to - n >= 258 + 3:
                toks.append((258, 300))
                n += 258
            if to - n >= 3:
                toks.append((min(to - n, 258), 299))
                n += min(to - n, 258)
            while n < to:
                toks.append(2)
                n += 1
        fill(16384 - 100)
        toks.append((258, 1000))            # crosses the first flush (16384)
        n += 258
        fill(32768 - 7)
        toks.append((200, 32761))           # crosses the ring's wrap, at the largest distance available there
        n += 200
        fill(32768 + 4000)
        toks.append((258, 32768))           # the largest distance
        n += 258
        toks.append((130, 32767))
        n += 130
        fill(49152 - 3)
        toks.append((258, 32768))           # distance 32768 across a flush
        n += 258
        d.fixed(toks)
        return pc.expand_tokens(toks)
    add(*token_image("tok_dist32768_wrap_flush", t_far, row=256))

    def t_onebit(d):
        toks = pattern(12, 4) + [(30, 1), 4, (258, 1), 0, 1]
        lit = [0] * 286
        used = [0, 1, 2, 3, 4, 256] + [257 + pc.length_symbol(30), 257 + pc.length_symbol(258)]
        for s, l in zip(used, pc.flat_lengths(range(8), 8)):
            lit[s] = l
        d.dynamic(toks, lit, [1])
        return pc.expand_tokens(toks)
    add(*token_image("tok_dynamic_one_bit_distance", t_onebit))

    def t_15(d):
        toks = pattern(30, 5) + [(3, 1), (4, 2), (5, 3), (6, 4), (7, 5), (8, 6), (9, 7), (10, 8), (11, 9), (13, 10)] + pattern(9, 6)
        lit = [0] * 286
        order = [0, 1, 2, 3, 4, 256] + list(range(257, 267))
        for s, l in zip(order, list(range(1, 15)) + [15, 15]):
            lit[s] = l
        d.dynamic(toks, lit, pc.flat_lengths(range(10), 10))
        return pc.expand_tokens(toks)
    add(*token_image("tok_dynamic_15_bit_codes", t_15))

    def t_span(d):
        toks = pattern(25, 7) + [(12, 5), (40, 20), (258, 60), 1, 2, (100, 3)]
        lit = [0] * 286
        for s in [0, 1, 2, 3, 4, 256] + list(range(260, 286)):
            lit[s] = 5
        d.dynamic(toks, lit, [5] * 28 + [4] * 2)
        return pc.expand_tokens(toks)
    add(*token_image("tok_dynamic_repeat_spans", t_span))

    # ---- streams the parser refuses
    g = content(4, 4, 1, 8, 200)
    ok = pc.write_png(4, 4, 8, 0, g)
    import struct
    add("bad_16bit", pc.write_png(4, 4, 16, 0, filtered=bytes(4 * 9)))
    add("bad_adam7", pc.write_png(4, 4, 8, 0, g, interlace=1))
    add("bad_crc", ok[:40] + bytes([ok[40] ^ 1]) + ok[41:])
    add("bad_no_plte", pc.write_png(4, 4, 8, 3, g))
    add("bad_apng", pc.write_png(4, 4, 8, 0, g, extra=[(b"acTL", struct.pack(">II", 1, 0))]))
    add("bad_depth_pair", pc.write_png(4, 4, 4, 2, filtered=bytes(4 * 7)))
    add("bad_signature", b"\x89PNG\r\n\x1a\r" + ok[8:])
    return cases


def main():
    import PIL
    from PIL import Image
    cases = []
    for name, data in build_cases():
        d = png.parse_png(data)
        c = {"name": name, "data": data, "supported": d.status == 0, "status": d.status}
        if d.status == 0:
            im = Image.open(io.BytesIO(data))
            im.load()
            c["RGB"] = np.asarray(im.convert("RGB"))
            c["RGBA"] = np.asarray(im.convert("RGBA"))
            if d.colour_type in (0, 4):
                c["L"] = np.asarray(im.convert("L"))
            for ch, mode in pc.MODES.items():
                if mode in c:
                    mine = pc.decode_png(data, ch)
                    if not np.array_equal(mine, c[mode]):
                        bad = np.argwhere(mine != c[mode])[0]
                        raise SystemExit("%s: the restatement differs from Pillow's %s at %s: %s vs %s" %
                                         (name, mode, bad, mine[tuple(bad[:2])], c[mode][tuple(bad[:2])]))
        else:
            assert name.startswith("bad_"), (name, d.reason)
        cases.append(c)
    pc.save_golden(cases, {"pillow": PIL.__version__, "zlib": zlib.ZLIB_RUNTIME_VERSION})
    print("wrote", pc.GOLDEN, os.path.getsize(pc.GOLDEN), "bytes,", len(cases), "cases")

    # the corrupt streams: what the host check says about a selection of mutations of the small streams
    sup = [c for c in cases if c["supported"]]
    streams = [png.parse_png(c["data"]).zlib_stream() for c in sup]
    muts = pc.mutations(streams)
    with tempfile.TemporaryDirectory() as tmp:
        exe = pc.build_hostcheck(os.path.join(tmp, "hostcheck"), sanitize=pc.sanitizers_link(tmp))
        pc.write_hostcheck_input(os.path.join(tmp, "in.bin"), sup, muts)
        rc, err, clean, st = pc.run_hostcheck(exe, os.path.join(tmp, "in.bin"))
    assert rc == 0 and not err, err
    assert all(s == 0 and m == 1 for _, s, m in clean), [x for x in clean if x[1:] != (0, 1)]
    per, dumped = {}, []
    for m, s in zip(muts, st):
        if 0 < len(m[4]) <= 700 and per.get((m[0], s), 0) < 3:
            per[(m[0], s)] = per.get((m[0], s), 0) + 1
            dumped.append((m[0], m[1], m[2], m[3], s, m[4]))
    # filter bytes above 4 behind a valid zlib stream: zlib does not judge them, the unfilter pass does
    for i in (0, 5):
        d = png.parse_png(sup[i]["data"])
        raw = bytearray(zlib.decompress(streams[i]))
        raw[(d.row_bytes + 1) * (d.height - 1)] = 5 + i
        dumped.append(("filter", i, 0, 0, 10, zlib.compress(bytes(raw))))
    pc.save_corrupt(dumped)
    print("wrote", pc.CORRUPT, os.path.getsize(pc.CORRUPT), "bytes,", len(dumped), "streams, statuses",
          sorted({d[4] for d in dumped}))


if __name__ == "__main__":
    main()
