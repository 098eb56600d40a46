"""CPU tests of the JPEG path (msml_amd/jpeg.py, csrc/jpeg_core.h): the numpy restatement tests/jpeg_cases.py against
the bytes Pillow (libjpeg-turbo) recorded in tests/golden/g15_jpeg.npz, the two upsampling edge rules in isolation, the
header parser, the RecordIO reader on a file written here, and the host check of the decoder's C++ under the
sanitizers (tools/jpeg_hostcheck.cpp, its own process)."""
import io
import os
import struct

import numpy as np
import pytest

from msml_amd import jpeg
from tests import jpeg_cases as J

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        _CACHE["g"] = J.load_golden()
    return _CACHE["g"]


def test_fixture_covers_sizes_samplings_and_qualities():
    cases, ver = golden()
    names = [c["name"] for c in cases]
    assert ver["pillow"] and ver["libjpeg_turbo"]
    for w, h in [(1, 1), (8, 8), (9, 1), (9, 2), (9, 3), (5, 2), (1, 7), (16, 16), (17, 23), (15, 33), (40, 3), (3, 40)]:
        for mode in ("444", "422", "420", "gray"):
            for q in (30, 75, 95, 100):
                assert any(n.startswith("%dx%d_%s_q%d_" % (w, h, mode, q)) for n in names)
    assert sum("112x112" in n for n in names) == 4
    sup = [c for c in cases if c["supported"]]
    ri = [jpeg.parse_jpeg(c["data"]).restart_interval > 0 for c in sup]
    assert 0.4 < np.mean(ri) < 0.6
    assert [c["name"] for c in cases if not c["supported"]] == ["progressive_16x16", "s411_32x16"]
    # a stuffed FF in entropy-coded data
    assert any(b"\xff\x00" in c["data"][jpeg.parse_jpeg(c["data"]).begin:] for c in sup)
    assert os.path.getsize(J.GOLDEN) < 1 << 20


def test_restatement_equals_pillow_recorded():
    cases, _ = golden()
    n = 0
    for c in cases:
        if c["supported"]:
            out = J.decode(c["data"])
            assert out.shape == c["pixels"].shape and np.array_equal(out, c["pixels"]), c["name"]
            n += 1
    assert n >= 200


def test_restatement_equals_installed_pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("the installed Pillow is not built on libjpeg-turbo")
    for c in golden()[0]:
        if c["supported"]:
            fresh = np.asarray(Image.open(io.BytesIO(c["data"])))
            assert np.array_equal(J.decode(c["data"]), fresh), c["name"]


def test_narrow_plane_rule():
    """dw <= 2: libjpeg replicates instead of filtering (h2v1 and h2v2)."""
    p = np.array([[10, 200]], np.uint8)
    assert J.upsample_h2v1(p).tolist() == [[10, 10, 200, 200]]
    assert J.upsample_h2v2(np.array([[10, 200], [50, 60]], np.uint8)).tolist() == \
        [[10, 10, 200, 200], [10, 10, 200, 200], [50, 50, 60, 60], [50, 50, 60, 60]]
    assert J.upsample_h2v1(np.array([[7]], np.uint8)).tolist() == [[7, 7]]
    # dw = 3 takes the filter: (3 * 10 + 200 + 2) >> 2 = 58 at output 1
    assert J.upsample_h2v1(np.array([[10, 200, 30]], np.uint8)).tolist() == \
        [[10, 58, (600 + 10 + 1) >> 2, (600 + 30 + 2) >> 2, (90 + 200 + 1) >> 2, 30]]
    # the fixture has such planes, and the whole decode follows the rule there
    cases = [c for c in golden()[0] if c["supported"] and c["name"].split("_")[0] in ("1x1", "1x7", "3x40", "5x2")
             and c["name"].split("_")[1] in ("422", "420")]
    assert len(cases) >= 16
    for c in cases:
        d = jpeg.parse_jpeg(c["data"])
        assert -(-d.width // 2) <= 3
        assert np.array_equal(J.decode(c["data"]), c["pixels"]), c["name"]


def test_vertical_edge_rule():
    """h2v2: row -1 counts as row 0 and row dh as row dh - 1; the first and last columns take (4 s + 8) >> 4, (4 s + 7) >> 4."""
    p = np.array([[0, 16, 32], [64, 80, 96], [128, 144, 255]], np.uint8)
    out = J.upsample_h2v2(p)
    assert out.shape == (6, 6)
    s_top = 3 * p[0].astype(int) + p[0]                 # output row 0: the neighbour above is row 0 itself
    assert out[0, 0] == (4 * s_top[0] + 8) >> 4 and out[0, 5] == (4 * s_top[2] + 7) >> 4
    assert out[0, 2] == (3 * s_top[1] + s_top[0] + 8) >> 4 and out[0, 3] == (3 * s_top[1] + s_top[2] + 7) >> 4
    s_bot = 3 * p[2].astype(int) + p[2]                 # output row 5: the neighbour below is row 2 itself
    assert out[5].tolist() == [(4 * s_bot[0] + 8) >> 4, (3 * s_bot[0] + s_bot[1] + 7) >> 4,
                               (3 * s_bot[1] + s_bot[0] + 8) >> 4, (3 * s_bot[1] + s_bot[2] + 7) >> 4,
                               (3 * s_bot[2] + s_bot[1] + 8) >> 4, (4 * s_bot[2] + 7) >> 4]
    s_mid = 3 * p[1].astype(int) + p[0]                 # output row 2 = 2 * 1 + 0: the neighbour is row 0
    assert out[2, 0] == (4 * s_mid[0] + 8) >> 4
    s_mid = 3 * p[1].astype(int) + p[2]                 # output row 3 = 2 * 1 + 1: the neighbour is row 2
    assert out[3, 5] == (4 * s_mid[2] + 7) >> 4
    # odd heights in the fixture end on a replicated row
    for c in golden()[0]:
        if c["name"].startswith(("9x3_420", "17x23_420", "15x33_420")):
            assert np.array_equal(J.decode(c["data"]), c["pixels"]), c["name"]


def test_parser_reads_every_field():
    by = {c["name"]: c for c in golden()[0]}
    d = jpeg.parse_jpeg(by["face0_112x112_420_q95_r3"]["data"])
    assert (d.status, d.height, d.width, d.components) == (0, 112, 112, 3)
    assert d.sampling == ((2, 2), (1, 1), (1, 1)) and d.qsel == (0, 1, 1) and d.dcsel == (0, 1, 1) and d.acsel == (0, 1, 1)
    assert d.restart_interval == 3 and d.end == len(by["face0_112x112_420_q95_r3"]["data"])
    data = by["face0_112x112_420_q95_r3"]["data"]
    sos = data.index(b"\xff\xda")
    assert d.begin == sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    assert sorted(d.qtables) == [0, 1] and all(q.shape == (64,) and q.min() >= 1 for q in d.qtables.values())
    assert sorted(d.huffman) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    d = jpeg.parse_jpeg(by["face2_112x112_422_q75_r3"]["data"])
    assert d.sampling == ((2, 1), (1, 1), (1, 1))
    d = jpeg.parse_jpeg(by["face1_112x112_444_q95_r0"]["data"])
    assert d.sampling == ((1, 1),) * 3 and d.restart_interval == 0
    d = jpeg.parse_jpeg(by["face3_112x112_gray_q95_r0"]["data"])
    assert d.components == 1 and d.sampling == ((1, 1),) and d.qsel == (0,)
    d = jpeg.parse_jpeg(by["mcu1_17x23_420_q75_r1"]["data"])
    assert (d.height, d.width, d.restart_interval) == (23, 17, 1)
    # 16-bit DQT: the same table as its 8-bit original would hold, in natural order
    d16 = jpeg.parse_jpeg(by["dqt16_17x23_422_q30_r0"]["data"])
    assert d16.status == 0 and b"\xff\xdb\x00\x83\x10" in by["dqt16_17x23_422_q30_r0"]["data"]
    assert d16.qtables[0][0] == by["dqt16_17x23_422_q30_r0"]["data"][
        by["dqt16_17x23_422_q30_r0"]["data"].index(b"\xff\xdb") + 6]
    # the natural order: entry 2 of the segment (zigzag) is row 1, column 0
    seg = data[data.index(b"\xff\xdb") + 5:]
    assert jpeg.parse_jpeg(data).qtables[0][8] == seg[2] and jpeg.parse_jpeg(data).qtables[0][1] == seg[1]


def test_parser_refuses_with_the_reason():
    by = {c["name"]: c for c in golden()[0]}
    assert jpeg.parse_jpeg(by["progressive_16x16"]["data"]).status == jpeg.PROGRESSIVE
    assert jpeg.parse_jpeg(by["s411_32x16"]["data"]).status == jpeg.SAMPLING
    good = bytearray(by["checker16x16_444_q75_r0"]["data"])
    sof = good.index(b"\xff\xc0")

    def patched(off, val, marker=None):
        b = bytearray(good)
        b[sof + off] = val
        if marker is not None:
            b[sof + 1] = marker
        return bytes(b)

    assert jpeg.parse_jpeg(patched(4, 12)).status == jpeg.PRECISION
    assert jpeg.parse_jpeg(patched(11, 0x12)).status == jpeg.SAMPLING          # 4:4:0
    assert jpeg.parse_jpeg(patched(4, 8, 0xC9)).status == jpeg.ARITHMETIC
    assert jpeg.parse_jpeg(patched(4, 8, 0xC1)).status == jpeg.FRAME
    assert jpeg.parse_jpeg(b"").status == jpeg.BAD_HEADER
    assert jpeg.parse_jpeg(b"\x89PNG\r\n\x1a\n").status == jpeg.BAD_HEADER
    assert jpeg.parse_jpeg(bytes(good[:sof + 6])).status == jpeg.BAD_HEADER    # cut inside a segment
    for n in range(0, len(good), 7):                                           # any cut ends in a verdict, never a guess
        d = jpeg.parse_jpeg(bytes(good[:n]))
        assert d.status != 0 or d.begin <= n
    dht = bytes(good).index(b"\xff\xc4")
    nodht = bytes(good[:dht]) + bytes(good[bytes(good).index(b"\xff\xda"):])
    assert jpeg.parse_jpeg(nodht).status == jpeg.TABLES
    assert all(jpeg.STATUS[s] for s in range(16, 27))


def test_parser_refuses_rgb_coded_components():
    """Three components are YCbCr only as libjpeg decides it: JFIF says so; without JFIF an Adobe segment with
    transform 0, or the ids 'R' 'G' 'B', mean RGB stored as it is -- refused, not converted."""
    by = {c["name"]: c for c in golden()[0]}
    good = by["checker16x16_444_q75_r0"]["data"]
    assert good[2:4] == b"\xff\xe0" and good[6:11] == b"JFIF\x00" and jpeg.parse_jpeg(good).status == 0
    app0_len = (good[4] << 8) | good[5]
    bare = good[:2] + good[4 + app0_len:]                                      # no JFIF marker
    assert jpeg.parse_jpeg(bare).status == 0                                   # ids 1, 2, 3: YCbCr

    def adobe(transform):
        return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])

    assert jpeg.parse_jpeg(bare[:2] + adobe(0) + bare[2:]).status == jpeg.COLORSPACE
    assert jpeg.parse_jpeg(bare[:2] + adobe(1) + bare[2:]).status == 0
    assert jpeg.parse_jpeg(good[:2] + adobe(0) + good[2:]).status == 0         # JFIF wins, as in libjpeg
    rgb = bytearray(bare)
    sof = rgb.index(b"\xff\xc0")
    sos = rgb.index(b"\xff\xda")
    for c, ident in enumerate(b"RGB"):
        rgb[sof + 10 + 3 * c] = ident
        rgb[sos + 5 + 2 * c] = ident
    assert jpeg.parse_jpeg(bytes(rgb)).status == jpeg.COLORSPACE
    gray = by["face3_112x112_gray_q95_r0"]["data"]
    assert jpeg.parse_jpeg(gray[:2] + adobe(0) + gray[2:]).status == 0         # one component: nothing to convert
    Image = pytest.importorskip("PIL.Image")                                   # libjpeg agrees: no conversion there
    plain = np.asarray(Image.open(io.BytesIO(bare)))
    asrgb = np.asarray(Image.open(io.BytesIO(bare[:2] + adobe(0) + bare[2:])))
    assert plain.shape == asrgb.shape and not np.array_equal(plain, asrgb)


def test_header_cache():
    cases = [c for c in golden()[0] if c["supported"]]
    cache = jpeg.HeaderCache(capacity=3)
    a = jpeg.pack_jpegs([c["data"] for c in cases], cache)
    b = jpeg.pack_jpegs([c["data"] for c in cases], cache)
    c = jpeg.pack_jpegs([c["data"] for c in cases])
    assert len(cache.headers) == 3 and cache.full > 0
    for x in (a, b):
        assert np.array_equal(x.desc.numpy(), c.desc.numpy()) and torch_equal(x.streams, c.streams)
        assert np.array_equal(x.qtabs.numpy(), c.qtabs.numpy()) and np.array_equal(x.htabs.numpy(), c.htabs.numpy())


def torch_equal(a, b):
    return np.array_equal(a.numpy(), b.numpy())


def test_pack_deduplicates_tables():
    cases = [c for c in golden()[0]]
    same = [c["data"] for c in cases if "_q95_" in c["name"] and "_gray_" not in c["name"] and c["supported"]]
    b = jpeg.pack_jpegs(same)
    assert len(b) == len(same) >= 30
    assert b.qtabs.shape == (2, 64) and b.htabs.shape == (4, jpeg.HUFF_WORDS)
    allb = jpeg.pack_jpegs([c["data"] for c in cases])
    nq = len({q.tobytes() for c in cases if c["supported"] for q in jpeg.parse_jpeg(c["data"]).qtables.values()})
    assert allb.qtabs.shape[0] == nq and allb.htabs.shape[0] == 4
    desc = allb.desc.numpy()
    for i, c in enumerate(cases):
        assert (desc[i, jpeg.JD_STATUS] == 0) == c["supported"]
        if c["supported"]:
            off = int(desc[i, jpeg.JD_BASE]) * 4
            assert allb.streams.numpy()[off:off + len(c["data"])].tobytes() == c["data"]
            d = allb.descriptors[i]
            for k in range(d.components):
                assert np.array_equal(allb.qtabs.numpy()[desc[i, jpeg.JD_QT + k]], d.qtables[d.qsel[k]])
    assert allb.ws_bytes > 0 and allb.ws_bytes % 256 == 0
    with pytest.raises(ValueError):
        jpeg.pack_jpegs([])


def test_huffman_lookup_form():
    d = jpeg.parse_jpeg(golden()[0][0]["data"])
    counts, symbols = d.huffman[(1, 0)]
    t = jpeg.huffman_lookup(counts, symbols)
    codes = J._codes(counts, symbols)
    for (ln, code), sym in codes.items():
        if ln <= 9:
            lo = code << (9 - ln)
            assert (t[lo:lo + (1 << (9 - ln))] == ((ln << 8) | sym)).all()
        else:
            assert code <= t[512 + ln] and t[547 + t[530 + ln] + code] == sym
    assert jpeg.huffman_lookup([3] + [0] * 15, bytes(3)) is None              # three codes of one bit


def test_record_file(tmp_path):
    cases = [c for c in golden()[0] if c["supported"]][:5]
    recs = [(0, 2, [6.0, 3.0], 0, 0, b"")]
    for k, c in enumerate(cases):
        key = 1 + k if k < 3 else 3 + k                              # keys 1, 2, 3, 6, 7: an index with gaps
        recs.append((key, 0, 10 + k, key, 0, c["data"]))
    assert any(len(r[5]) % 4 for r in recs[1:])                      # padded payloads
    rec, idx = J.write_records(tmp_path, recs)
    rf = jpeg.RecordFile(rec, idx)
    assert rf.header0 == (6, 3) and rf.img_idx.tolist() == [1, 2, 3, 4, 5]
    assert rf.keys == [0, 1, 2, 3, 6, 7]
    (flag, label, id1, id2), body = rf.read_idx(0)
    assert flag == 2 and label.tolist() == [6.0, 3.0] and body == b""
    for k, c in enumerate(cases):
        key = recs[1 + k][0]
        (flag, label, id1, _), body = rf.read_idx(key)
        assert flag == 0 and label == 10 + k and id1 == key and body == c["data"]
    with pytest.raises(KeyError):
        rf.read_idx(4)
    rf.close()
    # without the header-0 form the index range is the key list
    rec2, idx2 = J.write_records(tmp_path, recs[1:], "plain")
    assert jpeg.RecordFile(rec2, idx2).img_idx.tolist() == [1, 2, 3, 6, 7]
    # a continued record is refused, a bad magic too
    raw = bytearray(open(rec2, "rb").read())
    raw[7] |= 0x20
    open(rec2, "wb").write(raw)
    with pytest.raises(ValueError, match="unsupported"):
        jpeg.RecordFile(rec2, idx2).read_idx(1)
    raw[0] ^= 1
    open(rec2, "wb").write(raw)
    with pytest.raises(ValueError, match="magic"):
        jpeg.RecordFile(rec2, idx2).read_idx(1)


def test_record_face_source_batches(tmp_path):
    cases = [c for c in golden()[0] if "112x112" in c["name"] and "gray" not in c["name"]]
    recs = [(0, 2, [7.0, 5.0], 0, 0, b"")] + [(1 + k, 0, k % 5, 0, 0, cases[k % 3]["data"]) for k in range(6)]
    J.write_records(tmp_path, recs)
    src = jpeg.RecordFaceSource(str(tmp_path), 3, steps=2)
    items = list(src)
    assert len(items) == 2 and all(isinstance(b, jpeg.JpegBatch) and len(b) == 3 for b, _ in items)
    assert items[0][1].tolist() == [0, 1, 2] and items[1][1].tolist() == [3, 4, 0]
    assert items[1][0].sizes == [(112, 112)] * 3


def test_host_check_under_sanitizers(tmp_path):
    """tools/jpeg_hostcheck.cpp with -fsanitize=address,undefined, its own process: the clean streams decode to the
    fixture's pixels, every mutation ends in a status, nothing is reported, and the recorded corrupt fixture the GPU
    tests use is what this run dumps."""
    if J.host_compiler() is None:
        pytest.skip("no host C++ compiler")
    cases = golden()[0]
    if not J.sanitizers_link(str(tmp_path)):
        pytest.skip("the host compiler cannot link a trivial program with -fsanitize=address,undefined")
    exe = J.build_hostcheck(str(tmp_path / "hostcheck"), sanitize=True)      # a failure to build THIS is a failure
    J.write_hostcheck_input(str(tmp_path / "in.bin"), cases)
    rc, err, clean, muts, dumped = J.run_hostcheck(exe, str(tmp_path / "in.bin"))
    assert rc == 0 and err == "", err[-2000:]
    assert len(clean) == len(cases)
    for i, st, match in clean:
        if cases[i]["supported"]:
            assert (st, match) == (0, 1), cases[i]["name"]
        else:
            assert st >= 16
    assert len(muts) >= 2000
    kinds = {m[0] for m in muts}
    assert kinds == {"trunc", "ffxx", "subst", "cut", "rstdel", "rstswap"}
    assert all(0 <= m[4] <= 5 for m in muts)
    assert all(m[4] != 0 for m in muts if m[0] in ("rstdel", "rstswap"))
    trunc = [m for m in muts if m[0] == "trunc"]
    assert sum(m[4] != 0 for m in trunc) > 0.8 * len(trunc)           # the last bytes are the EOI and padding
    assert sum(m[4] != 0 for m in muts) > len(muts) // 3
    recorded = J.load_corrupt()
    assert [(d[0], d[1], d[2], d[3], d[4], d[5]) for d in dumped] == recorded
