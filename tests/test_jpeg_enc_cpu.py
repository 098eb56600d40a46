"""CPU tests of the JPEG encoder's host side: the numpy restatement (tests/jpeg_enc_cases.py) against the bytes Pillow
recorded into tests/golden/g16_jpeg_enc.npz and against the installed Pillow, the quantisation tables and the header
builder of msml_amd/jpeg.py, RecordWriter against RecordFile, and csrc/jpeg_enc_core.h itself, run on the host under
the sanitizers by tools/jpeg_enc_hostcheck.cpp in a process of its own."""
import functools
import io
import os
import struct

import numpy as np
import pytest

from msml_amd import jpeg
from tests import jpeg_cases as J
from tests import jpeg_enc_cases as E


@functools.lru_cache(maxsize=None)
def golden():
    return E.load_golden()


@functools.lru_cache(maxsize=None)
def restated():
    return [E.encode(c["source"], c["sampling"], c["quality"], c["restart"]) for c in golden()[0]]


def test_fixture_is_small_and_complete():
    assert os.path.getsize(E.GOLDEN) < (1 << 20)
    cases = golden()[0]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) >= 170
    assert {c["sampling"] for c in cases} == set(jpeg.SAMPLINGS) and all(1 <= c["quality"] <= 100 for c in cases)
    for w, h in [(1, 1), (8, 8), (5, 2), (9, 1), (1, 7), (16, 8), (17, 23), (3, 40), (40, 3), (33, 17)]:
        for mode in E.MODES:
            assert sum(c["source"].shape[:2] == (h, w) and c["sampling"] == mode for c in cases) >= 4
    scans = [c["data"][jpeg.parse_jpeg(c["data"]).begin:] for c in cases]
    assert sum(b"\xff\x00" in s for s in scans) >= 1
    assert any(c["restart"] == 1 for c in cases) and any(c["restart"] == 3 for c in cases)
    assert sum(c["name"].startswith("uniform") and (c["sampling"], c["quality"], c["restart"]) == ("420", 75, 0)
               for c in cases) == 4


def test_restatement_equals_recorded_bytes():
    for c, data in zip(golden()[0], restated()):
        assert data == c["data"], c["name"]


def test_restatement_equals_installed_pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow is not built on libjpeg-turbo")
    sub = {"444": 0, "422": 1, "420": 2}
    for c, data in zip(golden()[0], restated()):
        im = Image.fromarray(c["source"])
        kw = {}
        if c["sampling"] == "gray":
            im = im.convert("L")
        else:
            kw["subsampling"] = sub[c["sampling"]]
        if c["restart"]:
            kw["restart_marker_blocks"] = c["restart"]
        f = io.BytesIO()
        im.save(f, "JPEG", quality=c["quality"], **kw)
        assert f.getvalue() == data, c["name"]
    f = io.BytesIO()
    Image.fromarray(golden()[0][-1]["source"]).save(f, "JPEG")           # a bare save(): quality 75, 4:2:0
    assert f.getvalue() == E.encode(golden()[0][-1]["source"])


def test_restatement_decodes_to_the_recorded_decode():
    for c, data in zip(golden()[0], restated()):
        px = J.decode(data)
        assert px.shape[:2] == c["source"].shape[:2] and (px.ndim == 2) == (c["sampling"] == "gray")
        assert np.array_equal(px, J.decode(c["data"])), c["name"]


def test_gray_source_equals_gray_sampling_of_rgb():
    c = next(c for c in golden()[0] if c["name"].startswith("17x23_gray_q75"))
    y = E.rgb_to_ycc(c["source"])[0].astype(np.uint8)
    assert E.encode(y, "gray", c["quality"], c["restart"]) == c["data"]


def test_quant_tables():
    """jpeg_set_quality(q, force_baseline=TRUE) at the ends and at the switch of the scale formula."""
    luma, chroma = jpeg.quant_tables(50)
    assert luma[:8].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and chroma[:4].tolist() == [17, 18, 24, 47]
    assert all((t == 1).all() for t in jpeg.quant_tables(100))
    luma, chroma = jpeg.quant_tables(1)                          # scale 5000: everything clamps to 255
    assert (luma == 255).all() and (chroma == 255).all()
    luma, _ = jpeg.quant_tables(49)                              # scale 5000 // 49 = 102
    assert luma[:4].tolist() == [(16 * 102 + 50) // 100, (11 * 102 + 50) // 100, (10 * 102 + 50) // 100, 16]
    for q in (30, 75, 95, 100):                                  # and what Pillow wrote into the fixture's DQT segments
        c = next(c for c in golden()[0] if c["quality"] == q and c["sampling"] == "420")
        d = jpeg.parse_jpeg(c["data"])
        assert all(np.array_equal(d.qtables[i], jpeg.quant_tables(q)[i]) for i in (0, 1))
    for bad in (0, 101):
        with pytest.raises(ValueError):
            jpeg.quant_tables(bad)


def test_header_builder():
    for c in golden()[0]:
        d = jpeg.parse_jpeg(c["data"])
        h, w = c["source"].shape[:2]
        hb = jpeg.build_header(h, w, c["sampling"], jpeg.quant_tables(c["quality"]), c["restart"])
        assert hb == c["data"][:d.begin], c["name"]
    hb = jpeg.build_header(16, 8, "gray", jpeg.quant_tables(75))
    assert hb[:20] == b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    marks = [hb[i + 1] for i in range(len(hb) - 1) if hb[i] == 0xFF and hb[i + 1] not in (0, 0xFF)]
    assert [m for m in marks if m in (0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA)][:7] == [0xD8, 0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDA]
    d = jpeg.parse_jpeg(jpeg.build_header(9, 300, "422", jpeg.quant_tables(30), 5) + b"\xff\xd9")
    assert (d.status, d.height, d.width, d.sampling[0], d.restart_interval) == (0, 9, 300, (2, 1), 5)
    assert {k: (list(c), bytes(s)) for k, (c, s) in d.huffman.items()} == \
        {k: (list(c), bytes(s)) for k, (c, s) in jpeg.STD_HUFFMAN.items()}


def test_encode_plan_without_gpu():
    """Descriptors, deduplicated tables and headers, bounds: host work, no launch."""
    plan = jpeg.EncodePlan([(112, 112), (112, 112), (17, 23)], [75, 75, 30], ["420", "420", "gray"], [0, 0, 3])
    d = plan.desc.numpy()
    assert d[:, jpeg.JE_SAMP].tolist() == [3, 3, 0] and d[:, jpeg.JE_RI].tolist() == [0, 0, 3]
    assert plan.qtabs.shape == (4, 64) and d[:, jpeg.JE_QT].tolist() == [0, 0, 2]
    assert d[0, jpeg.JE_HOFF] == d[1, jpeg.JE_HOFF] == 0 and d[2, jpeg.JE_HOFF] == d[0, jpeg.JE_HLEN]
    assert plan.ws_bytes > 0 and d[:, jpeg.JE_WS].tolist()[0] == 0 and d[1, jpeg.JE_WS] > 0
    # 4:2:0 at 112 x 112: 49 MCUs of 6 blocks, 208 bytes each, doubled; one interval; header and EOI
    assert plan.bounds[0] == (d[0, jpeg.JE_HLEN] + 2 * 294 * 208 + 2 + 2 + 3) & ~3
    for c, data in zip(golden()[0], restated()):
        h, w = c["source"].shape[:2]
        hlen = jpeg.parse_jpeg(data).begin
        assert len(data) <= jpeg.value("msml_jpeg_encode_bound", h, w, jpeg.SAMPLINGS[c["sampling"]], c["restart"], hlen)
    assert jpeg.value("msml_jpeg_encode_bound", 0, 8, 3, 0, 0) == 0 and jpeg.value("msml_jpeg_encode_bound", 8, 8, 4, 0, 0) == 0
    with pytest.raises(ValueError):
        jpeg.EncodePlan([(8, 8)], 75, "411")
    with pytest.raises(ValueError):
        jpeg.EncodePlan([(8, 8), (8, 8)], [75], "420")


def test_record_writer_round_trip(tmp_path):
    rec, idx = str(tmp_path / "train.rec"), str(tmp_path / "train.idx")
    bodies = [b"abc", b"12345678", golden()[0][-1]["data"], b""]
    with jpeg.RecordWriter(rec, idx) as w:
        w.write_idx(0, (0, [len(bodies), 7], 1, 0), b"")                        # record 0: (count + 1, classes)
        w.write_idx(1, (0, 3, 0, 0), bodies[0])                                   # 27 bytes: padded by one
        w.write_idx(2, (0, [4.0, 5.5, 6.0], 9, 10), bodies[1])                    # flag 3
        w.write_idx(3, jpeg.RecordWriter.pack((0, 5.0, 0, 0), bodies[2]))         # already packed
        with pytest.raises(ValueError, match="record 4"):
            w.write_idx(4, (0, 1, 0, 0), b"\x00" * 4 + struct.pack("<I", jpeg.RECORD_MAGIC))   # header 24 + 4: aligned
        w.write_idx(4, (0, 1, 0, 0), b"\x00" * 3 + struct.pack("<I", jpeg.RECORD_MAGIC))       # not aligned: written
        assert w.keys == [0, 1, 2, 3, 4]
    raw = open(rec, "rb").read()
    lines = open(idx).read().splitlines()
    assert lines[0] == "0\t0" and lines[1] == "1\t%d" % (8 + 24 + 8)
    # record 1, byte by byte: magic, length 27, IRHeader(0, 3.0, 0, 0), the payload, one byte of padding
    o = 8 + 24 + 8
    assert raw[o:o + 36] == struct.pack("<II", 0xCED7230A, 27) + struct.pack("<IfQQ", 0, 3.0, 0, 0) + b"abc" + b"\x00"
    assert len(raw) % 4 == 0
    with jpeg.RecordFile(rec, idx) as f:
        assert f.header0 == (len(bodies), 7) and f.img_idx.tolist() == [1, 2, 3]
        (flag, label, id1, id2), body = f.read_idx(1)
        assert (flag, label, id1, id2, body) == (0, 3.0, 0, 0, b"abc")
        (flag, label, id1, id2), body = f.read_idx(2)
        assert flag == 3 and label.tolist() == [4.0, 5.5, 6.0] and (id1, id2, body) == (9, 10, bodies[1])
        assert f.read_idx(3)[1] == bodies[2] and f.read_idx(3)[0][1] == 5.0
        assert f.read_idx(4)[1][3:] == struct.pack("<I", jpeg.RECORD_MAGIC)


def test_write_faces_from_byte_strings(tmp_path):
    """write_faces with streams already on the host (the EncodedBatch path runs in the GPU tests)."""
    streams = [c["data"] for c in golden()[0][-4:]]
    rec, idx = str(tmp_path / "train.rec"), str(tmp_path / "train.idx")
    with jpeg.RecordWriter(rec, idx) as w:
        assert jpeg.write_faces(w, streams[:2], [5, 6], 1, header0=(4, 10)) == 3
        assert jpeg.write_faces(w, streams[2:], np.array([7, 8]), 3) == 5
        with pytest.raises(ValueError):
            jpeg.write_faces(w, streams, [1], 5)
    with jpeg.RecordFile(rec, idx) as f:
        assert f.header0 == (5, 10) and f.img_idx.tolist() == [1, 2, 3, 4]
        assert [f.read_idx(i)[1] for i in range(1, 5)] == streams
        assert [f.read_idx(i)[0][1] for i in range(1, 5)] == [5.0, 6.0, 7.0, 8.0]


def test_enc_host_check_under_sanitizers(tmp_path):
    """tools/jpeg_enc_hostcheck.cpp with -fsanitize=address,undefined, its own process: csrc/jpeg_enc_core.h on the host,
    in the kernels' order, gives the fixture's streams byte for byte; 3 000 random sizes and option sets stay inside
    workspaces and slots of exactly their size, fit the bound, repeat, and refuse a slot one byte short and a source one
    byte short; nothing is reported."""
    if J.host_compiler() is None:
        pytest.skip("no host C++ compiler")
    cases = golden()[0]
    if not J.sanitizers_link(str(tmp_path)):
        pytest.skip("the host compiler cannot link a trivial program with -fsanitize=address,undefined")
    exe = E.build_hostcheck(str(tmp_path / "hostcheck"), sanitize=True)       # a failure to build THIS is a failure
    E.write_hostcheck_input(str(tmp_path / "in.bin"), cases)
    rc, out, err, streams = E.run_hostcheck(exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), len(cases))
    assert rc == 0 and err == "", err[-2000:]
    assert out.split() == ["R", str(E.HOSTCHECK_RANDOM), "0"]
    assert len(streams) == len(cases)
    for c, (st, data) in zip(cases, streams):
        assert st == 0 and data == c["data"], c["name"]
