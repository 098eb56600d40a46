"""CPU tests of the PNG path (msml_amd/png.py, csrc/png_core.h): what the fixture tests/golden/g17_png.npz covers, the
numpy / zlib restatement tests/png_cases.py against the arrays Pillow recorded and against the installed Pillow, the
chunk parser, pack_pngs, verification.list_folder, and the host check of the decoder's C++ under the sanitizers
(tools/png_hostcheck.cpp, its own process) with its statuses compared against the zlib acceptance rule."""
import io
import os
import struct
import zlib

import numpy as np
import pytest

from msml_amd import png, verification
from tests import png_cases as P

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        _CACHE["g"] = P.load_golden()
    return _CACHE["g"]


def supported():
    return [c for c in golden()[0] if c["supported"]]


def _filters(c):
    d = png.parse_png(c["data"])
    raw = zlib.decompress(d.zlib_stream())
    return d, [raw[y * (d.row_bytes + 1)] for y in range(d.height)]


def test_fixture_covers_what_the_decoder_can_get_wrong():
    cases, ver = golden()
    assert ver["pillow"] and ver["zlib"]
    assert os.path.getsize(P.GOLDEN) + os.path.getsize(P.CORRUPT) < 700 << 10
    sup = supported()
    by = {c["name"]: c for c in cases}
    parsed = {c["name"]: _filters(c) for c in sup}
    # every colour type and allowed depth, the sizes
    pairs = {(d.colour_type, d.depth) for d, _ in parsed.values()}
    assert pairs == {(0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8)}
    sizes = {(d.height, d.width) for d, _ in parsed.values()}
    assert {(1, 1), (1, 7), (7, 1), (3, 5), (17, 13), (64, 64), (112, 112), (113, 111), (150, 150), (128, 128)} <= sizes
    # every filter on every bpp, and on the first row; rows that cycle 0..4
    seen = {(max(1, d.bits_per_pixel // 8), f[0]) for d, f in parsed.values()}
    assert seen == {(b, ft) for b in (1, 2, 3, 4) for ft in range(5)}
    assert any(f[:5] == [0, 1, 2, 3, 4] for _, f in parsed.values())
    assert set(parsed["paeth_ties_8x8"][1]) == {4}
    d = parsed["pal4_short_trns_past_end"][0]
    assert len(d.trns) < len(d.plte) // 3
    idx = P.unfilter(zlib.decompress(d.zlib_stream()), d.height, d.row_bytes, 1)
    assert max(int(v) >> 4 for v in idx.reshape(-1)) >= len(d.plte) // 3
    for name in ("gray8_key", "gray4_key", "gray1_key", "rgb_key"):
        a = by[name]["RGBA"][..., 3]
        assert (a == 0).any() and (a == 255).any() and set(np.unique(a)) == {0, 255}, name
    # IDAT pieces of 1, 7 and 4096 bytes
    for name, size in (("rgb_17x13_idat1", 1), ("rgb_17x13_idat7", 7), ("rgb_112x112_idat4096", 4096)):
        pieces = [b - a for a, b in parsed[name][0].idat]
        assert len(pieces) > 1 and set(pieces[:-1]) == {size}
    # several stored blocks
    facts = {n: P.trace_inflate(parsed[n][0].zlib_stream())[1] for n in parsed if n.startswith("tok_") or "level0" in n
             or "occluder" in n or "fixed" in n or "pillow" in n}
    assert facts["rgb_150x150_level0"]["blocks"].count(0) >= 2
    assert set(facts["rgb_64x64_fixed"]["blocks"]) == {1}
    assert 2 in facts["rgb_112x112_pillow"]["blocks"]
    assert max(m[1] for m in facts["rgba_128x128_occluder"]["matches"]) == 258
    f = facts["tok_empty_stored_final_empty_fixed"]
    assert f["empty_stored"] and f["final_empty_fixed"] and f["blocks"] == [1, 0, 0, 1]
    assert facts["tok_d1_l258"]["d1_l258"]
    f = facts["tok_dist32768_wrap_flush"]
    assert f["max_dist"] == 32768
    assert any(p < 32768 < p + ln for p, ln, _ in f["matches"])           # a match across the ring's wrap
    assert any(p < 16384 < p + ln for p, ln, _ in f["matches"])           # and across a flush of a half
    assert any(p < 49152 < p + ln and dd == 32768 for p, ln, dd in f["matches"])
    assert facts["tok_dynamic_one_bit_distance"]["one_bit_dist"]
    assert facts["tok_dynamic_15_bit_codes"]["max_code"] == 15
    assert facts["tok_dynamic_repeat_spans"]["repeat_spans"]
    assert [c["name"] for c in cases if not c["supported"]] == [
        "bad_16bit", "bad_adam7", "bad_crc", "bad_no_plte", "bad_apng", "bad_depth_pair", "bad_signature"]


def test_restatement_equals_pillow_recorded():
    n = 0
    for c in supported():
        for ch, mode in P.MODES.items():
            if mode in c:
                out = P.decode_png(c["data"], ch)
                assert out.shape == c[mode].shape and np.array_equal(out, c[mode]), (c["name"], mode)
                n += 1
        assert ("L" in c) == (png.parse_png(c["data"]).colour_type in (0, 4))
    assert n >= 180


def test_restatement_equals_installed_pillow():
    Image = pytest.importorskip("PIL.Image")
    import warnings
    for c in supported():
        im = Image.open(io.BytesIO(c["data"]))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for ch, mode in P.MODES.items():
                if mode in c:
                    assert np.array_equal(np.asarray(im.convert(mode)), P.decode_png(c["data"], ch)), (c["name"], mode)


def test_python_inflate_equals_zlib():
    for c in supported():
        z = png.parse_png(c["data"]).zlib_stream()
        assert P.trace_inflate(z)[0] == zlib.decompress(z), c["name"]


def test_parser_reads_every_field():
    pal = bytes(range(30))
    data = P.write_png(5, 3, 4, 3, np.zeros((3, 5), np.uint8), plte=pal, trns=b"\x01\x02", splits=3,
                       extra=[(b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"k\x00v")])
    d = png.parse_png(data)
    assert (d.status, d.width, d.height, d.depth, d.colour_type) == (0, 5, 3, 4, 3)
    assert d.plte == pal and d.trns == b"\x01\x02" and d.reason == "ok"
    assert d.row_bytes == 3 and d.expected == 12 and d.bits_per_pixel == 4
    assert b"".join(data[a:b] for a, b in d.idat) == d.zlib_stream() and len(d.idat) > 1
    assert zlib.decompress(d.zlib_stream()) == bytes(12)
    p = d.palette()
    assert p.shape == (256, 4) and p[:10, :3].tobytes() == pal and list(p[:3, 3]) == [1, 2, 255]
    assert (p[10:] == np.array([0, 0, 0, 255], np.uint8)).all()
    assert png.parse_png(P.write_png(2, 2, 8, 0, np.zeros((2, 2), np.uint8), trns=b"\x00\x07")).key() == (7,)
    assert png.parse_png(P.write_png(2, 2, 2, 0, np.zeros((2, 2), np.uint8), trns=b"\x00\x07")).key() == (3,)


def test_parser_refuses_with_a_reason():
    cases = {c["name"]: c for c in golden()[0]}
    want = {"bad_16bit": png.SIXTEEN_BIT, "bad_adam7": png.INTERLACE, "bad_crc": png.BAD_CRC, "bad_no_plte": png.NO_PLTE,
            "bad_apng": png.APNG, "bad_depth_pair": png.COLOUR, "bad_signature": png.BAD_HEADER}
    for name, st in want.items():
        d = png.parse_png(cases[name]["data"])
        assert d.status == st == cases[name]["status"] and d.reason == png.STATUS[st] and png.reason(st) == d.reason
    assert len(set(png.STATUS.values())) == len(png.STATUS) and min(want.values()) >= 16
    g = np.zeros((2, 2), np.uint8)
    ok = P.write_png(2, 2, 8, 0, g)
    assert png.parse_png(ok).status == 0

    def ihdr(w, h, dp, ct, comp=0, filt=0, lace=0, ln=13):
        body = struct.pack(">IIBBBBB", w, h, dp, ct, comp, filt, lace)[:ln] + bytes(max(0, ln - 13))
        return png.SIGNATURE + P.chunk(b"IHDR", body) + ok[33:]
    assert png.parse_png(ihdr(2, 2, 8, 0)).status == 0
    assert png.parse_png(ihdr(0, 2, 8, 0)).status == png.SIZE
    assert png.parse_png(ihdr(2, 32768, 8, 0)).status == png.SIZE
    assert png.parse_png(ihdr(2, 2, 8, 0, comp=1)).status == png.METHOD
    assert png.parse_png(ihdr(2, 2, 8, 0, filt=1)).status == png.METHOD
    assert png.parse_png(ihdr(2, 2, 8, 0, lace=1)).status == png.INTERLACE
    assert png.parse_png(ihdr(2, 2, 3, 0)).status == png.COLOUR
    assert png.parse_png(ihdr(2, 2, 8, 5)).status == png.COLOUR
    assert png.parse_png(ihdr(2, 2, 16, 6)).status == png.SIXTEEN_BIT
    assert png.parse_png(ihdr(2, 2, 8, 0, ln=14)).status == png.BAD_HEADER
    head, idat, iend = ok[:33], P.chunk(b"IDAT", zlib.compress(bytes(6))), P.chunk(b"IEND", b"")
    assert png.parse_png(head + idat + iend).status == 0
    assert png.parse_png(head + P.chunk(b"IDAT", b"") + iend).status == png.NO_IDAT
    assert png.parse_png(head + iend).status == png.NO_IDAT
    assert png.parse_png(head + idat).status == png.BAD_HEADER                       # no IEND
    assert png.parse_png(idat + head + iend).status == png.BAD_HEADER
    assert png.parse_png(head + idat + P.chunk(b"tEXt", b"a\x00b") + idat + iend).status == png.BAD_HEADER
    assert png.parse_png(head + idat + P.chunk(b"PLTE", bytes(3)) + iend).status == png.BAD_HEADER
    assert png.parse_png(ok[:-3]).status == png.BAD_HEADER
    assert png.parse_png(b"").status == png.BAD_HEADER and png.parse_png(b"\xff\xd8\xff").status == png.BAD_HEADER
    for cut in range(len(ok)):                               # never raises
        png.parse_png(ok[:cut])


def test_pack_concatenates_idats_and_dedups_palettes():
    cases = {c["name"]: c for c in supported()}
    names = ["rgb_17x13_idat1", "pal4_short_trns_past_end", "bad_crc", "pal8_trns_past_end", "pal4_short_trns_past_end",
             "ct3_d8_17x13_cycle"]
    allc = {c["name"]: c for c in golden()[0]}
    batch = png.pack_pngs([allc[n]["data"] for n in names])
    desc = batch.desc.numpy()
    flat = batch.streams.numpy()
    assert list(batch.status) == [0, 0, png.BAD_CRC, 0, 0, 0] and len(batch) == 6
    for i, n in enumerate(names):
        if desc[i, png.PD_STATUS] == 0:
            z = png.parse_png(allc[n]["data"]).zlib_stream()
            o = int(desc[i, png.PD_BASE]) * 4
            assert flat[o:o + desc[i, png.PD_END]].tobytes() == z and len(z) == desc[i, png.PD_END]
    assert len(png.parse_png(cases["rgb_17x13_idat1"]["data"]).idat) == desc[0, png.PD_END]
    # the two pal4 streams share a palette; pal8_trns_past_end has the same PLTE but another tRNS
    assert batch.palettes.shape == (3, 256, 4)
    assert desc[1, png.PD_PAL] == desc[4, png.PD_PAL] != desc[3, png.PD_PAL] and desc[0, png.PD_PAL] == -1
    assert batch.ws_bytes > 0 and batch.ws_bytes % 256 == 0
    assert list(np.diff(desc[[0, 1, 3, 4, 5], png.PD_WS]) > 0) == [True] * 4
    with pytest.raises(ValueError):
        png.pack_pngs([])


def test_list_folder_follows_the_order_rules(tmp_path):
    for ident, files in (("b_id", ["0002.png", "0001.jpg", "0010.png"]), ("a_id", ["z.png", "a.png"]), ("empty", [])):
        (tmp_path / ident).mkdir()
        for f in files:
            (tmp_path / ident / f).write_bytes(b"x")
    (tmp_path / "pairs.txt").write_text("a_id 1 2\n")
    (tmp_path / "b_id" / "sub").mkdir()
    files = verification.list_folder(str(tmp_path))
    assert files == {"a_id": ["a.png", "z.png"], "b_id": ["0001.jpg", "0002.png", "0010.png"], "empty": []}
    assert verification.pairs_file_order(files) == [("a_id", "a.png"), ("a_id", "z.png"), ("b_id", "0001.jpg"),
                                                    ("b_id", "0002.png"), ("b_id", "0010.png")]
    pairs, same = verification.read_pairs_txt(["a_id 1 2", "a_id 2 b_id 3"], files)
    assert pairs.tolist() == [[0, 1], [1, 4]] and same.tolist() == [True, False]


def test_host_check_under_sanitizers(tmp_path):
    """The C++ of csrc/png_core.h, compiled for the host with ASan + UBSan: the clean streams give the fixture's
    pixels; every one of >= 3000 mutated zlib streams ends in a status with no sanitizer report, and the status is 0
    exactly when the zlib rule accepts the stream.  Left out of that comparison (counted, <= 2 %): a stream zlib
    accepts whose damage fell into a filter byte (status 10), which zlib does not judge."""
    if P.host_compiler() is None or not P.sanitizers_link(str(tmp_path)):
        pytest.skip("no host compiler that links the sanitizers")
    sup = supported()
    streams = [png.parse_png(c["data"]).zlib_stream() for c in sup]
    muts = P.mutations(streams)
    assert len(muts) >= 3000 and {m[0] for m in muts} == {"trunc", "subst", "hdrbit", "splice", "trailer"}
    exe = P.build_hostcheck(str(tmp_path / "hostcheck"))
    P.write_hostcheck_input(str(tmp_path / "in.bin"), sup, muts)
    rc, err, clean, st = P.run_hostcheck(exe, str(tmp_path / "in.bin"))
    assert rc == 0 and err == "", err[-2000:]
    assert len(clean) == len(sup) and all(s == 0 and m == 1 for _, s, m in clean), [c for c in clean if c[1:] != (0, 1)]
    assert len(st) == len(muts)
    left_out, accepted = 0, 0
    for m, s in zip(muts, st):
        d = png.parse_png(sup[m[1]]["data"])
        assert s in png.STATUS and 0 <= s <= 10, (m[:4], s)
        ok = P.zlib_accepts(m[4], d.expected)
        if ok and s == png.STATUS_FILTER:
            left_out += 1
            continue
        assert (s == 0) == ok, (m[:4], s, ok)
        accepted += ok
    assert left_out <= 0.02 * len(muts), (left_out, len(muts))
    assert accepted > 0                                       # some mutations do leave a valid stream
    # the recorded corrupt streams carry the statuses this program prints
    rec = P.load_corrupt()
    by = {(m[0], m[1], m[2], m[3]): s for m, s in zip(muts, st)}
    for kind, i, a, b, s, z in rec:
        if kind != "filter":
            assert by[(kind, i, a, b)] == s
    assert {r[4] for r in rec} >= set(range(1, 11))
