"""CPU tests of progressive JPEG decoding (msml_amd/jpeg.py progressive=True, csrc/jpeg_prog_core.h): the Python
restatement tests/jpeg_prog_cases.py against the pixels Pillow (libjpeg-turbo) recorded in
tests/golden/g18_jpeg_prog.npz, the writer's streams against Pillow, the multi-scan parser and its refusals, the scan
table pack_jpegs writes, the events the fixture must contain, and the host check of the decoder's C++ under the
sanitizers (tools/jpeg_prog_hostcheck.cpp, its own process)."""
import collections
import io
import os

import numpy as np
import pytest

from msml_amd import jpeg
from tests import jpeg_cases as J
from tests import jpeg_prog_cases as P

_CACHE = {}


def golden():
    if "g" not in _CACHE:
        _CACHE["g"] = P.load_golden()
    return _CACHE["g"]


def restated():
    """Every fixture stream through the restatement, once: ([pixels], events)."""
    if "r" not in _CACHE:
        ev = collections.Counter()
        _CACHE["r"] = ([P.decode(c["data"], ev) for c in golden()[0]], ev)
    return _CACHE["r"]


def test_fixture_covers_sizes_samplings_scripts():
    cases, ver = golden()
    names = [c["name"] for c in cases]
    assert ver["pillow"] and ver["libjpeg_turbo"]
    for w, h in [(1, 1), (9, 1), (5, 2), (16, 16), (17, 23), (23, 17), (33, 47)]:
        for mode in ("444", "422", "420", "gray"):
            assert any(n.startswith("%dx%d_%s_q" % (w, h, mode)) for n in names)
    pil = [c for c in cases if not c["name"].startswith("w_")]
    assert {n.split("_")[-2] for n in names if not n.startswith("w_")} == {"q30", "q75", "q95"}
    assert {n.split("_")[-1] for n in names if not n.startswith("w_")} == {"r0", "r1", "r2"}
    ri = [[s.restart_interval for s in jpeg.parse_jpeg(c["data"], True).scans] for c in pil]
    assert any(len(set(r)) > 1 for r in ri) and any(set(r) == {0} for r in ri)   # the interval changes between scans
    assert sum("112x112" in n for n in names) == 4
    for kind in ("dc1", "spectral", "deep", "skew", "reorder", "eobs"):
        assert any(n.startswith("w_" + kind) for n in names), kind
    assert all(c["base"] for c in cases if c["name"].startswith("w_"))
    assert os.path.getsize(P.GOLDEN) < 1 << 20 and os.path.getsize(P.CORRUPT) < 1 << 20


def test_restatement_equals_pillow_recorded():
    cases, _ = golden()
    outs, _ = restated()
    assert len(cases) >= 50
    for c, out in zip(cases, outs):
        assert out.shape == c["pixels"].shape and np.array_equal(out, c["pixels"]), c["name"]


def test_restatement_equals_installed_pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("the installed Pillow is not built on libjpeg-turbo")
    for c, out in zip(golden()[0], restated()[0]):
        assert np.array_equal(out, np.asarray(Image.open(io.BytesIO(c["data"])))), c["name"]


def test_writer_streams_decode_in_pillow_as_their_baseline():
    Image = pytest.importorskip("PIL.Image")
    made = [c for c in golden()[0] if c["name"].startswith("w_")]
    assert len(made) >= 20
    for c in made:
        assert jpeg.parse_jpeg(c["base"]).status == 0 and not jpeg.parse_jpeg(c["base"], True).scans
        want = np.asarray(Image.open(io.BytesIO(c["base"])))
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(c["data"]))), want), c["name"]
        assert np.array_equal(c["pixels"], want), c["name"]
    # the writer, run again here on a stream's coefficients, gives back the recorded bytes of one case
    by = {c["name"]: c for c in golden()[0]}
    name = next(n for n in by if n.startswith("w_spectral_17x23_420"))
    coefs, d = P.coefficients(by[name[len("w_spectral_"):]]["data"])
    script = [((0, 1, 2), 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in range(3) for a, b in ((1, 5), (6, 20), (21, 63))]
    assert P.write_progressive(coefs, d, script) == by[name]["data"]
    assert P.write_baseline(coefs, d) == by[name]["base"]


def test_parser_reads_every_scan_field():
    by = {c["name"]: c for c in golden()[0]}
    data = by["face0_112x112_420_q95_r1"]["data"]
    d = jpeg.parse_jpeg(data, progressive=True)
    assert (d.status, d.progressive, d.height, d.width, d.components) == (0, True, 112, 112, 3)
    assert d.sampling == ((2, 2), (1, 1), (1, 1)) and d.qsel == (0, 1, 1)
    assert [(s.components, s.ss, s.se, s.ah, s.al) for s in d.scans] == P.PILLOW_SCRIPT_3
    assert d.begin == d.scans[0].begin and d.end == len(data)
    at = 0
    for s in d.scans:
        sos = data.index(b"\xff\xda", at)
        assert s.begin == sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
        assert data[s.end] == 0xFF and data[s.end + 1] in (0xC4, 0xDD, 0xD9, 0xDA) and s.end > s.begin
        at = s.end
        assert len(s.tables) == len(s.components)
        assert all((t is None) == (s.ss == 0 and s.ah != 0) for t in s.tables)
    # restart_marker_blocks=3 counts MCUs in the interleaved DC scans and blocks in the one-component AC scans
    assert {s.restart_interval for s in d.scans} == {3}
    rows = jpeg.parse_jpeg(by["face2_112x112_422_q75_r2"]["data"], True)
    assert {s.restart_interval for s in rows.scans if len(s.components) == 3} == {7}
    assert {(s.components, s.restart_interval) for s in rows.scans if len(s.components) == 1} == {((0,), 14), ((1,), 7), ((2,), 7)}
    # tables are rewritten under the same ids before every scan: the scan holds the table as it stood at its SOS
    acs = [s for s in d.scans if s.ss and s.components == (0,)]
    assert len({s.acsel for s in acs}) == 1 and len({(bytes(s.tables[0][0]), s.tables[0][1]) for s in acs}) > 1
    g = jpeg.parse_jpeg(by["face3_112x112_gray_q95_r0"]["data"], True)
    assert g.components == 1 and all(s.components == (0,) for s in g.scans) and g.status == 0
    w = jpeg.parse_jpeg(by[next(n for n in by if n.startswith("w_dc1_17x23_420"))]["data"], True)
    assert [(s.components, s.ss, s.se) for s in w.scans] == [((c,), 0, 0) for c in range(3)] + [((c,), 1, 63) for c in range(3)]
    # a baseline stream reads as before under the keyword
    b = jpeg.parse_jpeg(by[next(n for n in by if n.startswith("w_dc1_17x23_420"))]["base"], True)
    assert b.status == 0 and b.scans == [] and not b.progressive


def test_default_keeps_status_17():
    for c in golden()[0]:
        assert jpeg.parse_jpeg(c["data"]).status == jpeg.PROGRESSIVE == 17
        assert jpeg.parse_jpeg(c["data"], progressive=False).status == 17
    b = jpeg.pack_jpegs([c["data"] for c in golden()[0][:4]])
    assert (b.status == 17).all() and b.scans is None and b.ws_bytes == 0
    assert jpeg.STATUS[jpeg.PROGRESSION] and jpeg.STATUS[jpeg.INCOMPLETE] and (jpeg.PROGRESSION, jpeg.INCOMPLETE) == (27, 28)


def _sos_patch(data, scan, off, val):
    """The stream with byte `off` (from the end of scan `scan`'s SOS segment, negative) set to val."""
    d = jpeg.parse_jpeg(data, True)
    b = bytearray(data)
    b[d.scans[scan].begin + off] = val
    return bytes(b)


def test_parser_refuses_invalid_and_incomplete_progressions():
    by = {c["name"]: c for c in golden()[0]}
    data = by[next(n for n in by if n.startswith("17x23_420_"))]["data"]
    head, ch = P.split_scans(data)
    assert len(ch) == 10 and P.join_scans(head, ch) == data
    st = lambda s: jpeg.parse_jpeg(s, progressive=True).status                       # noqa: E731
    assert st(data) == 0
    # incomplete: the last scan dropped, an AC band never sent, the last refinements missing, the file cut
    assert st(P.join_scans(head, ch[:-1])) == jpeg.INCOMPLETE
    assert st(P.join_scans(head, ch[:4] + ch[5:6] + ch[6:7])) == jpeg.PROGRESSION        # 6..63 never sent, then refined
    assert st(P.join_scans(head, ch[:4])) == jpeg.INCOMPLETE                             # luma 6..63 never sent
    assert st(P.join_scans(head, ch[:6])) == jpeg.INCOMPLETE
    d = jpeg.parse_jpeg(data, True)
    for s in d.scans[1:]:
        assert st(data[:s.begin - 3]) == jpeg.INCOMPLETE
        # a cut inside the last scan leaves the headers complete: the device finds the end of the data (status 5)
        assert st(data[:(s.begin + s.end) // 2]) == (0 if s is d.scans[-1] else jpeg.INCOMPLETE)
    assert st(data[:d.scans[0].begin - 3]) == jpeg.BAD_HEADER
    assert st(data[:-2]) == 0                                                            # no EOI: as baseline takes it
    # invalid: a refinement skipped, a refinement before its first scan, a scan sent twice, AC before DC
    assert st(P.join_scans(head, ch[:5] + ch[6:])) == jpeg.PROGRESSION
    assert st(P.join_scans(head, ch[:1] + ch[5:])) == jpeg.PROGRESSION
    assert st(P.join_scans(head, ch[:2] + ch[1:])) == jpeg.PROGRESSION
    assert st(P.join_scans(head, ch[1:])) == jpeg.PROGRESSION
    # reordered independent scans are fine
    assert st(P.join_scans(head, [ch[i] for i in (0, 3, 2, 1, 4, 5, 6, 9, 8, 7)])) == 0
    # scan parameters: Ss = 0 with Se != 0, Ss > Se, Se > 63, Al > 13, Al != Ah - 1, an interleaved AC scan
    assert st(_sos_patch(data, 0, -2, 5)) == jpeg.PROGRESSION
    assert st(_sos_patch(data, 1, -3, 9)) == jpeg.PROGRESSION
    assert st(_sos_patch(data, 4, -2, 64)) == jpeg.PROGRESSION
    assert st(_sos_patch(data, 0, -1, 0x0E)) == jpeg.PROGRESSION
    assert st(_sos_patch(data, 5, -1, 0x20)) == jpeg.PROGRESSION
    assert st(_sos_patch(data, 0, -3, 1)) == jpeg.PROGRESSION
    # components: not of the frame, repeated / out of frame order
    assert st(_sos_patch(data, 1, -5, 9)) == jpeg.PROGRESSION
    assert st(_sos_patch(data, 0, -7, 3)) == jpeg.PROGRESSION
    # a selected table that is missing
    assert st(_sos_patch(data, 1, -4, 0x03)) == jpeg.TABLES
    # the frame's own refusals keep their statuses
    sof = data.index(b"\xff\xc2")
    b = bytearray(data)
    b[sof + 4] = 12
    assert st(bytes(b)) == jpeg.PRECISION
    b = bytearray(data)
    b[sof + 11] = 0x41
    assert st(bytes(b)) == jpeg.SAMPLING
    b = bytearray(data)
    b[sof + 1] = 0xCA
    assert st(bytes(b)) == jpeg.ARITHMETIC


def test_parser_ends_in_a_verdict_for_mutated_headers():
    """Seeded byte flips anywhere in a small stream, and every cut: a status, never an exception; a supported verdict
    only with scans inside the data."""
    by = {c["name"]: c for c in golden()[0]}
    data = by[next(n for n in by if n.startswith("9x1_420_"))]["data"]
    rng = np.random.RandomState(18)
    for k in range(1500):
        b = bytearray(data)
        for _ in range(1 + k % 3):
            b[rng.randint(len(b))] = rng.randint(256)
        d = jpeg.parse_jpeg(bytes(b), progressive=True)
        assert d.status in jpeg.STATUS
        if d.status == 0:
            assert all(0 <= s.begin <= s.end <= len(b) for s in d.scans)
            assert all(p.end <= q.begin for p, q in zip(d.scans, d.scans[1:]))
    for n in range(len(data)):
        assert jpeg.parse_jpeg(data[:n], progressive=True).status in jpeg.STATUS


def test_pack_writes_the_scan_table_and_deduplicates():
    cases = golden()[0]
    c = next(c for c in cases if c["name"].startswith("17x23_420_"))
    base = next(c for c in cases if c["name"].startswith("w_dc1_17x23_420"))["base"]
    one = jpeg.pack_jpegs([c["data"]], progressive=True)
    d = one.descriptors[0]
    distinct = {(bytes(t[0]), bytes(t[1])) for s in d.scans for t in s.tables if t is not None}
    assert one.htabs.shape == (len(distinct), jpeg.HUFF_WORDS) and one.scans.shape == (10, jpeg.SCAN_WORDS)
    three = jpeg.pack_jpegs([c["data"], base, c["data"]], progressive=True)
    nb = len({(bytes(t[0]), bytes(t[1])) for t in jpeg.parse_jpeg(base).huffman.values()})
    assert three.htabs.shape[0] == len(distinct) + nb and three.qtabs.shape[0] == 2
    dn, sn = three.desc.numpy(), three.scans.numpy()
    assert dn[:, jpeg.JD_NSCAN].tolist() == [10, 0, 10] and dn[:, jpeg.JD_SCAN0].tolist() == [0, 0, 10]
    assert np.array_equal(sn[:10], sn[10:]) and (dn[:, 24:] == 0).all()
    for r, s in zip(sn[:10], d.scans):
        assert (r[jpeg.JS_BEGIN], r[jpeg.JS_END], r[jpeg.JS_NCOMP]) == (s.begin, s.end, len(s.components))
        assert (r[jpeg.JS_SS], r[jpeg.JS_SE], r[jpeg.JS_AH], r[jpeg.JS_AL], r[jpeg.JS_RI]) == (s.ss, s.se, s.ah, s.al, s.restart_interval)
        for k, (comp, t) in enumerate(zip(s.components, s.tables)):
            assert r[jpeg.JS_COMP + k] == comp
            if t is not None:
                assert np.array_equal(three.htabs.numpy()[r[jpeg.JS_TAB + k]], jpeg.huffman_lookup(*t))
    # the workspace is the baseline one of the same frame
    assert three.ws_bytes == 3 * jpeg.pack_jpegs([base]).ws_bytes
    # a batch without progressive streams carries no table and takes the baseline entry
    assert jpeg.pack_jpegs([base], progressive=True).scans is None


def test_header_cache_and_record_source_pass_progressive_streams(tmp_path):
    cases = golden()[0]
    faces = [c for c in cases if "112x112" in c["name"] and "gray" not in c["name"]]
    base = next(c for c in cases if c["name"].startswith("w_dc1_17x23_420"))["base"]
    cache = jpeg.HeaderCache()
    a = jpeg.pack_jpegs([faces[0]["data"], base, faces[0]["data"], base], cache, progressive=True)
    b = jpeg.pack_jpegs([faces[0]["data"], base, faces[0]["data"], base], progressive=True)
    assert len(cache.headers) == 1 and np.array_equal(a.desc.numpy(), b.desc.numpy())
    assert np.array_equal(a.scans.numpy(), b.scans.numpy())
    assert (jpeg.pack_jpegs([faces[0]["data"]], cache).status == 17).all()
    recs = [(0, 2, [7.0, 5.0], 0, 0, b"")] + [(1 + k, 0, k % 5, 0, 0, faces[k % 3]["data"]) for k in range(6)]
    J.write_records(tmp_path, recs)
    items = list(jpeg.RecordFaceSource(str(tmp_path), 3, steps=2, progressive=True))
    assert all((b.status == 0).all() and b.scans.shape[0] == 30 for b, _ in items)
    items = list(jpeg.RecordFaceSource(str(tmp_path), 3, steps=1))
    assert (items[0][0].status == 17).all()


def test_fixture_runs_the_hard_paths():
    """A condition on the fixture: every event the restatement counts occurs, so a green run means those paths ran."""
    _, ev = restated()
    for name in P.EVENTS:
        assert ev[name] > 0, name
    assert ev["eob14"] >= 1


def test_host_check_under_sanitizers(tmp_path):
    """tools/jpeg_prog_hostcheck.cpp with -fsanitize=address,undefined, its own process: the clean streams decode to the
    fixture's pixels, every mutation ends in a status, nothing is reported, and the recorded corrupt fixture the GPU
    tests use is what this run dumps."""
    if J.host_compiler() is None:
        pytest.skip("no host C++ compiler")
    cases = golden()[0]
    if not J.sanitizers_link(str(tmp_path)):
        pytest.skip("the host compiler cannot link a trivial program with -fsanitize=address,undefined")
    exe = P.build_hostcheck(str(tmp_path / "hostcheck"), sanitize=True)      # a failure to build THIS is a failure
    P.write_hostcheck_input(str(tmp_path / "in.bin"), cases)
    rc, err, clean, muts, dumped = P.run_hostcheck(exe, str(tmp_path / "in.bin"))
    assert rc == 0 and err == "", err[-2000:]
    assert [(i, st, m) for i, st, m in clean] == [(i, 0, 1) for i in range(len(cases))]
    assert len(muts) >= 3000
    assert {m[0] for m in muts} == {"subst", "ffxx", "trunc", "drop", "swap", "seltab", "scanhdr"}
    assert all(-1 <= m[4] <= 5 for m in muts)
    assert sum(m[4] > 0 for m in muts) > len(muts) // 4
    assert any(m[4] == -1 for m in muts if m[0] == "seltab") and {m[4] for m in muts} >= {-1, 0, 1, 2, 3, 5}
    trunc = [m for m in muts if m[0] == "trunc"]
    assert sum(m[4] != 0 for m in trunc) > 0.5 * len(trunc)
    assert dumped == P.load_corrupt()
