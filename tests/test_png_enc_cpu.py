"""CPU tests of PNG encoding: the numpy restatement (tests/png_enc_cases.py: filter pass, container, bound, reference
cost) against straightforward references, Pillow, zlib and the project's own parser; PNG payloads through write_faces and
RecordFile; the argument errors of png.encode_batch; and the encoder's core header built on the host under the sanitizers
(tools/png_enc_hostcheck.cpp, its own process) with every file it writes inflated by the installed zlib."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from msml_amd import imageio, jpeg, png
from tests import hostcheck
from tests import png_enc_cases as E

_CACHE = {}
MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def golden():
    if "g" not in _CACHE:
        _CACHE["g"] = {k: E.as_hwc(v) for k, v in E.load_golden().items()}
    return _CACHE["g"]


def reference_filter(a, flt):
    """The PNG specification's filters, one byte at a time; adaptive: the smallest sum of abs((int8) byte), ties low."""
    h, w, c = a.shape
    raw = a.reshape(h, w * c).astype(int)
    out = bytearray()
    for y in range(h):
        rows = []
        for f in range(5):
            r = []
            for j in range(w * c):
                x, left = raw[y, j], raw[y, j - c] if j >= c else 0
                up, ul = (raw[y - 1, j] if y else 0), (raw[y - 1, j - c] if y and j >= c else 0)
                p = left + up - ul
                pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                paeth = left if pa <= pb and pa <= pc else up if pb <= pc else ul
                r.append((x - (0, left, up, (left + up) // 2, paeth)[f]) & 255)
            rows.append(r)
        if flt == "adaptive":
            sums = [sum(v if v < 128 else 256 - v for v in r) for r in rows]
            f = sums.index(min(sums))
        else:
            f = E.FILTERS[flt]
        out += bytes([f]) + bytes(rows[f])
    return bytes(out)


@pytest.mark.parametrize("flt", sorted(E.FILTERS))
def test_filter_restatement_against_per_byte_reference(flt):
    r = np.random.RandomState(3)
    small = [r.randint(0, 256, s).astype(np.uint8) for s in ((1, 1, 1), (1, 9, 3), (9, 1, 4), (6, 7, 2), (5, 4, 3))]
    small += [golden()[k] for k in ("rgba7x5", "png_paeth_ties_8x8", "png_ct2_d8_17x13_cycle", "png_tok_d1_l258")]
    small.append((r.randint(0, 3, (8, 8, 3)) * 127).astype(np.uint8))          # many ties
    for a in small:
        assert E.filtered_bytes(a, flt) == reference_filter(E.as_hwc(a), flt), (a.shape, flt)
    a = small[4]
    assert E.filtered_bytes(np.ascontiguousarray(a[..., ::-1]), flt, "bgr") == E.filtered_bytes(a, flt)


def test_container_reads_back_everywhere():
    """Every fixture image: Pillow verifies the CRCs and returns the source, the project's parser takes the file."""
    for name, a in golden().items():
        for flt in ("adaptive", "none"):
            data = E.encode(a, flt)
            Image.open(io.BytesIO(data)).verify()
            im = Image.open(io.BytesIO(data))
            assert im.mode == MODES[a.shape[2]] and np.array_equal(E.as_hwc(np.asarray(im)), a), name
            d = png.parse_png(data)
            assert d.status == 0 and (d.height, d.width, d.depth) == (a.shape[0], a.shape[1], 8), name
            assert d.colour_type == png.COLOUR_TYPE_OF[a.shape[2]] and len(d.idat) == 1
            assert zlib.decompress(E.idat_of(data)) == E.filtered_bytes(a, flt)


def test_bound_is_the_all_stored_file():
    for shape in ((1, 1, 1), (112, 112, 3), (200, 150, 3), (3, 32767, 1), (257, 255, 1), (3, 21845, 1), (1, 65534, 1)):
        h, w, c = shape
        if w > 32767:
            continue
        a = np.zeros(shape, np.uint8)
        assert len(E.encode(a, "none")) == E.bound(h, w, c) == png.encode_bound(h, w, c), shape
    assert png.encode_bound(0, 5, 3) == 0 and png.encode_bound(5, 5, 5) == 0 and png.encode_bound(32767, 32767, 4) == 0
    n = 65535 * 2 + 1                                           # three stored blocks
    assert E.bound(1, n - 1, 1) == 8 + 25 + 12 + 2 + n + 15 + 4 + 12


def test_reference_cost():
    """Package-merge: Kraft holds, the limit holds, and without the limit binding it is Huffman's cost."""
    import heapq
    r = np.random.RandomState(1)
    for _ in range(20):
        counts = r.randint(0, 50, 257) * (r.rand(257) < 0.5)
        counts[256] = 1
        lens = E.limited_lengths(counts)
        heap = [int(c) for c in counts if c]
        heapq.heapify(heap)
        cost = 0
        while len(heap) > 1:
            s = heapq.heappop(heap) + heapq.heappop(heap)
            cost += s
            heapq.heappush(heap, s)
        assert int((counts * lens).sum()) == cost
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    lens = E.limited_lengths(np.array(fib), 15)
    assert lens.max() == 15 and (2.0 ** -lens).sum() <= 1
    assert E.literal_cost_bits(b"\x00" * 100) == 101


def test_png_payloads_through_records(tmp_path):
    """write_faces / RecordFile with PNG files as payloads, from byte strings (the EncodedBatch path runs on the GPU)."""
    ns = ["face0", "face1", "rgba7x5", "s1x300x1"]
    files = [E.encode(golden()[k]) for k in ns]
    rec, idx = str(tmp_path / "train.rec"), str(tmp_path / "train.idx")
    with jpeg.RecordWriter(rec, idx) as w:
        assert jpeg.write_faces(w, files[:2], [5, 6], 1, header0=(4, 10)) == 3
        assert jpeg.write_faces(w, files[2:], np.array([7, 8]), 3) == 5
    with jpeg.RecordFile(rec, idx) as f:
        assert f.header0 == (5, 10) and f.img_idx.tolist() == [1, 2, 3, 4]
        assert [f.read_idx(i)[1] for i in range(1, 5)] == files
        assert [f.read_idx(i)[0][1] for i in range(1, 5)] == [5.0, 6.0, 7.0, 8.0]
    with jpeg.RecordFaceSource(str(tmp_path), 2, steps=2, raw=True) as src:
        got = [(blobs, lab.tolist()) for blobs, lab in src]
    assert got == [(files[:2], [5, 6]), (files[2:], [7, 8])]
    assert [imageio.sniff(b) for b in files] == ["png"] * 4
    length = torch.tensor([len(b) for b in files], dtype=torch.int32)
    caps = np.array([(len(b) + 3) & ~3 for b in files], np.int64)
    slots = np.stack([np.cumsum(caps) - caps, caps], 1)
    buf = torch.zeros(int(caps.sum()), dtype=torch.uint8)
    for (o, _), b in zip(slots, files):
        buf[o:o + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy())
    enc = jpeg.EncodedBatch(buf, torch.from_numpy(slots), slots, length, torch.zeros(4, dtype=torch.int32), None)
    assert enc.to_bytes() == files
    with jpeg.RecordWriter(rec, idx) as w:
        assert jpeg.write_faces(w, enc, [1, 2, 3, 4]) == 5
    with jpeg.RecordFile(rec, idx) as f:
        assert [f.read_idx(i)[1] for i in range(1, 5)] == files


def test_argument_errors_without_a_gpu():
    ok = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    for kwargs in (dict(images=ok.float()), dict(images=torch.zeros(2, 4, 4, 5, dtype=torch.uint8)),
                   dict(images=ok, filter="best"), dict(images=ok[..., 0], order="bgr"),
                   dict(images=torch.zeros(2, 4, 4, 1, dtype=torch.uint8)), dict(images=ok, order="gbr"),
                   dict(images=(ok.reshape(-1), np.zeros((2, 4), np.int64)), channels=5),
                   dict(images=torch.zeros(4, 4, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            png.encode_batch(device="cpu", **kwargs)
    with pytest.raises(ValueError):
        imageio.format_of("a.bmp")
    assert [imageio.format_of(s) for s in ("png", "JPG", ".jpeg", "x/y.PNG", "a.b.jfif")] == ["png", "jpeg", "jpeg", "png", "jpeg"]
    plan = png.PngEncodePlan([(112, 112), (1, 1)], 3)
    assert plan.bounds.tolist() == [(E.bound(112, 112, 3) + 3) & ~3, (E.bound(1, 1, 3) + 3) & ~3]
    assert plan.ws_bytes > 0 and plan.desc.numpy()[0, png.PE_WS] == 0 and plan.desc.numpy()[1, png.PE_WS] > 0


def test_enc_host_check_under_sanitizers(tmp_path):
    """tools/png_enc_hostcheck.cpp with -fsanitize=address,undefined, its own process: csrc/png_enc_core.h on the host in
    the kernels' order over the fixture and 3 000 random sizes, channel counts, filters, orders and contents (flat,
    noise, periods around 1, 3, 258, 32767, 32768, 32769).  The program itself checks that the bits it writes are the
    bits it counted and that no file passes the bound; here every file is a PNG Pillow and the project's parser take
    (CRCs), and zlib inflates its IDAT to the restatement's filtered bytes; nothing is reported."""
    if hostcheck.host_compiler() is None:
        pytest.skip("no host C++ compiler")
    if not hostcheck.sanitizers_link(str(tmp_path)):
        pytest.skip("the host compiler cannot link a trivial program with -fsanitize=address,undefined")
    exe = E.build_hostcheck(str(tmp_path / "hostcheck"))                      # a failure to build THIS is a failure
    cases = [(a, flt, "rgb") for a in golden().values() for flt in ("adaptive", "none", "paeth")]
    cases += [(E.tall(32767, 1), "none", "rgb"), (E.tall(16384, 2), "none", "rgb")]
    cases += E.random_cases(3000)
    E.write_hostcheck_input(str(tmp_path / "in.bin"), cases)
    rc, err, files = E.run_hostcheck(exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"))
    assert rc == 0 and err == "", err[-2000:]
    assert len(files) == len(cases)
    packed = 0
    for (a, flt, order), data in zip(cases, files):
        a = E.as_hwc(a)
        filt = E.filtered_bytes(a, flt, order)
        assert len(data) <= E.bound(*a.shape), (a.shape, flt)
        assert png.parse_png(data).status == 0, (a.shape, flt)
        assert zlib.decompress(E.idat_of(data)) == filt, (a.shape, flt, order)
        packed += len(data) < len(filt)
    assert packed > len(cases) // 4                              # the matcher and the codes do work
    big = [(a, f) for (a, f, o), d in zip(cases, files) if E.as_hwc(a).size > 20000][:12]
    for (a, flt), data in zip(big, [d for (a, f, o), d in zip(cases, files) if E.as_hwc(a).size > 20000][:12]):
        assert len(data) <= E.size_limit(E.filtered_bytes(a, flt))
        Image.open(io.BytesIO(data)).verify()
