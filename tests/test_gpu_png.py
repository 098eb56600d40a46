"""GPU tests of the PNG decoder (msml_amd/png.py, csrc/png.hip): every supported stream of tests/golden/g17_png.npz
bit for bit against the L / RGB / RGBA arrays Pillow recorded, in one mixed-size packed launch and in uniform launches,
RGB / BGR, inside guard bands around the destination and the workspace; batches of 1, 2, 65 and 300; the corrupt
streams the host check recorded (tests/golden/g17_png_corrupt.npz, tools/png_hostcheck.cpp) with the host's statuses;
the refusals of the C entry point; and the consumers (imageio.decode_images, verification.load_folder,
ijb.align_faces).  Every comparison is equality."""
import io

import numpy as np
import pytest
import torch

from msml_amd import _lib, ijb, imageio, jpeg, png, verification
from tests import jpeg_cases as J
from tests import png_cases as P
from tests.packed_cases import FILL, bands_untouched, batch_sizes, canaries_intact, decode_at, guarded, packed_meta, unpack

pytestmark = pytest.mark.gpu
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        cases, _ = P.load_golden()
        _CACHE["g"] = (cases, [c for c in cases if c["supported"]], {c["name"]: c for c in cases})
    return _CACHE["g"]


def decode_guarded(streams, channels=3, order="rgb"):
    """One packed launch into a guarded, pre-filled dst and a guarded workspace -> ((dst, meta), status numpy)."""
    batch = png.pack_pngs(streams)
    meta, total = packed_meta(batch_sizes(batch), channels, gap=32)
    dwhole, dst = guarded(total)
    wwhole, ws = guarded(batch.ws_bytes, 0x5C)
    status = png.decode_into(batch, dst, meta, channels, order, ws=ws)
    torch.cuda.synchronize()
    assert bands_untouched(dwhole) and bands_untouched(wwhole, 0x5C) and canaries_intact(dst, meta)
    return (dst, meta), status.cpu().numpy()


def swapped(img, order):
    if order == "rgb" or img.ndim == 2:
        return img
    return np.concatenate([img[..., 2::-1], img[..., 3:]], axis=2)


def test_bit_exact_mixed_sizes_one_launch():
    _, sup, _ = golden()
    assert len(sup) >= 80
    for channels, mode in ((3, "RGB"), (4, "RGBA")):
        for order in ("rgb", "bgr"):
            (buf, meta), status = decode_guarded([c["data"] for c in sup], channels, order)
            assert (status == 0).all(), [(c["name"], s) for c, s in zip(sup, status) if s]
            for c, img in zip(sup, unpack(buf, meta, channels)):
                assert np.array_equal(img, swapped(c[mode], order)), (mode, order, c["name"])
    gray = [c for c in sup if "L" in c]
    assert len(gray) >= 20
    (buf, meta), status = decode_guarded([c["data"] for c in gray], 1)
    assert (status == 0).all()
    for c, img in zip(gray, unpack(buf, meta, 1)):
        assert np.array_equal(img, c["L"]), c["name"]


def test_bit_exact_uniform_launches():
    _, sup, by = golden()
    groups = {}
    for c in sup:
        groups.setdefault(c["RGB"].shape[:2], []).append(c)
    assert len(groups) >= 12
    for (h, w), cs in groups.items():
        for channels, mode, order in ((3, "RGB", "rgb"), (3, "RGB", "bgr"), (4, "RGBA", "rgb"), (4, "RGBA", "bgr")):
            out = png.decode_batch([c["data"] for c in cs], size=(h, w), order=order, channels=channels)
            assert out.shape == (len(cs), h, w, channels) and out.dtype == torch.uint8
            for c, img in zip(cs, out.cpu().numpy()):
                assert np.array_equal(img, swapped(c[mode], order)), (c["name"], mode, order)
        g = [c for c in cs if "L" in c]
        if g:
            out = png.decode_batch([c["data"] for c in g], size=(h, w), channels=1)
            assert out.shape == (len(g), h, w)
            for c, img in zip(g, out.cpu().numpy()):
                assert np.array_equal(img, c["L"]), c["name"]
    with pytest.raises(ValueError, match="image 1 is"):
        png.decode_batch([by["rgb_64x64_level9"]["data"], by["rgb_112x112_pillow"]["data"]], size=(64, 64))
    with pytest.raises(ValueError, match="gray"):
        png.decode_batch([by["rgb_64x64_level9"]["data"]], size=(64, 64), channels=1)
    with pytest.raises(ValueError):
        png.decode_batch([by["rgb_64x64_level9"]["data"]], channels=2)


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_batch_independence(n):
    """Large streams among tiny ones; every image's result is that of its stream wherever it stands, more images than
    one launch's first wave of workgroups (300 > 256 CUs), and two runs give the same bits."""
    _, sup, by = golden()
    big = [by[k] for k in ("rgb_112x112_pillow", "rgba_128x128_occluder", "tok_dist32768_wrap_flush", "rgba_113x111_cycle")]
    tiny = [c for c in sup if c["RGB"].shape[0] * c["RGB"].shape[1] <= 15]
    assert len(tiny) >= 20
    seq = [(big[(i // 2) % 4] if i % 2 == 0 else tiny[(7 * i) % len(tiny)]) for i in range(n)]
    (buf, meta), status = decode_guarded([c["data"] for c in seq], 4)
    assert (status == 0).all()
    for c, img in zip(seq, unpack(buf, meta, 4)):
        assert np.array_equal(img, c["RGBA"]), c["name"]
    (buf2, _), _ = decode_guarded([c["data"] for c in seq], 4)
    assert torch.equal(buf, buf2)


def test_corrupt_streams_as_the_host_check():
    """Only inputs tools/png_hostcheck.cpp has decoded on the host under the sanitizers: the device gives the host's
    statuses, an image with a status leaves its rectangle as it was, the clean neighbours are bit-exact, the guard
    bands intact."""
    _, sup, by = golden()
    rec = P.load_corrupt()
    assert len(rec) >= 90 and {r[0] for r in rec} == {"trunc", "subst", "hdrbit", "splice", "trailer", "filter"}
    assert {r[4] for r in rec} >= set(range(0, 11))
    neighbours = [by["rgb_112x112_pillow"], by["ct3_d4_17x13_cycle"], by["tok_dynamic_15_bit_codes"]]
    streams, expect = [], []
    for i, r in enumerate(rec):
        streams.append(P.with_zlib_stream(sup[r[1]]["data"], r[5]))
        expect.append(r[4])
        if i % 8 == 0:
            streams.append(neighbours[(i // 8) % 3]["data"])
            expect.append(None)
    (buf, meta), status = decode_guarded(streams)
    imgs = unpack(buf, meta, ok=status == 0)
    k = 0
    for i, (e, st) in enumerate(zip(expect, status)):
        if e is None:
            assert st == 0 and np.array_equal(imgs[i], neighbours[k % 3]["RGB"])
            k += 1
        else:
            r = rec[i - k]
            assert st == e, (i, r[:5], st)
            if e == 0:                                       # a mutation that left a valid stream: the host's pixels
                assert np.array_equal(imgs[i], P.decode_png(streams[i], 3))
    bad = next(r for r in rec if r[4] == 9)
    with pytest.raises(ValueError, match="image 1: Adler-32 mismatch"):
        png.decode_batch([neighbours[1]["data"], P.with_zlib_stream(sup[bad[1]]["data"], bad[5]), neighbours[2]["data"]])


def test_unsupported_streams(monkeypatch):
    cases, sup, by = golden()
    bad = [by["bad_16bit"]["data"], by["bad_adam7"]["data"], by["bad_crc"]["data"]]
    mixed = [sup[0]["data"], bad[0], sup[7]["data"], bad[1]]
    buf, meta, status = png.decode_batch(mixed, strict=False)
    assert status.cpu().tolist() == [0, png.SIXTEEN_BIT, 0, png.INTERLACE]
    flat = buf.cpu().numpy()
    for i in (0, 2):
        off, h, w, pitch = meta[i]
        assert np.array_equal(flat[off:off + h * pitch].reshape(h, pitch)[:, :w * 3].reshape(h, w, 3), sup[(0, 0, 7)[i]]["RGB"])
    with pytest.raises(ValueError, match="image 1: 16-bit"):
        png.decode_batch(mixed)

    def no_call(*a, **k):
        raise AssertionError("a launch for a batch without a supported stream")

    monkeypatch.setattr(png, "call", no_call)
    _, _, status = png.decode_batch(bad, strict=False)
    assert status.cpu().tolist() == [png.SIXTEEN_BIT, png.INTERLACE, png.BAD_CRC]
    with pytest.raises(ValueError, match="image 0"):
        png.decode_batch(bad)


def test_unaligned_destinations_inside_canaries():
    """The byte path of the store (an offset or a pitch that is no multiple of 4) next to canaries: rectangles at offset
    5 with pitch = row bytes + 3 get the fixture's pixels and leave every byte between a row's end and its pitch alone;
    at offset 8 with whole dwords per row those bytes are 0.  Every W mod 4 and W < 4."""
    _, sup, by = golden()
    picked = [c for c in sup if any(k in c["name"] for k in ("_1x1_", "_7x1_", "_3x5_", "_1x7_"))]
    picked += [by["paeth_ties_8x8"], by["rgb_150x150_level0"]]
    assert len(picked) == 20 and {c["RGB"].shape[1] % 4 for c in picked} == {0, 1, 2, 3}
    for channels, mode in ((1, "L"), (3, "RGB"), (4, "RGBA")):
        cs = [c for c in picked if mode in c]
        assert len(cs) >= 7
        batch = png.pack_pngs([c["data"] for c in cs])
        for offset, extra, pad in ((5, 3, FILL), (8, None, 0)):
            imgs = decode_at(batch, png.decode_into, channels, offset, extra, pad)
            for c, img in zip(cs, imgs):
                assert np.array_equal(img, c[mode]), (mode, offset, c["name"])


def test_abi_errors():
    _, sup, by = golden()
    batch = png.pack_pngs([by["rgb_112x112_pillow"]["data"], by["ct3_d4_17x13_cycle"]["data"]])
    meta, total = packed_meta(batch_sizes(batch))
    streams, desc, pal = batch.to_device(torch.device("cuda", 0))
    dst = torch.zeros(total + 8, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(batch.ws_bytes + 16, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    mdev = torch.from_numpy(meta).cuda()
    host = batch.desc.data_ptr()

    def run(**kw):
        a = dict(streams=streams, sb=streams.numel(), desc=desc, host=host, pal=pal, pb=pal.numel(), dst=dst,
                 db=dst.numel(), meta=mdev, ch=3, swap=0, status=status, ws=ws, wb=batch.ws_bytes, n=2)
        a.update(kw)
        return _lib.call_status("msml_png_decode", *a.values())

    SHAPE, UNSUP, WORKSPACE = -1, -4, -5
    for name in ("streams", "desc", "host", "pal", "dst", "meta", "status", "ws"):
        assert run(**{name: None}) == SHAPE, name
    assert run(dst=dst.data_ptr() + 1) == SHAPE and run(ws=ws.data_ptr() + 4) == SHAPE
    assert run(streams=streams.data_ptr() + 2) == SHAPE and run(meta=mdev.data_ptr() + 4) == SHAPE
    assert run(status=status.data_ptr() + 2) == SHAPE
    assert run(n=0) == UNSUP and run(n=-1) == UNSUP and run(n=65536) == UNSUP
    assert run(ch=2) == UNSUP and run(ch=5) == UNSUP and run(ch=1) == UNSUP   # a colour stream into one channel
    assert run(wb=batch.ws_bytes - 1) == WORKSPACE and run(wb=0) == WORKSPACE
    assert run(pb=0) == SHAPE and run(pb=1000) == SHAPE                   # not whole palettes / the index past them
    assert run(sb=streams.numel() - 4) == SHAPE                           # a stream past the buffer
    assert run(sb=streams.numel() - 1) == SHAPE                           # not whole dwords
    assert "png_decode" in _lib.load().msml_last_error().decode()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [-7, -7] and int(dst.sum()) == 0      # before any launch
    assert _lib.value("msml_png_workspace", None, 2) == 0 and _lib.value("msml_png_workspace", host, 0) == 0
    # a destination the image does not fit: status 11 for that image alone, nothing written outside
    small = meta.copy()
    small[1, 2] += 1
    st = png.decode_into(batch, dst, small)
    assert st.cpu().tolist() == [0, png.STATUS_OUTPUT]
    short = torch.zeros(int(meta[1, 0]) + 8, dtype=torch.uint8, device="cuda")
    st = png.decode_into(batch, short, meta)
    assert st.cpu().tolist() == [0, png.STATUS_OUTPUT]
    assert run() == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0]


def _jpeg_cases():
    cases, _ = J.load_golden()
    by = {c["name"]: c for c in cases}
    return [by[n] for n in ("face0_112x112_420_q95_r3", "17x23_420_q95_r0", "face3_112x112_gray_q95_r0")]


def test_decode_images_interleaves_both_formats():
    _, sup, by = golden()
    jp = _jpeg_cases()
    pn = [by["rgb_112x112_pillow"], by["rgba_128x128_occluder"], by["ct3_d4_17x13_cycle"], by["gray_la_112x112_pillow"]]
    seq = [pn[0], jp[0], jp[1], pn[1], pn[2], jp[2], pn[3]]
    isj = [False, True, True, False, False, True, False]
    for order in ("rgb", "bgr"):
        buf, meta = imageio.decode_images([c["data"] for c in seq], order=order)
        assert meta.dtype == np.int64 and meta.shape == (7, 4) and buf.dtype == torch.uint8
        jbuf, jmeta = jpeg.decode_batch([c["data"] for c in jp], order=order)
        pbuf, pmeta = png.decode_batch([c["data"] for c in pn], order=order)
        apart = iter(unpack(jbuf, jmeta)), iter(unpack(pbuf, pmeta))
        for c, j, img in zip(seq, isj, unpack(buf, meta)):
            assert np.array_equal(img, next(apart[0] if j else apart[1])), c["name"]
            want = J.as_rgb(c["pixels"]) if j else c["RGB"]
            assert np.array_equal(img, want if order == "rgb" else want[:, :, ::-1])
    blobs = [seq[0]["data"], b"GIF89a" + bytes(20), seq[1]["data"], by["bad_adam7"]["data"]]
    with pytest.raises(ValueError, match="image 1: neither"):
        imageio.decode_images(blobs)
    buf, meta, status = imageio.decode_images(blobs, strict=False)
    assert status.cpu().tolist() == [0, imageio.UNKNOWN_FORMAT, 0, png.INTERLACE]
    imgs = unpack(buf, meta[[0, 2]])
    assert np.array_equal(imgs[0], seq[0]["RGB"]) and np.array_equal(imgs[1], J.as_rgb(seq[1]["pixels"]))
    with pytest.raises(ValueError, match="image 0: Adam7"):
        imageio.decode_images([by["bad_adam7"]["data"]])
    assert imageio.sniff(seq[0]["data"]) == "png" and imageio.sniff(seq[1]["data"]) == "jpeg" and imageio.sniff(b"") is None


def test_load_folder_then_read_pairs(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(5)
    tree = {"bob": ["0002.png", "0001.jpg", "0003.png"], "alice": ["0001.png", "0002.jpg"]}
    arrays = {}
    for ident, files in tree.items():
        (tmp_path / "faces" / ident).mkdir(parents=True)
        for f in files:
            h, w = (112, 112) if f != "0003.png" else (37, 53)
            a = (np.add.outer(np.arange(h) * 2, np.arange(w))[:, :, None] + rng.randint(0, 40, (h, w, 3))).astype(np.uint8)
            Image.fromarray(a).save(str(tmp_path / "faces" / ident / f), quality=95)
            arrays[(ident, f)] = a
    files, buf, meta = verification.load_folder(str(tmp_path / "faces"))
    assert files == {"alice": ["0001.png", "0002.jpg"], "bob": ["0001.jpg", "0002.png", "0003.png"]}
    order = verification.pairs_file_order(files)
    imgs = unpack(buf, meta)
    for (ident, f), img in zip(order, imgs):
        blob = (tmp_path / "faces" / ident / f).read_bytes()
        if f.endswith(".png"):
            assert np.array_equal(img, arrays[(ident, f)])                      # lossless: the array that was saved
            assert np.array_equal(img, np.asarray(Image.open(io.BytesIO(blob)).convert("RGB")))
        else:
            jb, jm = jpeg.decode_batch([blob])
            assert np.array_equal(img, unpack(jb, jm)[0])
    pairs, same = verification.read_pairs_txt(["alice 1 2", "alice 2 bob 3", "bob 1 2"], files)
    assert pairs.tolist() == [[0, 1], [1, 4], [2, 3]] and same.tolist() == [True, False, True]
    assert imgs[4].shape == (37, 53, 3) and order[4] == ("bob", "0003.png")
    (tmp_path / "faces" / "bob" / "0004.png").write_bytes(golden()[2]["bad_adam7"]["data"])
    with pytest.raises(ValueError, match="bob/0004.png.*Adam7"):
        verification.load_folder(str(tmp_path / "faces"))


def test_align_faces_takes_the_decoded_batch():
    _, sup, by = golden()
    cs = [by["rgb_112x112_pillow"], by["ct2_d8_17x13_cycle"], by["gray_la_112x112_pillow"], by["rgba_128x128_occluder"]]
    rng = np.random.RandomState(3)
    mats = np.stack([np.array([[0.9, 0.1, 2.0], [-0.1, 0.9, 3.0]]) + rng.uniform(-0.05, 0.05, (2, 3)) for _ in cs])
    buf, meta = png.decode_batch([c["data"] for c in cs], order="bgr")
    got = ijb.align_faces(buf, meta, mats)
    hbuf, hmeta = ijb.pack_images([np.ascontiguousarray(c["RGB"][:, :, ::-1]) for c in cs])
    want = ijb.align_faces(hbuf, hmeta, mats)
    assert got.shape == (4, 112, 112, 3) and torch.equal(got, want)
    assert int(got.float().std()) > 0
