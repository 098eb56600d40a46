"""GPU tests of the JPEG decoder (msml_amd/jpeg.py, csrc/jpeg.hip): every supported stream of tests/golden/g15_jpeg.npz
bit for bit against the pixels Pillow (libjpeg-turbo) recorded, in one mixed-size packed launch and in uniform
launches, RGB / BGR / single channel, inside guard bands; batches whose neighbours differ 100x in length; the
corrupt streams the host check recorded (tests/golden/g15_jpeg_corrupt.npz, tools/jpeg_hostcheck.cpp) with the host's
statuses; the refusals of the C entry point; and the three consumers (DeviceLoaderX, ijb.align_faces, load_bin)."""
import pickle

import numpy as np
import pytest
import torch

from msml_amd import _lib, data, ijb, jpeg, verification
from tests import jpeg_cases as J
from tests import jpeg_enc_cases as E
from tests.packed_cases import FILL, bands_untouched, batch_sizes, decode_at, guarded, packed_meta, unpack

pytestmark = pytest.mark.gpu
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        cases, _ = J.load_golden()
        _CACHE["g"] = (cases, [c for c in cases if c["supported"]], {c["name"]: c for c in cases})
    return _CACHE["g"]


def decode_guarded(streams, channels=3, order="rgb"):
    """One packed launch into guarded dst and workspace -> (images, status numpy); asserts the guard bands."""
    batch = jpeg.pack_jpegs(streams)
    meta, total = packed_meta(batch_sizes(batch), channels)
    dwhole, dst = guarded(total)
    wwhole, ws = guarded(batch.ws_bytes, 0x5C)
    status = jpeg.decode_into(batch, dst, meta, channels, order, ws=ws)
    torch.cuda.synchronize()
    assert bands_untouched(dwhole) and bands_untouched(wwhole, 0x5C)
    return (dst, meta), status.cpu().numpy()


def test_bit_exact_mixed_sizes_one_launch():
    _, sup, _ = golden()
    assert len(sup) >= 200
    for order in ("rgb", "bgr"):
        (buf, meta), status = decode_guarded([c["data"] for c in sup], 3, order)
        assert (status == 0).all()
        for c, img in zip(sup, unpack(buf, meta)):
            want = J.as_rgb(c["pixels"])
            assert np.array_equal(img, want if order == "rgb" else want[:, :, ::-1]), (order, c["name"])
    gray = [c for c in sup if c["pixels"].ndim == 2]
    assert len(gray) >= 48
    (buf, meta), status = decode_guarded([c["data"] for c in gray], 1)
    assert (status == 0).all()
    for c, img in zip(gray, unpack(buf, meta, 1)):
        assert np.array_equal(img, c["pixels"]), c["name"]


def test_bit_exact_uniform_launches():
    _, sup, _ = golden()
    groups = {}
    for c in sup:
        groups.setdefault(c["pixels"].shape[:2], []).append(c)
    assert len(groups) >= 13
    for (h, w), cs in groups.items():
        for order in ("rgb", "bgr"):
            out = jpeg.decode_batch([c["data"] for c in cs], size=(h, w), order=order)
            assert out.shape == (len(cs), h, w, 3) and out.dtype == torch.uint8
            got = out.cpu().numpy()
            for c, img in zip(cs, got):
                want = J.as_rgb(c["pixels"])
                assert np.array_equal(img, want if order == "rgb" else want[:, :, ::-1]), c["name"]
        g = [c for c in cs if c["pixels"].ndim == 2]
        if g:
            out = jpeg.decode_batch([c["data"] for c in g], size=(h, w), channels=1)
            assert out.shape == (len(g), h, w)
            for c, img in zip(g, out.cpu().numpy()):
                assert np.array_equal(img, c["pixels"]), c["name"]
    with pytest.raises(ValueError, match="image 1 is"):
        jpeg.decode_batch([sup[0]["data"], golden()[2]["face0_112x112_420_q95_r3"]["data"]], size=sup[0]["pixels"].shape[:2])
    with pytest.raises(ValueError, match="gray"):
        jpeg.decode_batch([golden()[2]["face0_112x112_420_q95_r3"]["data"]], size=(112, 112), channels=1)


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_batch_independence(n):
    """112 x 112 streams among tiny ones (lengths differ 100x); every image's result is that of its stream wherever it
    stands, more images than one launch's first wave of workgroups (300 > 256 CUs), and two runs give the same bits."""
    _, sup, by = golden()
    big = [c for c in sup if "112x112" in c["name"]]
    tiny = [c for c in sup if c["name"].startswith(("1x1_", "9x1_", "5x2_"))]

    def coded(c):
        d = jpeg.parse_jpeg(c["data"])
        return d.end - d.begin

    assert max(coded(c) for c in big) >= 100 * min(coded(c) for c in tiny)
    seq = [(big[(i // 2) % 4] if i % 2 == 0 else tiny[(7 * i) % len(tiny)]) for i in range(n)]
    (buf, meta), status = decode_guarded([c["data"] for c in seq])
    assert (status == 0).all()
    for c, img in zip(seq, unpack(buf, meta)):
        assert np.array_equal(img, J.as_rgb(c["pixels"])), c["name"]
    (buf2, _), _ = decode_guarded([c["data"] for c in seq])
    assert torch.equal(buf, buf2)


def test_edge_cases():
    _, sup, by = golden()
    one = by["mcu1_17x23_420_q75_r1"]
    assert jpeg.parse_jpeg(one["data"]).restart_interval == 1
    ff = [c for c in sup if b"\xff\x00" in c["data"][jpeg.parse_jpeg(c["data"]).begin:]]
    assert ff, "the fixture must hold a stream with a stuffed FF"
    d16 = by["dqt16_17x23_422_q30_r0"]
    assert b"\xff\xdb\x00\x83\x10" in d16["data"]
    gray = by["face3_112x112_gray_q95_r0"]
    checker = by["checker17x9_420_q95_r3"]
    assert checker["pixels"].min() == 0 and checker["pixels"].max() == 255       # the clamps
    for c in [one, ff[0], ff[-1], d16, gray, checker]:
        h, w = c["pixels"].shape[:2]
        out = jpeg.decode_batch([c["data"]], size=(h, w))[0].cpu().numpy()
        assert np.array_equal(out, J.as_rgb(c["pixels"])), c["name"]
    out = jpeg.decode_batch([gray["data"]], size=(112, 112))[0]
    assert torch.equal(out[..., 0], out[..., 1]) and torch.equal(out[..., 0], out[..., 2])


def test_unsupported_streams(monkeypatch):
    cases, sup, by = golden()
    bad = [by["progressive_16x16"]["data"], by["s411_32x16"]["data"]]
    mixed = [sup[0]["data"], bad[0], sup[5]["data"], bad[1]]
    buf, meta, status = jpeg.decode_batch(mixed, strict=False)
    assert status.cpu().tolist() == [0, jpeg.PROGRESSIVE, 0, jpeg.SAMPLING]
    imgs = unpack(buf, meta, check_pad=False)
    assert np.array_equal(imgs[0], J.as_rgb(sup[0]["pixels"])) and np.array_equal(imgs[2], J.as_rgb(sup[5]["pixels"]))
    with pytest.raises(ValueError, match="image 1: progressive"):
        jpeg.decode_batch(mixed)
    # only refused streams: the statuses come from the parser, nothing is launched

    def no_call(*a, **k):
        raise AssertionError("a launch for a batch without a supported stream")

    monkeypatch.setattr(jpeg, "call", no_call)
    _, _, status = jpeg.decode_batch(bad, strict=False)
    assert status.cpu().tolist() == [jpeg.PROGRESSIVE, jpeg.SAMPLING]
    with pytest.raises(ValueError, match="image 0"):
        jpeg.decode_batch(bad)


def test_corrupt_streams_as_the_host_check():
    """Only inputs tools/jpeg_hostcheck.cpp has decoded on the host under the sanitizers: the device gives the host's
    statuses, the clean neighbours are bit-exact, the guard bands intact."""
    _, sup, by = golden()
    rec = J.load_corrupt()
    assert len(rec) >= 300 and {r[0] for r in rec} == {"trunc", "ffxx", "subst", "cut", "rstdel", "rstswap"}
    assert sum(r[4] != 0 for r in rec) >= 100 and {r[4] for r in rec} >= {0, 1, 4, 5}
    neighbours = [by["face0_112x112_420_q95_r3"], by["9x3_422_q75_r3"], by["17x23_444_q100_r3"]]
    streams, expect = [], []
    for i, r in enumerate(rec):
        streams.append(r[5])
        expect.append(r[4])
        if i % 8 == 0:
            streams.append(neighbours[(i // 8) % 3]["data"])
            expect.append(None)
    (buf, meta), status = decode_guarded(streams)
    imgs = unpack(buf, meta, check_pad=False)
    k = 0
    for i, (e, st) in enumerate(zip(expect, status)):
        if e is None:
            assert st == 0 and np.array_equal(imgs[i], J.as_rgb(neighbours[k % 3]["pixels"]))
            k += 1
        else:
            assert st == e, (i, rec[i - k][:5], st)
    # strict decoding names the first image the device refused, and why
    cut = next(r for r in rec if r[4] == 5)
    with pytest.raises(ValueError, match="image 1: the data ends before the last MCU"):
        jpeg.decode_batch([neighbours[1]["data"], cut[5], neighbours[2]["data"]])


def test_unaligned_destinations_inside_canaries():
    """The byte path of the store (an offset or a pitch that is no multiple of 4) next to canaries: rectangles at offset
    5 with pitch = row bytes + 3 get the fixture's pixels and leave every byte between a row's end and its pitch alone;
    at offset 8 with whole dwords per row those bytes are 0.  Every W mod 4 and W < 4; the fixture has no width = 2
    (mod 4), so those streams are made here by the restated encoder and decoder (tests/jpeg_enc_cases.py,
    tests/jpeg_cases.py), which the CPU tests pin to Pillow."""
    _, sup, by = golden()
    picked = [c for c in sup if c["name"].startswith(("1x1_", "9x1_", "5x2_", "3x40_", "8x8_"))]
    assert len(picked) == 80 and {c["pixels"].shape[1] % 4 for c in picked} == {0, 1, 3}
    cases = [(c["data"], c["pixels"]) for c in picked + [by["mcu1_17x23_420_q75_r1"]]]
    rng = np.random.RandomState(18)
    for h, w in ((3, 6), (2, 2)):
        src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        for sampling in ("444", "422", "420", "gray"):
            data = E.encode(src, sampling, 75)
            cases.append((data, J.decode(data)))
    assert {px.shape[1] % 4 for _, px in cases} == {0, 1, 2, 3}
    gray = [(data, px) for data, px in cases if px.ndim == 2]
    assert len(gray) == 22
    for channels, cs in ((3, cases), (1, gray)):
        batch = jpeg.pack_jpegs([data for data, _ in cs])
        for offset, extra, pad in ((5, 3, FILL), (8, None, 0)):
            imgs = decode_at(batch, jpeg.decode_into, channels, offset, extra, pad)
            for i, ((_, px), img) in enumerate(zip(cs, imgs)):
                assert np.array_equal(img, J.as_rgb(px) if channels == 3 else px), (channels, offset, i)


def test_abi_errors():
    _, sup, by = golden()
    batch = jpeg.pack_jpegs([by["face0_112x112_420_q95_r3"]["data"], by["9x3_422_q75_r3"]["data"]])
    meta, total = packed_meta(batch_sizes(batch))
    streams, desc, qt, ht = batch.to_device(torch.device("cuda", 0))
    dst = torch.zeros(total + 8, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(batch.ws_bytes + 16, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    mdev = torch.from_numpy(meta).cuda()
    host = batch.desc.data_ptr()

    def run(**kw):
        a = dict(streams=streams, sb=streams.numel(), desc=desc, host=host, qt=qt, nq=qt.shape[0], ht=ht, nh=ht.shape[0],
                 dst=dst, db=dst.numel(), meta=mdev, ch=3, swap=0, status=status, ws=ws, wb=batch.ws_bytes, n=2)
        a.update(kw)
        return _lib.call_status("msml_jpeg_decode", *a.values())

    SHAPE, UNSUP, WORKSPACE = -1, -4, -5
    for name in ("streams", "desc", "host", "qt", "ht", "dst", "meta", "status", "ws"):
        assert run(**{name: None}) == SHAPE, name
    assert run(dst=dst.data_ptr() + 1) == SHAPE and run(ws=ws.data_ptr() + 4) == SHAPE
    assert run(streams=streams.data_ptr() + 2) == SHAPE and run(meta=mdev.data_ptr() + 4) == SHAPE
    assert run(status=status.data_ptr() + 2) == SHAPE
    assert run(n=0) == UNSUP and run(n=-1) == UNSUP and run(n=65536) == UNSUP
    assert run(ch=2) == UNSUP and run(ch=1) == UNSUP                      # a 3-component stream into one channel
    assert run(wb=batch.ws_bytes - 1) == WORKSPACE and run(wb=0) == WORKSPACE
    assert run(nq=1) == SHAPE and run(nh=3) == SHAPE                      # a table selector past the tables
    assert run(sb=streams.numel() - 4) == SHAPE                           # a stream past the buffer
    assert "jpeg_decode" in _lib.load().msml_last_error().decode()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [-7, -7] and int(dst.sum()) == 0      # before any launch
    assert _lib.value("msml_jpeg_workspace", None, 2) == 0 and _lib.value("msml_jpeg_workspace", host, 0) == 0
    # a destination the image does not fit: status 6 for that image alone, nothing written outside
    small = meta.copy()
    small[1, 2] += 1
    st = jpeg.decode_into(batch, dst, small)
    assert st.cpu().tolist() == [0, 6]
    short = torch.zeros(int(meta[1, 0]) + 8, dtype=torch.uint8, device="cuda")
    st = jpeg.decode_into(batch, short, meta)
    assert st.cpu().tolist() == [0, 6]
    assert run() == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0]


def _faces():
    _, sup, by = golden()
    return [by[n] for n in ("face0_112x112_420_q95_r3", "face1_112x112_444_q95_r0", "face2_112x112_422_q75_r3",
                            "face3_112x112_gray_q95_r0")]


def _pil_gray(rgb):
    """Image.convert('L') of an RGB array (ImagingConvert's rgb2l)."""
    r, g, b = [rgb[..., k].astype(np.int64) for k in range(3)]
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


class _DecodedSource:
    """What a host decoder would hand DeviceLoaderX for the same records: uint8 arrays from the fixture's pixels."""

    def __init__(self, items):
        self.items = items

    def __iter__(self):
        return iter(self.items)


@pytest.mark.parametrize("p_mask", [0.0, 0.5])
def test_device_loader_over_jpeg_records(tmp_path, p_mask):
    B, steps, seed = 8, 2, 77
    faces = _faces()
    pick = [faces[(3 * k) % 4] for k in range(B * steps)]
    render = [faces[(k + 1) % 4] for k in range(B * steps)]
    # the mask records: gray streams in the first batch, colour ones in the second (convert('L') of the decode)
    maskr = [faces[3] if k < B else faces[k % 3] for k in range(B * steps)]
    head = (0, 2, [B * steps + 1.0, 5.0], 0, 0, b"")
    J.write_records(tmp_path, [head] + [(1 + k, 0, k % 5, 0, 0, pick[k]["data"]) for k in range(B * steps)])
    J.write_records(tmp_path, [(1 + k, 0, 0, 0, 0, render[k]["data"]) for k in range(B * steps)], "mask_out")
    J.write_records(tmp_path, [(1 + k, 0, 0, 0, 0, maskr[k]["data"]) for k in range(B * steps)], "mask")
    src = jpeg.RecordFaceSource(str(tmp_path), B, steps=steps, masks=p_mask > 0, seed=seed, p_mask=p_mask)
    decoded = []
    for s in range(steps):
        ks = range(s * B, (s + 1) * B)
        item = [torch.from_numpy(np.stack([J.as_rgb(pick[k]["pixels"]) for k in ks]))]
        if p_mask > 0:
            fl = data.mask_flags(seed, s * B, B, p_mask)
            assert fl.any() and not fl.all()
            rows = np.full(B, -1, np.int32)
            rows[fl] = np.arange(fl.sum())
            sel = [k for k in ks if fl[k - s * B]]
            item += [torch.from_numpy(np.stack([J.as_rgb(render[k]["pixels"]) for k in sel])),
                     torch.from_numpy(np.stack([_pil_gray(J.as_rgb(maskr[k]["pixels"])) for k in sel])),
                     torch.from_numpy(rows)]
        item.append(torch.tensor([k % 5 for k in ks], dtype=torch.int64))
        decoded.append(tuple(item))
    got = []
    loader = data.DeviceLoaderX(src, 0, seed=seed, p_mask=p_mask)
    for batch in loader:
        got.append([t.clone() for t in batch])
        assert loader.jpeg_status.shape == (B,) and loader.jpeg_status.cpu().tolist() == [0] * B   # of THIS batch
    want = [[t.clone() for t in batch] for batch in data.DeviceLoaderX(_DecodedSource(decoded), 0, seed=seed, p_mask=p_mask)]
    assert len(got) == len(want) == steps
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and torch.equal(a, b)


def test_device_loader_status_belongs_to_its_batch(tmp_path):
    """A corrupt face in batch 0 and a corrupt mask_out render in batch 1 (both from the host check's record): after
    each __next__, loader.jpeg_status is the status of the batch just returned -- read on the current stream with no
    synchronisation of the test's own -- and a render's failure shows at the face that uses it."""
    B, steps, seed, p_mask = 8, 2, 77, 0.5
    faces = _faces()
    cut = {r[1]: r for r in J.load_corrupt() if r[0] == "cut"}
    cases = golden()[0]
    bad = next(r for i, r in cut.items() if cases[i]["name"] == faces[0]["name"])
    assert bad[4] == 5 and jpeg.parse_jpeg(bad[5]).status == 0
    fl1 = data.mask_flags(seed, B, B, p_mask)
    n1 = int(np.flatnonzero(fl1)[0])
    head = (0, 2, [B * steps + 1.0, 5.0], 0, 0, b"")
    body = [bad[5] if k == 2 else faces[k % 4]["data"] for k in range(B * steps)]
    render = [bad[5] if k == B + n1 else faces[(k + 1) % 4]["data"] for k in range(B * steps)]
    J.write_records(tmp_path, [head] + [(1 + k, 0, k % 5, 0, 0, body[k]) for k in range(B * steps)])
    J.write_records(tmp_path, [(1 + k, 0, 0, 0, 0, render[k]) for k in range(B * steps)], "mask_out")
    J.write_records(tmp_path, [(1 + k, 0, 0, 0, 0, faces[3]["data"]) for k in range(B * steps)], "mask")
    want = [[5 if n == 2 else 0 for n in range(B)], [5 if n == n1 else 0 for n in range(B)]]
    with jpeg.RecordFaceSource(str(tmp_path), B, steps=steps, masks=True, seed=seed, p_mask=p_mask) as src:
        loader = data.DeviceLoaderX(src, 0, seed=seed, p_mask=p_mask)
        seen = []
        for img, msk, ori, lab in loader:
            seen.append(loader.jpeg_status)                     # kept: each batch has a tensor of its own
            assert loader.jpeg_status.tolist() == want[len(seen) - 1]
            assert lab.tolist() == [k % 5 for k in range((len(seen) - 1) * B, len(seen) * B)]
        assert [s.tolist() for s in seen] == want
    # a render the parser refuses is an error with its place, not a silent status
    prog = jpeg.pack_jpegs([golden()[2]["progressive_16x16"]["data"]])
    with pytest.raises(ValueError, match="mask_out: image 0: progressive"):
        jpeg.decode_renders(prog, prog, (112, 112))
    with pytest.raises(ValueError, match="decode_renders: mask: image 0"):
        jpeg.decode_renders(jpeg.pack_jpegs([faces[0]["data"]]), prog, (112, 112))


def test_align_faces_takes_the_decoded_batch():
    _, sup, by = golden()
    cs = [by["face0_112x112_420_q95_r3"], by["17x23_420_q95_r0"], by["face3_112x112_gray_q95_r0"], by["40x3_444_q75_r3"]]
    rng = np.random.RandomState(3)
    mats = np.stack([np.array([[0.9, 0.1, 2.0], [-0.1, 0.9, 3.0]]) + rng.uniform(-0.05, 0.05, (2, 3)) for _ in cs])
    buf, meta = jpeg.decode_batch([c["data"] for c in cs], order="bgr")
    got = ijb.align_faces(buf, meta, mats)
    hbuf, hmeta = ijb.pack_images([np.ascontiguousarray(J.as_rgb(c["pixels"])[:, :, ::-1]) for c in cs])
    want = ijb.align_faces(hbuf, hmeta, mats)
    assert got.shape == (4, 112, 112, 3) and torch.equal(got, want)
    assert int(got.float().std()) > 0


def test_load_bin(tmp_path):
    faces = _faces()
    seq = [faces[(5 * k + k // 4) % 4] for k in range(12)]
    issame = [True, False, True, True, False, False]
    path = tmp_path / "pairs.bin"
    with open(path, "wb") as f:
        pickle.dump(([np.frombuffer(c["data"], np.uint8) for c in seq], issame), f)
    (plain, flipped), same = verification.load_bin(str(path), (112, 112))
    assert same == issame and plain.shape == flipped.shape == (12, 3, 112, 112) and plain.dtype == torch.float32
    want = np.stack([J.as_rgb(c["pixels"]).transpose(2, 0, 1) for c in seq]).astype(np.float32)
    assert np.array_equal(plain.cpu().numpy(), want)
    assert np.array_equal(flipped.cpu().numpy(), want[:, :, :, ::-1])
    with open(path, "wb") as f:
        pickle.dump(([golden()[2]["17x23_420_q95_r0"]["data"]] * 2, [True]), f)
    with pytest.raises(NotImplementedError):
        verification.load_bin(str(path), (112, 112))
