"""GPU tests of the PNG encoder (msml_amd/png.py encode_batch / encode_into, csrc/png_enc.hip): every file is read back by
three readers (Pillow, zlib against the numpy restatement's filtered bytes, msml_png_decode); statuses, neighbours and
canaries around images that do not fit; determinism over repeats and batch compositions; sizes against references that do
not involve the encoder (tests/png_enc_cases.py); and the doors (imageio, verification.save_folder, write_faces).

Sizes on the MI355X (test_sizes_of_the_faces prints them; recorded in DESIGN.md section 5)."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from msml_amd import imageio, jpeg, png, verification
from tests import png_enc_cases as E
from tests.packed_cases import bands_untouched, canaries_intact, guarded, packed_meta, unpack

pytestmark = pytest.mark.gpu
_CACHE = {}
FILTERS = ("adaptive", "none", "paeth")


def cases():
    """name -> [H, W, C] array: the fixture (faces, the decoded PNG fixtures, the synthetic shapes) and the two images
    whose rows repeat at distance 32768 (gray, 32767 wide) and 32769 (gray + alpha, 16384 wide: sizes end at 32767, so
    a one-channel image with that row distance, 32768 wide, does not exist)."""
    if "cases" not in _CACHE:
        c = {k: E.as_hwc(v) for k, v in E.load_golden().items()}
        c["tall32768"] = E.tall(32767, 1)
        c["tall32769"] = E.tall(16384, 2)
        _CACHE["cases"] = c
    return _CACHE["cases"]


def names_for(flt):
    return [k for k in cases() if not k.startswith("tall") or flt == "none"]


def pack_sources(arrays, channels, fill=0xA5):
    """The packed (buf, meta) of arrays with `channels` each: pitch = row bytes + 5, 32 canary bytes between images."""
    meta, total = packed_meta([a.shape[:2] for a in arrays], channels, gap=32, pitch_extra=5)
    buf = np.full(total, fill, np.uint8)
    for a, (off, h, w, pitch) in zip(arrays, meta):
        rows = buf[off:off + h * pitch].reshape(h, pitch)
        rows[:, :w * channels] = a.reshape(h, w * channels)
    return buf, meta


def encode_guarded(arrays, channels, flt="adaptive", order="rgb", caps=None, meta_edit=None, slots_edit=None):
    """One launch of arrays (one channel count) through the packed form into guarded dst and workspace; the slots lie
    back to back with 16 canary bytes between them.  -> (files or None per image, length, status, slots)."""
    src, meta = pack_sources(arrays, channels)
    if meta_edit is not None:
        meta = meta_edit(meta.copy())
    plan = png.PngEncodePlan([a.shape[:2] for a in arrays], channels)
    caps = plan.bounds if caps is None else np.asarray(caps, np.int64)
    offs = np.cumsum(caps + 16) - (caps + 16)
    slots = np.stack([offs, caps], 1)
    if slots_edit is not None:
        slots = slots_edit(slots.copy())
    dwhole, dst = guarded(int((caps + 16).sum()))
    wwhole, ws = guarded(plan.ws_bytes, 0x5C)
    length, status = png.encode_into(torch.from_numpy(src).cuda(), torch.from_numpy(meta).cuda(), dst,
                                     torch.from_numpy(slots).cuda(), channels, order, flt, ws=ws, plan=plan)
    torch.cuda.synchronize()
    assert bands_untouched(dwhole) and bands_untouched(wwhole, 0x5C)
    host, length, status = dst.cpu().numpy(), length.cpu().numpy(), status.cpu().numpy()
    used = np.zeros(host.size, bool)
    for (o, c), l in zip(np.stack([offs, caps], 1), length):
        used[o:o + c] = True                                 # the tail of a slot behind `length` is the encoder's to use
    assert (host[~used] == 0xA5).all(), "canary bytes between the slots"
    files = [host[o:o + l].tobytes() if s == 0 else None for (o, _), l, s in zip(slots, length, status)]
    return files, length, status, slots


def encoded(flt):
    """name -> file for every case under one filter: one launch per channel count, shared by the tests."""
    key = ("enc", flt)
    if key not in _CACHE:
        out = {}
        for ch in (1, 2, 3, 4):
            ns = [k for k in names_for(flt) if cases()[k].shape[2] == ch]
            files, length, status, _ = encode_guarded([cases()[k] for k in ns], ch, flt)
            assert status.tolist() == [0] * len(ns), dict(zip(ns, status.tolist()))
            out.update(zip(ns, files))
        _CACHE[key] = out
    return _CACHE[key]


def filtered(name, flt):
    key = ("filt", name, flt)
    if key not in _CACHE:
        _CACHE[key] = E.filtered_bytes(cases()[name], flt)
    return _CACHE[key]


@pytest.mark.parametrize("flt", FILTERS)
def test_round_trip_three_readers(flt):
    """Pillow verifies the CRCs and returns the pixels; zlib inflates the IDAT payload to the restatement's filtered
    bytes (the filter choice and the Adler-32); msml_png_decode returns the source; nothing passes the bound."""
    files = encoded(flt)
    modes = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
    for name in names_for(flt):
        a, data = cases()[name], files[name]
        assert len(data) <= E.bound(*a.shape) == png.encode_bound(*a.shape), name
        Image.open(io.BytesIO(data)).verify()
        im = Image.open(io.BytesIO(data))
        assert im.mode == modes[a.shape[2]] and np.array_equal(E.as_hwc(np.asarray(im)), a), name
        assert zlib.decompress(E.idat_of(data)) == filtered(name, flt), name
    for ch in (1, 2, 3, 4):
        ns = [k for k in names_for(flt) if cases()[k].shape[2] == ch]
        dch = 4 if ch == 2 else ch                           # gray + alpha reads back as RGBA
        buf, meta = png.decode_batch(png.pack_pngs([files[k] for k in ns]), channels=dch)
        for k, got in zip(ns, unpack(buf, meta, dch, check_pad=False)):
            a = cases()[k]
            want = a if ch != 2 else np.concatenate([a[..., :1]] * 3 + [a[..., 1:]], axis=2)
            assert np.array_equal(E.as_hwc(got), want), k


def test_bgr_sources():
    """order="bgr": B, G, R(, A) sources give the file of the R, G, B(, A) image."""
    for ch in (3, 4):
        ns = [k for k in ("face0", "rgba7x5", "s1x300x3", "s300x1x4", "png_rgba_113x111_cycle") if cases()[k].shape[2] == ch]
        perm = [2, 1, 0] + ([3] if ch == 4 else [])
        files, _, status, _ = encode_guarded([np.ascontiguousarray(cases()[k][..., perm]) for k in ns], ch, order="bgr")
        assert status.tolist() == [0] * len(ns) and files == [encoded("adaptive")[k] for k in ns]


@pytest.mark.parametrize("flt", FILTERS)
def test_sizes_against_references(flt):
    """(a) every file is within what "dynamic, literals only" with the most expensive header costs under the optimal
    15-bit-limited code of its filtered bytes (E.size_limit states the allowance for blocks of 65535 bytes); (b) the flat
    image and the image of identical rows take less than n / 16, which a coder without matches cannot reach (n / 8);
    of the 3-row image whose rows repeat at distance 32768, the two later rows take less than n / 16 on top of a first
    row that is stored at worst."""
    files = encoded(flt)
    for name in names_for(flt):
        f = filtered(name, flt)
        assert len(files[name]) <= E.size_limit(f), (name, len(files[name]), E.size_limit(f))
    for name in ("flat", "rows"):
        n = len(filtered(name, flt))
        assert len(files[name]) < n / 16, (name, len(files[name]), n)
    if flt == "none":
        n = len(filtered("tall32768", flt))
        assert len(files["tall32768"]) < n / 3 + n / 16, (len(files["tall32768"]), n)


def test_sizes_of_the_faces():
    """(c) a record, not a threshold: the four faces against Pillow's default save and zlib level 1 of the same filtered
    bytes."""
    ns = ["face%d" % i for i in range(4)]
    ours = sum(len(encoded("adaptive")[k]) for k in ns)
    pil = 0
    for k in ns:
        b = io.BytesIO()
        Image.fromarray(cases()[k]).save(b, "PNG")
        pil += len(b.getvalue())
    z1 = sum(len(zlib.compress(filtered(k, "adaptive"), 1)) + 57 for k in ns)
    raw = sum(cases()[k].size for k in ns)
    print("png_enc faces: device %d bytes, Pillow %d, zlib level 1 %d, raw %d: device / Pillow %.3f, device / level 1 %.3f"
          % (ours, pil, z1, raw, ours / pil, ours / z1))
    assert ours < raw


def test_containment():
    """A slot that is too small (2), a meta row outside src (1), a slot outside dst (2): each sets its status and length
    0, the neighbours' files are those of the clean batch, canaries and guard bands hold (encode_guarded asserts them)."""
    ns = ["face0", "rows", "face1", "noise"]
    arrays = [cases()[k] for k in ns]
    clean, length, status, slots = encode_guarded(arrays, 3)
    assert status.tolist() == [0, 0, 0, 0] and clean == [encoded("adaptive")[k] for k in ns]

    caps = png.PngEncodePlan([a.shape[:2] for a in arrays], 3).bounds.copy()
    caps[1] = (len(clean[1]) - 1) & ~3                       # one byte short, rounded down
    files, length, status, _ = encode_guarded(arrays, 3, caps=caps)
    assert status.tolist() == [0, 2, 0, 0] and length[1] == 0
    assert [files[i] for i in (0, 2, 3)] == [clean[i] for i in (0, 2, 3)]

    def beyond(meta):
        meta[2, 0] = meta[3, 0] + meta[3, 1] * meta[3, 3] - 64   # image 2 would end far behind the buffer
        return meta
    files, length, status, _ = encode_guarded(arrays, 3, meta_edit=beyond)
    assert status.tolist() == [0, 0, 1, 0] and length[2] == 0
    assert [files[i] for i in (0, 1, 3)] == [clean[i] for i in (0, 1, 3)]

    def outside(s):
        s[0, 0] = s[3, 0] + s[3, 1]                          # starts inside dst, ends behind it
        return s
    files, length, status, _ = encode_guarded(arrays, 3, slots_edit=outside)
    assert status.tolist() == [2, 0, 0, 0] and length[0] == 0
    assert files[1:] == clean[1:]


def test_determinism_and_batch_composition():
    """The same batch twice, reversed, and split into two calls: identical bytes per image."""
    ns = ["face0", "rows", "flat", "noise", "face3", "s1x300x3", "png_rgb_150x150_level0"]
    arrays = [cases()[k] for k in ns]
    first = encode_guarded(arrays, 3)[0]
    assert encode_guarded(arrays, 3)[0] == first
    assert encode_guarded(arrays[::-1], 3)[0][::-1] == first
    assert encode_guarded(arrays[:3], 3)[0] + encode_guarded(arrays[3:], 3)[0] == first
    assert first == [encoded("adaptive")[k] for k in ns]


def test_encode_batch_tensors():
    """The tensor forms of encode_batch: [N, H, W, C] for C 2..4 and [N, H, W], default slots, to_bytes."""
    for ch, ns in ((3, ["face0", "face1", "face2", "face3"]), (1, ["s1x300x1"]), (2, ["s300x1x2"]), (4, ["rgba7x5"])):
        x = torch.from_numpy(np.stack([cases()[k] for k in ns])).cuda()
        enc = png.encode_batch(x[..., 0] if ch == 1 else x)
        assert isinstance(enc, jpeg.EncodedBatch) and isinstance(enc.plan, png.PngEncodePlan)
        assert enc.to_bytes() == [encoded("adaptive")[k] for k in ns]
    with pytest.raises(ValueError):
        png.encode_batch(torch.from_numpy(cases()["face0"][None]).cuda(), slot_bytes=1000).to_bytes()


def test_doors(tmp_path):
    """imageio.encode_images with mixed formats gives the bytes of the two codecs called on their rows; save_folder
    followed by load_folder returns the tensors (PNG names) and jpeg.recompress's pixels (JPEG names); a PNG write_faces
    -> RecordFaceSource(raw=True) -> imageio.decode_images round trip returns the tensors."""
    ns = ["face0", "face1", "face2", "face3"]
    x = torch.from_numpy(np.stack([cases()[k] for k in ns])).cuda()
    mixed = imageio.encode_images(x, ["png", ".jpg", "a/b.PNG", "jpeg"], quality=90).to_bytes()
    assert [mixed[0], mixed[2]] == png.encode_batch(x[[0, 2]]).to_bytes()
    assert [mixed[1], mixed[3]] == jpeg.encode_batch(x[[1, 3]], quality=90).to_bytes()
    assert imageio.encode_images(x, "png").to_bytes() == [encoded("adaptive")[k] for k in ns]
    with pytest.raises(ValueError):
        imageio.encode_images(x, "bmp")

    names = [("id0", "a.png"), ("id0", "b.jpg"), "id1/a.png", "id1/b.png"]
    paths = verification.save_folder(str(tmp_path / "faces"), names, x, quality=90)
    assert [p[-9:] for p in paths] == ["id0/a.png", "id0/b.jpg", "id1/a.png", "id1/b.png"]
    files, buf, meta = verification.load_folder(str(tmp_path / "faces"))
    assert files == {"id0": ["a.png", "b.jpg"], "id1": ["a.png", "b.png"]}
    got = unpack(buf, meta, 3, check_pad=False)
    want = x.cpu().numpy()
    lossy = jpeg.recompress(x[1:2], quality=90).cpu().numpy()[0]
    for k, (g, w) in enumerate(zip(got, [want[0], lossy, want[2], want[3]])):
        assert np.array_equal(g, w), k

    labels = [3, 1, 4, 1]
    with jpeg.RecordWriter(str(tmp_path / "train.rec"), str(tmp_path / "train.idx")) as w:
        assert jpeg.write_faces(w, png.encode_batch(x), labels, 1, header0=(4, 10)) == 5
    with jpeg.RecordFaceSource(str(tmp_path), 4, steps=1, raw=True) as src:
        for blobs, lab in src:
            assert lab.tolist() == labels and blobs == [encoded("adaptive")[k] for k in ns]
            buf, meta = imageio.decode_images(blobs)
            assert all(np.array_equal(g, w) for g, w in zip(unpack(buf, meta, 3, check_pad=False), want))
