"""GPU tests of the JPEG encoder (msml_amd/jpeg.py, csrc/jpeg_enc.hip): every case of tests/golden/g16_jpeg_enc.npz byte
for byte against what Pillow (libjpeg-turbo) wrote, in ONE mixed launch through the packed form; uniform tensors, RGB /
BGR / one channel, pitched sources; images wider than one tile with hundreds of restart intervals; repeatability; slots that are too small and sources that do not fit, inside guard
bands; the refusals of the C entry point; recompress against the decode of Pillow's bytes; and crops on the device
through write_faces, RecordFaceSource and decode_batch."""
import numpy as np
import pytest
import torch

from msml_amd import _lib, jpeg
from tests import jpeg_cases as J
from tests import jpeg_enc_cases as E
from tests.packed_cases import bands_untouched, guarded

pytestmark = pytest.mark.gpu
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        cases, _ = E.load_golden()
        _CACHE["g"] = (cases, {c["name"]: c for c in cases})
    return _CACHE["g"]


def uniform_faces():
    cases, _ = golden()
    cs = [c for c in cases if c["name"].startswith("uniform")]
    assert len(cs) == 4
    return cs


def encode_guarded(cases, caps=None, meta_edit=None, src_cut=0):
    """One packed launch of `cases` into guarded dst and workspace; the slots lie back to back with a canary byte 0xA5
    wherever the launch does not write.  -> (dst numpy, slots, length, status)."""
    src, meta = E.pack_sources(cases)
    if meta_edit is not None:
        meta = meta_edit(meta.copy())
    plan = jpeg.EncodePlan([c["source"].shape[:2] for c in cases], [c["quality"] for c in cases],
                           [c["sampling"] for c in cases], [c["restart"] for c in cases])
    caps = plan.bounds if caps is None else np.asarray(caps, np.int64)
    slots = np.stack([np.cumsum(caps) - caps, caps], 1)
    dwhole, dst = guarded(int(caps.sum()))
    wwhole, ws = guarded(plan.ws_bytes, 0x5C)
    srcd = torch.from_numpy(src[:src.size - src_cut]).cuda()
    length, status = jpeg.encode_into(plan, srcd, torch.from_numpy(meta).cuda(), dst, torch.from_numpy(slots).cuda(), ws=ws)
    torch.cuda.synchronize()
    assert bands_untouched(dwhole) and bands_untouched(wwhole, 0x5C)
    return dst.cpu().numpy(), slots, length.cpu().numpy(), status.cpu().numpy()


def streams_of(dst, slots, length):
    return [dst[o:o + l].tobytes() for o, l in zip(slots[:, 0], length)]


def test_whole_fixture_in_one_launch():
    """Mixed sizes, samplings, qualities and restart intervals in one call: every length and every byte is Pillow's."""
    cases, _ = golden()
    dst, slots, length, status = encode_guarded(cases)
    assert status.tolist() == [0] * len(cases)
    assert length.tolist() == [len(c["data"]) for c in cases]
    for c, s in zip(cases, streams_of(dst, slots, length)):
        assert s == c["data"], c["name"]
    # nothing behind a stream is written: the rest of every slot still holds the fill
    for (o, cap), l in zip(slots, length):
        assert (dst[o + l:o + cap] == 0xA5).all()


def test_uniform_tensor_rgb_and_bgr():
    cs = uniform_faces()
    rgb = torch.from_numpy(np.stack([c["source"] for c in cs])).cuda()
    enc = jpeg.encode_batch(rgb)                                         # the defaults are a bare save()'s
    assert enc.status.cpu().tolist() == [0] * 4 and len(enc) == 4
    assert enc.to_bytes() == [c["data"] for c in cs]
    assert enc.length.cpu().tolist() == [len(c["data"]) for c in cs]
    bgr = rgb.flip(-1).contiguous()
    assert jpeg.encode_batch(bgr, order="bgr").to_bytes() == [c["data"] for c in cs]
    assert jpeg.encode_batch(bgr).to_bytes() != [c["data"] for c in cs]
    _, by = golden()
    bare = by["face0_112x112_bare_420_q75_r0"]
    assert jpeg.encode_batch(torch.from_numpy(bare["source"][None]).cuda()).to_bytes() == [bare["data"]]
    # per-image options on a tensor
    two = jpeg.encode_batch(rgb[:2], quality=[75, 97], sampling=["420", "444"], restart=[0, 2]).to_bytes()
    assert two[0] == cs[0]["data"] and two[1] == E.encode(cs[1]["source"], "444", 97, 2)


def test_gray_tensor_and_pitched_source():
    cases, by = golden()
    gray = [c for c in cases if c["sampling"] == "gray" and c["source"].shape[:2] == (23, 17)]
    assert len(gray) == 4
    y = np.stack([E.rgb_to_ycc(c["source"])[0].astype(np.uint8) for c in gray])
    enc = jpeg.encode_batch(torch.from_numpy(y).cuda(), quality=[c["quality"] for c in gray],
                            restart=[c["restart"] for c in gray])
    assert enc.to_bytes() == [c["data"] for c in gray]
    with pytest.raises(ValueError):
        jpeg.encode_batch(torch.from_numpy(y).cuda(), sampling=["420"] * 4)
    # a source whose pitch is larger than its row, at an odd offset, between bytes that must not leak in
    c = by["33x17_420_q75_r3"]
    h, w = c["source"].shape[:2]
    pitch, off = 3 * w + 13, 5
    buf = np.full(off + h * pitch, 0xEE, np.uint8)
    rows = buf[off:off + h * pitch].reshape(h, pitch)
    rows[:, :3 * w] = c["source"].reshape(h, 3 * w)
    meta = np.array([[off, h, w, pitch]], np.int64)
    enc = jpeg.encode_batch((torch.from_numpy(buf).cuda(), meta), c["quality"], c["sampling"], c["restart"])
    assert enc.to_bytes() == [c["data"]]


def test_two_runs_give_identical_buffers():
    cases, _ = golden()
    a = encode_guarded(cases)
    b = encode_guarded(cases)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_slot_one_byte_too_small():
    cases, by = golden()
    pick = [by["uniform0_112x112_420_q75_r0"], by["mcu1_17x23_420_q75_r1"], by["uniform1_112x112_420_q75_r0"]]
    # in the middle: the neighbours are exact; at the end: the byte behind the slot is the guard band's
    for order in ([0, 1, 2], [0, 2, 1]):
        cs = [pick[i] for i in order]
        small = order.index(1)
        caps = [len(c["data"]) for c in cs]
        caps[small] -= 1
        dst, slots, length, status = encode_guarded(cs, caps)
        assert status.tolist() == [2 if i == small else 0 for i in range(3)]
        assert length.tolist() == [0 if i == small else len(c["data"]) for i, c in enumerate(cs)]
        got = streams_of(dst, slots, length)
        assert all(got[i] == cs[i]["data"] for i in range(3) if i != small)
    caps = [len(c["data"]) for c in pick]
    # the slot that just fits
    dst, slots, length, status = encode_guarded(pick, caps)
    assert status.tolist() == [0, 0, 0] and streams_of(dst, slots, length) == [c["data"] for c in pick]
    # a slot that is not inside dst: status, nothing written
    plan = jpeg.EncodePlan([pick[1]["source"].shape[:2]], 75, "420", 1)
    src, meta = E.pack_sources(pick[1:2])
    dwhole, dst = guarded(int(plan.bounds[0]))
    for slot in ([8, int(plan.bounds[0])], [-4, 64], [0, -1]):
        length, status = jpeg.encode_into(plan, torch.from_numpy(src).cuda(), torch.from_numpy(meta).cuda(), dst,
                                          torch.tensor([slot], dtype=torch.int64, device="cuda"))
        assert (length.item(), status.item()) == (0, 2)
    assert bands_untouched(dwhole) and (dst == 0xA5).all()
    with pytest.raises(ValueError, match="image 0"):
        jpeg.encode_batch(torch.from_numpy(pick[0]["source"][None]).cuda(), slot_bytes=1000).to_bytes()


def test_meta_row_that_does_not_fit():
    cases, by = golden()
    pick = [by["uniform0_112x112_420_q75_r0"], by["17x23_422_q75_r3"], by["uniform1_112x112_420_q75_r0"]]

    def wider(meta):
        meta[1, 2] += 1                                                  # W that is not the descriptor's
        return meta
    dst, slots, length, status = encode_guarded(pick, meta_edit=wider)
    assert status.tolist() == [0, 1, 0] and length[1] == 0
    got = streams_of(dst, slots, length)
    assert got[0] == pick[0]["data"] and got[2] == pick[2]["data"]
    assert (dst[slots[1, 0]:slots[1, 0] + slots[1, 1]] == 0xA5).all()
    # the last image ends one byte past the source buffer
    dst, slots, length, status = encode_guarded(pick, src_cut=3)       # pitch 336 = 3 * 112: no padding behind the last row
    assert status.tolist() == [0, 0, 1] and length[2] == 0

    def negative(meta):
        meta[0, 0] = -8
        meta[1, 3] = 3 * meta[1, 2] - 1                                  # a pitch shorter than the row
        return meta
    _, _, length, status = encode_guarded(pick, meta_edit=negative)
    assert status.tolist() == [1, 1, 0] and length.tolist()[:2] == [0, 0]


def test_abi_errors():
    cases, by = golden()
    pick = [by["uniform0_112x112_420_q75_r0"], by["mcu1_17x23_420_q75_r1"]]
    src, meta = E.pack_sources(pick)
    plan = jpeg.EncodePlan([c["source"].shape[:2] for c in pick], 75, "420", [0, 1])
    desc, qt, hd = plan.to_device(torch.device("cuda", 0))
    srcd, mdev = torch.from_numpy(src).cuda(), torch.from_numpy(meta).cuda()
    slots = np.stack([np.cumsum(plan.bounds) - plan.bounds, plan.bounds], 1)
    sdev = torch.from_numpy(slots).cuda()
    dst = torch.zeros(int(plan.bounds.sum()), dtype=torch.uint8, device="cuda")
    ws = torch.zeros(plan.ws_bytes + 16, dtype=torch.uint8, device="cuda")
    length = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    host = plan.desc.clone()

    def run(**kw):
        a = dict(src=srcd, sb=srcd.numel(), meta=mdev, ch=3, swap=0, desc=desc, host=host.data_ptr(), qt=qt, nq=qt.shape[0],
                 hd=hd, hb=hd.numel(), dst=dst, db=dst.numel(), slots=sdev, length=length, status=status, ws=ws,
                 wb=plan.ws_bytes, n=2)
        a.update(kw)
        return _lib.call_status("msml_jpeg_encode", *a.values())

    def with_desc(row, word, v):
        h = plan.desc.clone()
        h[row, word] = v
        return run(host=h.data_ptr()), h

    SHAPE, UNSUP, WORKSPACE = -1, -4, -5
    for name in ("src", "meta", "desc", "host", "qt", "hd", "dst", "slots", "length", "status", "ws"):
        assert run(**{name: None}) == SHAPE, name
    assert run(ws=ws.data_ptr() + 4) == SHAPE and run(meta=mdev.data_ptr() + 4) == SHAPE
    assert run(slots=sdev.data_ptr() + 4) == SHAPE and run(status=status.data_ptr() + 2) == SHAPE
    assert run(length=length.data_ptr() + 2) == SHAPE and run(qt=qt.data_ptr() + 2) == SHAPE
    assert run(n=0) == UNSUP and run(n=-1) == UNSUP and run(n=65536) == UNSUP
    assert run(ch=2) == UNSUP and run(ch=1) == UNSUP                      # a colour sampling from one channel
    assert with_desc(1, jpeg.JE_SAMP, 4)[0] == UNSUP and with_desc(1, jpeg.JE_SAMP, -1)[0] == UNSUP
    assert with_desc(0, jpeg.JE_H, 0)[0] == UNSUP and with_desc(0, jpeg.JE_W, 32768)[0] == UNSUP
    assert run(wb=plan.ws_bytes - 1) == WORKSPACE and run(wb=0) == WORKSPACE
    assert run(nq=1) == SHAPE                                             # a table selector past the tables
    assert run(hb=hd.numel() - 8) == SHAPE                                # a header past the header bytes
    assert with_desc(1, jpeg.JE_RI, 65536)[0] == SHAPE and with_desc(1, jpeg.JE_WS, 0)[0] == SHAPE
    assert "jpeg_encode" in _lib.load().msml_last_error().decode()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [-7, -7] and length.cpu().tolist() == [-7, -7] and int(dst.sum()) == 0   # before any launch
    assert _lib.value("msml_jpeg_encode_workspace", None, 2) == 0 and _lib.value("msml_jpeg_encode_workspace", host.data_ptr(), 0) == 0
    assert run() == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0] and length.cpu().tolist() == [len(c["data"]) for c in pick]


def test_recompress_equals_decode_of_pillows_bytes():
    cases, _ = golden()
    faces = [c for c in cases if c["source"].shape[:2] == (112, 112)]
    assert len(faces) == 9
    groups = {}
    for c in faces:
        if c["restart"] == 0:
            groups.setdefault((c["quality"], c["sampling"]), []).append(c)
    assert sum(len(g) for g in groups.values()) >= 7
    for (q, s), g in groups.items():
        x = torch.from_numpy(np.stack([c["source"] for c in g])).cuda()
        want = np.stack([J.as_rgb(J.decode(c["data"])) for c in g])
        if s == "gray":                                                   # one channel in, one channel out
            y = torch.from_numpy(np.stack([E.rgb_to_ycc(c["source"])[0].astype(np.uint8) for c in g])).cuda()
            out = jpeg.recompress(y, q, s)
            assert out.shape == y.shape and np.array_equal(out.cpu().numpy(), want[..., 0])
            continue
        out = jpeg.recompress(x, q, s)
        assert out.shape == x.shape and out.dtype == torch.uint8
        assert np.array_equal(out.cpu().numpy(), want), (q, s)
        back = jpeg.recompress(x.flip(-1).contiguous(), q, s, order="bgr")
        assert np.array_equal(back.cpu().numpy(), want[..., ::-1])
    # the streams with restart markers too, through encode + decode_batch
    rest = [c for c in faces if c["restart"]]
    for c in rest:
        enc = jpeg.encode_batch(torch.from_numpy(c["source"][None]).cuda(), c["quality"], c["sampling"], c["restart"])
        out = jpeg.decode_batch(enc.to_bytes(), size=(112, 112))
        assert np.array_equal(out[0].cpu().numpy(), J.as_rgb(J.decode(c["data"])))


def test_crops_to_records_and_back(tmp_path):
    """align_multi-shaped input (uint8 [N][112][112][3] on the device) -> encode -> write_faces -> RecordFaceSource ->
    decode_batch: the pixels recompress gives, the labels, and record 0."""
    cs = uniform_faces()
    crops = torch.from_numpy(np.stack([c["source"] for c in cs] * 2)).cuda()          # 8 crops
    labels = [3, 1, 4, 1, 5, 9, 2, 6]
    with jpeg.RecordWriter(str(tmp_path / "train.rec"), str(tmp_path / "train.idx")) as w:
        nxt = jpeg.write_faces(w, jpeg.encode_batch(crops[:4], quality=97), labels[:4], 1, header0=(8, 10))
        assert nxt == 5
        assert jpeg.write_faces(w, jpeg.encode_batch(crops[4:], quality=97), torch.tensor(labels[4:]), nxt) == 9
    want = jpeg.recompress(crops, quality=97)
    assert not torch.equal(want, crops)
    with jpeg.RecordFaceSource(str(tmp_path), 4, steps=2) as src:
        assert src.rec.header0 == (9, 10)
        got, seen = [], []
        for batch, lab in src:
            got.append(jpeg.decode_batch(batch, size=(112, 112)))
            seen += lab.tolist()
    assert seen == labels and torch.equal(torch.cat(got), want)
    with jpeg.RecordFile(str(tmp_path / "train.rec"), str(tmp_path / "train.idx")) as f:
        assert f.read_idx(1)[1] == E.encode(cs[0]["source"], "420", 97)


def test_wide_images_and_many_intervals():
    """Sizes past one tile per MCU row in every sampling (more than 32 / 16 / 16 / 8 MCUs across), more than 256 restart
    intervals and more than 256 blocks in one image (several rounds of the scans), against the numpy restatement that
    the CPU tests pin to Pillow."""
    rng = np.random.RandomState(1616)

    def image(h, w):
        y, x = np.mgrid[:h, :w]
        a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) % 256], -1) + rng.randint(-20, 21, (h, w, 3))
        return np.clip(a, 0, 255).astype(np.uint8)
    cs = [{"source": image(136, 136), "sampling": "444", "quality": 75, "restart": 1},      # 289 MCUs = 289 intervals
          {"source": image(20, 300), "sampling": "420", "quality": 95, "restart": 0},       # 19 MCUs across
          {"source": image(9, 300), "sampling": "gray", "quality": 50, "restart": 5},       # 38 across
          {"source": image(17, 260), "sampling": "422", "quality": 100, "restart": 4}]      # 17 across
    for c in cs:
        c["data"] = E.encode(c["source"], c["sampling"], c["quality"], c["restart"])
    dst, slots, length, status = encode_guarded(cs)
    assert status.tolist() == [0] * 4 and length.tolist() == [len(c["data"]) for c in cs]
    assert streams_of(dst, slots, length) == [c["data"] for c in cs]
