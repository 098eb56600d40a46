"""GPU tests of progressive JPEG decoding (msml_amd/jpeg.py progressive=True, csrc/jpeg.hip k_jpeg_prog): every stream
of tests/golden/g18_jpeg_prog.npz bit for bit against the pixels Pillow (libjpeg-turbo) recorded, in one mixed-size
packed launch inside guard bands and in uniform launches; baseline and progressive streams alternating in one batch;
the coefficient workspace of the padded-plane cases against the restatement (tests/jpeg_prog_cases.py); a 1024 x 1024
stream whose AC scans are nothing but maximal end-of-band runs; the refusals; the mutations the host check recorded
(g18_jpeg_prog_corrupt.npz, tools/jpeg_prog_hostcheck.cpp) with the host's statuses; and the two folder doors."""
import io

import numpy as np
import pytest
import torch

from msml_amd import imageio, jpeg, verification
from tests import jpeg_cases as J
from tests import jpeg_prog_cases as P
from tests.packed_cases import bands_untouched, batch_sizes, guarded, packed_meta, unpack

pytestmark = pytest.mark.gpu
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        cases, _ = P.load_golden()
        _CACHE["g"] = (cases, {c["name"]: c for c in cases})
    return _CACHE["g"]


def baseline():
    if "b" not in _CACHE:
        _CACHE["b"] = [c for c in J.load_golden()[0] if c["supported"]]
    return _CACHE["b"]


def decode_guarded(streams, channels=3, order="rgb", batch=None):
    """One packed launch into guarded dst and workspace -> ((buf, meta), status numpy, ws); asserts the guard bands."""
    if batch is None:
        batch = jpeg.pack_jpegs(streams, progressive=True)
    meta, total = packed_meta(batch_sizes(batch), channels)
    dwhole, dst = guarded(total)
    wwhole, ws = guarded(batch.ws_bytes, 0x5C)
    status = jpeg.decode_into(batch, dst, meta, channels, order, ws=ws, progressive=True)
    torch.cuda.synchronize()
    assert bands_untouched(dwhole) and bands_untouched(wwhole, 0x5C)
    return (dst, meta), status.cpu().numpy(), ws


def test_bit_exact_mixed_sizes_one_launch():
    cases, _ = golden()
    assert len(cases) >= 50
    for order in ("rgb", "bgr"):
        (buf, meta), status, _ = decode_guarded([c["data"] for c in cases], 3, order)
        assert (status == 0).all(), status
        for c, img in zip(cases, unpack(buf, meta)):
            want = J.as_rgb(c["pixels"])
            assert np.array_equal(img, want if order == "rgb" else want[:, :, ::-1]), (order, c["name"])
    gray = [c for c in cases if c["pixels"].ndim == 2]
    assert len(gray) >= 10
    (buf, meta), status, _ = decode_guarded([c["data"] for c in gray], 1)
    assert (status == 0).all()
    for c, img in zip(gray, unpack(buf, meta, 1)):
        assert np.array_equal(img, c["pixels"]), c["name"]


def test_bit_exact_uniform_launches():
    cases, _ = golden()
    groups = {}
    for c in cases:
        groups.setdefault(c["pixels"].shape[:2], []).append(c)
    assert len(groups) >= 9
    for (h, w), cs in groups.items():
        out = jpeg.decode_batch([c["data"] for c in cs], size=(h, w), progressive=True)
        assert out.shape == (len(cs), h, w, 3) and out.dtype == torch.uint8
        for c, img in zip(cs, out.cpu().numpy()):
            assert np.array_equal(img, J.as_rgb(c["pixels"])), c["name"]
        g = [c for c in cs if c["pixels"].ndim == 2]
        if g:
            out = jpeg.decode_batch([c["data"] for c in g], size=(h, w), channels=1, progressive=True)
            for c, img in zip(g, out.cpu().numpy()):
                assert np.array_equal(img, c["pixels"]), c["name"]
    # the default still refuses them
    with pytest.raises(ValueError, match="progressive JPEG is unsupported"):
        jpeg.decode_batch([cases[0]["data"]])


@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_baseline_and_progressive_alternate(n):
    """Baseline and progressive streams in turn, 112 x 112 among tiny ones: every image is that of its own stream
    wherever it stands, and two runs give the same bits."""
    cases, _ = golden()
    base = baseline()
    pools = {False: ([c for c in base if "112x112" in c["name"]], [c for c in base if c["name"].startswith(("1x1_", "9x1_"))]),
             True: ([c for c in cases if "112x112" in c["name"]], [c for c in cases if c["name"].startswith(("1x1_", "9x1_", "5x2_"))])}
    seq = []
    for i in range(n):
        big, tiny = pools[i % 2 == 1 if n > 1 else True]
        seq.append(big[(i // 4) % len(big)] if (i // 2) % 2 == 0 else tiny[(5 * i) % len(tiny)])
    (buf, meta), status, _ = decode_guarded([c["data"] for c in seq])
    assert (status == 0).all(), status
    for c, img in zip(seq, unpack(buf, meta)):
        assert np.array_equal(img, J.as_rgb(c["pixels"])), c["name"]
    (buf2, _), _, _ = decode_guarded([c["data"] for c in seq])
    assert torch.equal(buf, buf2)


def test_padded_planes_hold_the_restatements_coefficients():
    """17 x 23 4:2:0 (3 x 3 luma blocks of its own in a 4 x 4 plane) and 9 x 1: the whole coefficient workspace, own and
    padding blocks, against the restatement -- a padding block keeps the DC of the interleaved scan and zero AC."""
    cases, _ = golden()
    picked = [c for c in cases if c["name"].startswith(("17x23_420_", "9x1_", "w_dc1_17x23_420", "w_deep_9x1_422"))]
    assert len(picked) >= 7
    batch = jpeg.pack_jpegs([c["data"] for c in picked], progressive=True)
    (buf, meta), status, ws = decode_guarded(None, batch=batch)
    assert (status == 0).all()
    wsn = ws.cpu().numpy()
    padded = 0
    for i, c in enumerate(picked):
        coefs, d = P.coefficients(c["data"])
        at = int(batch.desc.numpy()[i, jpeg.JD_WS]) * 256
        for comp in coefs:
            n = comp.shape[0] * comp.shape[1] * 64
            got = wsn[at:at + 2 * n].view(np.int16).reshape(comp.shape)
            assert np.array_equal(got, comp), c["name"]
            at += 2 * n
        for k, comp in enumerate(coefs):
            oh, ow = P.own_blocks(d, k)
            pad = np.ones(comp.shape[:2], bool)
            pad[:oh, :ow] = False
            padded += int(pad.sum())
            assert not comp[pad][:, 1:].any()
    assert padded >= 7
    for c, img in zip(picked, unpack(buf, meta)):
        assert np.array_equal(img, J.as_rgb(c["pixels"])), c["name"]


def test_maximal_eobruns_1024():
    """1024 x 1024 gray with zero AC: both AC scans are one EOB14 run over all 16384 blocks.  Expected: the baseline
    kernel on the baseline stream of the same coefficients."""
    d = jpeg.JpegDescriptor()
    d.height = d.width = 1024
    d.components, d.sampling, d.qsel, d.qtables = 1, ((1, 1),), (0,), {0: jpeg.quant_tables(75)[0]}
    coef = np.zeros((128 * 128, 64), np.int64)
    coef[:, 0] = (np.arange(128 * 128) * 11 % 61) - 30
    coefs = [coef.reshape(128, 128, 64)]
    script = [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    prog, base = P.write_progressive(coefs, d, script), P.write_baseline(coefs, d)
    dp = jpeg.parse_jpeg(prog, progressive=True)
    assert dp.status == 0 and [s.end - s.begin for s in dp.scans][1::2] == [2, 2]      # EOB14 + 14 zero bits, padded
    want = jpeg.decode_batch([base], size=(1024, 1024), channels=1)
    got = jpeg.decode_batch([prog], size=(1024, 1024), channels=1, progressive=True)
    assert torch.equal(got, want) and int(want.max()) > int(want.min())


def test_refusals(monkeypatch):
    cases, by = golden()
    c = by[next(n for n in by if n.startswith("17x23_420_"))]
    head, ch = P.split_scans(c["data"])
    incomplete = P.join_scans(head, ch[:-1])
    invalid = P.join_scans(head, ch[:5] + ch[6:])                    # the 2 -> 1 refinement of luma skipped
    assert jpeg.parse_jpeg(incomplete, True).status == jpeg.INCOMPLETE
    assert jpeg.parse_jpeg(invalid, True).status == jpeg.PROGRESSION
    base = baseline()[40]
    mixed = [c["data"], incomplete, base["data"], invalid, cases[-2]["data"]]
    buf, meta, status = jpeg.decode_batch(mixed, strict=False, progressive=True)
    assert status.cpu().tolist() == [0, jpeg.INCOMPLETE, 0, jpeg.PROGRESSION, 0]
    imgs = unpack(buf, meta, check_pad=False)
    for i, want in ((0, c), (2, base), (4, cases[-2])):
        assert np.array_equal(imgs[i], J.as_rgb(want["pixels"]))
    with pytest.raises(ValueError, match="image 1: an incomplete progression"):
        jpeg.decode_batch(mixed, progressive=True)

    def no_call(*a, **k):
        raise AssertionError("a launch for a batch without a supported stream")

    monkeypatch.setattr(jpeg, "call", no_call)
    _, _, status = jpeg.decode_batch([incomplete, invalid], strict=False, progressive=True)
    assert status.cpu().tolist() == [jpeg.INCOMPLETE, jpeg.PROGRESSION]


def test_corrupt_streams_as_the_host_check():
    """Only inputs tools/jpeg_prog_hostcheck.cpp has decoded on the host under the sanitizers, handed over as it got
    them (stream bytes and scan records): the device gives the host's statuses, the clean neighbours are bit-exact, the
    guard bands intact.  Records the host's checks refused (-1) make the entry point refuse the call."""
    cases, by = golden()
    rec = P.load_corrupt()
    assert len(rec) >= 300 and {r[0] for r in rec} == {"subst", "ffxx", "trunc", "drop", "swap", "seltab", "scanhdr"}
    assert sum(r[4] > 0 for r in rec) >= 100 and {r[4] for r in rec} >= {-1, 0, 1, 2, 5}
    run = [r for r in rec if r[4] >= 0]
    # the records name Huffman tables by their index in the host check's batch, which packed the fixture in order: the
    # fixture's streams go first here, so that every table keeps its index; they are the clean neighbours as well
    clean, patches, expect = [c["data"] for c in cases], [], [None] * len(cases)
    for r in run:
        patches.append((len(clean), r[5], r[6]))
        clean.append(cases[r[1]]["data"])
        expect.append(r[4])
    assert jpeg.pack_jpegs(clean, progressive=True).htabs.shape[0] == \
        jpeg.pack_jpegs(clean[:len(cases)], progressive=True).htabs.shape[0]
    (buf, meta), status, _ = decode_guarded(None, batch=P.corrupt_batch(clean, patches))
    imgs = unpack(buf, meta, check_pad=False)
    for i, (e, st) in enumerate(zip(expect, status)):
        if e is None:
            assert st == 0 and np.array_equal(imgs[i], J.as_rgb(cases[i]["pixels"])), cases[i]["name"]
        else:
            assert st == e, (i, run[i - len(cases)][:5], st)
    refused = next(r for r in rec if r[4] == -1)
    n = len(cases)
    batch = P.corrupt_batch(clean[:n] + [cases[refused[1]]["data"]], [(n, refused[5], refused[6])])
    meta, total = packed_meta(batch_sizes(batch))
    dst = torch.zeros(total, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="scan records of image %d" % n):
        jpeg.decode_into(batch, dst, meta)


def test_folder_doors(tmp_path):
    """imageio.decode_images and verification.load_folder over baseline JPEG, progressive JPEG and PNG files."""
    Image = pytest.importorskip("PIL.Image")
    cases, by = golden()
    prog = [by["face0_112x112_420_q95_r1"], cases[6], by["face3_112x112_gray_q95_r0"]]
    base = baseline()[33]
    png = io.BytesIO()
    Image.fromarray(J.as_rgb(prog[1]["pixels"])).save(png, "PNG")
    blobs = [prog[0]["data"], base["data"], png.getvalue(), prog[1]["data"], prog[2]["data"]]
    want = [J.as_rgb(c["pixels"]) for c in (prog[0], base, prog[1], prog[1], prog[2])]
    buf, meta = imageio.decode_images(blobs, progressive=True)
    for img, w in zip(unpack(buf, meta), want):
        assert np.array_equal(img, w)
    with pytest.raises(imageio.DecodeError, match="image 0: progressive JPEG is unsupported"):
        imageio.decode_images(blobs)
    for ident, names in (("anna", (0, 1, 2)), ("ben", (3, 4))):
        (tmp_path / ident).mkdir()
        for k in names:
            (tmp_path / ident / ("%d.%s" % (k, "png" if k == 2 else "jpg"))).write_bytes(blobs[k])
    files, buf, meta = verification.load_folder(str(tmp_path), progressive=True)
    assert files == {"anna": ["0.jpg", "1.jpg", "2.png"], "ben": ["3.jpg", "4.jpg"]}
    for img, w in zip(unpack(buf, meta), want):
        assert np.array_equal(img, w)
    with pytest.raises(ValueError, match="0.jpg"):
        verification.load_folder(str(tmp_path))
