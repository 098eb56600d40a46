"""GPU tests of the test.py evaluation inputs (msml_eval_pairs, csrc/evalin.hip) against the PIL restatement of
tests/sweep_cases.py, bit for bit, and of the driver around it (msml_amd.verification.eval_pairs / extract_sum /
occlusion_sweep) against the same steps composed by hand.  What is NOT shown here: equality with a torchvision build
(none was available; see tests/sweep_cases.py)."""
import numpy as np
import pytest
import torch

from tests import sweep_cases as S

pytestmark = pytest.mark.gpu
GUARD = 4096                                   # f32 elements of NaN on either side of `out`
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
# seeds of the gauss cases: chosen on the CPU so that the restatement counts no pixel within S.NEAR of an integer
GAUSS_SEED = 1


def _run(src_np, desc_np, oh, ow, gray, norm, fill, protocol, seed, index0):
    """msml_eval_pairs on a guarded output: returns the rows; asserts the guards and the source are untouched."""
    from msml_amd._lib import call
    n, h, w, _ = src_np.shape
    src = torch.from_numpy(src_np).cuda()
    desc = None if desc_np is None else torch.from_numpy(np.ascontiguousarray(desc_np)).cuda()
    ch = 1 if gray else 3
    numel = 2 * n * ch * oh * ow
    buf = torch.full((numel + 2 * GUARD,), float("nan"), device="cuda")
    out = buf[GUARD:GUARD + numel].view(2 * n, ch, oh, ow)
    call("msml_eval_pairs", src, n, h, w, desc, out, oh, ow, gray, norm, S.FILLS.index(fill), int(protocol == "NB"),
         seed, index0)
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + numel:]).all()), "guard band written"
    assert np.array_equal(src.cpu().numpy(), src_np), "source written"
    return out.clone()


def _equal(got, want, name):
    same = torch.equal(got.cpu(), torch.from_numpy(want))
    if not same:
        bad = int((got.cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
        print("%s: %d of %d elements differ" % (name, bad, want.size))
    return same


@pytest.mark.parametrize("case", S.CASES, ids=["%dx%d-%dx%d-g%d-n%d" % c for c in S.CASES])
def test_rows_equal_pil_bit_for_bit(case):
    h, w, oh, ow, gray, norm = case
    src = S.faces(h, w, 100 + h + w)
    # no descriptors at all
    want, _, _ = S.reference_rows(src, None, oh, ow, gray, norm)
    assert _equal(_run(src, None, oh, ow, gray, norm, "black", "BB", 1, 0), want, "desc = NULL")
    if gray:
        assert want.shape[1] == 1
    for lo, hi in S.LEVELS:
        for index0 in (0, 1):
            desc = S.draw(7, 5, index0, lo, hi, ow)
            assert (desc[:, 0] == (0 if lo == 0 else 3)).all()
            for fill in ("black", "white"):
                for protocol in ("BB",) if gray else ("BB", "NB"):
                    want, _, _ = S.reference_rows(src, desc, oh, ow, gray, norm, fill, protocol, 5, index0)
                    got = _run(src, desc, oh, ow, gray, norm, fill, protocol, 5, index0)
                    assert _equal(got, want, "%s %s [%d, %d) index0=%d" % (fill, protocol, lo, hi, index0))
    d = S.draw(7, 5, 0, 10, 11, ow)                            # the mirrored copy draws a block of its own
    assert (d[0::2, 1:3] != d[1::2, 1:3]).any()


def test_foreign_descriptor_kind_poisons_its_row_only():
    src = S.faces(112, 112, 3)
    desc = S.draw(7, 2, 0, 40, 41, 112)
    desc[4, 0], desc[5, 0] = 1, 4                             # image 2: a rectangle and a polygon of the training mix
    got = _run(src, desc, 112, 112, 0, 1, "black", "BB", 2, 0)
    assert bool(torch.isnan(got[4:6]).all())
    clean = desc.copy()
    clean[4:6, 0] = 0
    want, _, _ = S.reference_rows(src, clean, 112, 112, 0, 1, "black", "BB", 2, 0)
    keep = [0, 1, 2, 3] + list(range(6, 14))
    assert torch.equal(got[keep].cpu(), torch.from_numpy(want[keep]))
    # NB skips the step for odd images: the descriptor of image 2 + 1 is not read
    got = _run(src, desc, 112, 112, 0, 1, "black", "NB", 2, 1)
    assert bool(torch.isfinite(got).all())


def _bytes(rows, norm):
    v = rows.double() * 0.5 + 0.5 if norm else rows.double()
    return torch.round(v * 255).to(torch.int64).cpu().numpy()


@pytest.mark.parametrize("case", S.CASES, ids=["%dx%d-%dx%d-g%d-n%d" % c for c in S.CASES])
def test_gauss_fill(case):
    """Exact equality except where the restated z * 255 lies within 1e-6 of an integer (either neighbour accepted, at
    most 1 in 10^4 block pixels; the seed is chosen so that the restatement counts none)."""
    h, w, oh, ow, gray, norm = case
    src = S.faces(h, w, 200 + h + w)
    for lo, hi in ((10, 11), (90, 91)):
        desc = S.draw(7, GAUSS_SEED, 1, lo, hi, ow)
        want, near, drawn = S.reference_rows(src, desc, oh, ow, gray, norm, "gauss", "BB", GAUSS_SEED, 1)
        got = _run(src, desc, oh, ow, gray, norm, "gauss", "BB", GAUSS_SEED, 1).cpu().numpy()
        diff = got.view(np.uint32) != want.view(np.uint32)
        print("gauss [%d, %d): %d block values drawn, %d near an integer, %d elements differ"
              % (lo, hi, drawn, int(near.sum()), int(diff.sum())))
        assert drawn > 0 and near.sum() * 10000 <= drawn
        assert not (diff & ~near).any()
        if diff.any():                                         # a neighbouring byte, nothing else
            gb, wb = _bytes(torch.from_numpy(got), norm), _bytes(torch.from_numpy(want), norm)
            step = (gb - wb)[diff] % 256
            assert np.isin(step, (1, 255)).all()


def test_gauss_block_is_not_degenerate():
    """A 106 x 106 block (RGB 112, [90, 91)): the device's bytes are the restatement's, so their mean and variance are
    too; the restated normals behind them have mean 0 and variance 1 within four standard errors."""
    src = S.faces(112, 112, 9)[:1]
    desc = S.draw(1, GAUSS_SEED, 0, 90, 91, 112)
    x0, y0, bw, bh = (int(v) for v in desc[0, 1:5])
    assert (bw, bh) == (106, 106)
    got = _run(src, desc, 112, 112, 0, 0, "gauss", "BB", GAUSS_SEED, 0)
    z = S.normals(GAUSS_SEED, 0, 106, 106, 3)
    dev = np.ascontiguousarray(_bytes(got[0, :, y0:y0 + bh, x0:x0 + bw], 0).transpose(1, 2, 0))     # same layout, same sums
    ref = np.asarray(S.block_image("gauss", "RGB", 106, 106, z)).astype(np.int64)
    print("device bytes mean %.4f var %.2f, restated mean %.4f var %.2f; z mean %.4f var %.4f"
          % (dev.mean(), dev.var(), ref.mean(), ref.var(), z.mean(), z.var()))
    assert dev.mean() == ref.mean() and dev.var() == ref.var()
    assert len(np.unique(dev)) == 256
    n = z.size
    assert abs(z.mean()) < 4 / np.sqrt(n) and abs(z.var() - 1) < 4 * np.sqrt(2 / n)


def test_eval_pairs_python_path_and_batch_split():
    from msml_amd import verification as V
    for h, w, oh, ow, gray, norm in (S.CASES[0], S.CASES[2], S.CASES[3]):
        src = S.faces(h, w, 300 + w)
        dev = torch.from_numpy(src).cuda()
        for fill, protocol in (("black", "BB"), ("gauss", "BB")) + ((("white", "NB"),) if not gray else ()):
            desc = S.draw(7, 11, 3, 40, 41, ow)
            want, near, _ = S.reference_rows(src, desc, oh, ow, gray, norm, fill, protocol, 11, 3)
            got = V.eval_pairs(dev, seed=11, index0=3, lo=40, hi=41, fill=fill, protocol=protocol, out_size=(oh, ow),
                               gray=bool(gray), use_norm=bool(norm))
            assert not near.any() and _equal(got, want, "eval_pairs %s %s" % (fill, protocol))
    # (0, 1) and None are the clean inputs
    clean, _, _ = S.reference_rows(src, None, oh, ow, gray, norm)
    for lo, hi in ((0, 1), (None, None)):
        assert _equal(V.eval_pairs(dev, lo=lo, hi=hi, out_size=(oh, ow), use_norm=bool(norm)), clean, "clean")
    # 8 images at once = two calls of 4 with index0 = 0 / 4
    src8 = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (8, 112, 112, 3), dtype=np.uint8)).cuda()
    for kw in (dict(fill="gauss", protocol="BB"), dict(fill="white", protocol="NB"),
               dict(fill="gauss", gray=True, out_size=128, use_norm=False)):
        whole = V.eval_pairs(src8, seed=3, lo=40, hi=41, **kw)
        halves = torch.cat([V.eval_pairs(src8[:4], seed=3, index0=0, lo=40, hi=41, **kw),
                            V.eval_pairs(src8[4:], seed=3, index0=4, lo=40, hi=41, **kw)])
        assert torch.equal(whole, halves), kw
        assert torch.equal(whole, V.eval_pairs(src8, seed=3, lo=40, hi=41, **kw))          # two runs, the same bits
    with pytest.raises(ValueError):
        V.eval_pairs(src8, out_size=(112, 110))


_MODEL = {}


def _ires18():
    if "m" not in _MODEL:
        from msml_amd.backbones import MSML
        from oracle.fill import fill_module
        torch.manual_seed(0)
        _MODEL["m"] = fill_module(MSML("iresnet18", "unet", (1, 1, 1, 1), 8, fp16=False,
                                       fm_params=(3, 2, "sigmoid", "mul"), header_type="AMArcFace",
                                       peer_params=dict(PEER_OFF))).cuda().eval()
    return _MODEL["m"]


def _pair_faces(n_pairs, size, seed):
    """2 * n_pairs synthetic faces: pair p is the same face twice with small noise when p is even, two faces otherwise."""
    rng = np.random.default_rng(seed)
    out = np.empty((2 * n_pairs, size, size, 3), np.uint8)
    issame = []
    for p in range(n_pairs):
        a = rng.integers(0, 256, (size // 8, size // 8, 3)).repeat(8, 0).repeat(8, 1)
        b = a if p % 2 == 0 else rng.integers(0, 256, (size // 8, size // 8, 3)).repeat(8, 0).repeat(8, 1)
        out[2 * p] = np.clip(a + rng.integers(-8, 9, a.shape), 0, 255)
        out[2 * p + 1] = np.clip(b + rng.integers(-8, 9, a.shape), 0, 255)
        issame.append(p % 2 == 0)
    return out, issame


def test_extract_sum_batches_give_the_same_bits():
    from msml_amd import verification as V
    model = _ires18()
    src = torch.from_numpy(_pair_faces(4, 112, 2)[0]).cuda()
    a = V.extract_sum(model, src, batch=8, seed=4, lo=40, hi=41)
    b = V.extract_sum(model, src, batch=3, seed=4, lo=40, hi=41)
    assert a.dtype == torch.float32 and a.shape[0] == 8 and a.is_cuda and bool(torch.isfinite(a).all())
    print("extract_sum batch 3 vs 8: max abs diff %.3e" % float((a - b).abs().max()))
    assert torch.equal(a, b)


def test_occlusion_sweep_equals_the_steps_composed_by_hand():
    from msml_amd import verification as V
    model = _ires18()
    faces, issame = _pair_faces(40, 112, 6)
    src = torch.from_numpy(faces).cuda()
    levels = ((0, 1), (40, 41))
    res = V.occlusion_sweep(model, src, issame, levels=levels, repeats=2, seed=3, batch=80)
    assert res["levels"] == [(0, 1), (40, 41)] and [len(a) for a in res["acc"]] == [1, 2]      # (0, 1): one extraction
    assert res["tarfar"].shape == (2, 5) and [t.shape for t in res["tarfar_runs"]] == [(1, 5), (2, 5)]
    for k, (lo, hi) in enumerate(levels):
        accs, fars = [], []
        for r in range(len(res["acc"][k])):
            x = V.eval_pairs(src, seed=V.sweep_seed(3, k, r), lo=lo, hi=hi)
            with torch.no_grad():
                f = model(x)[0].float()
            emb = f[0::2] + f[1::2]
            if k == 0:      # clean 112 -> 112 rows: row 2i + 1 IS the mirror of row 2i, extract_embeddings' own protocol
                assert torch.equal(x[1::2], x[0::2].flip(3))
                ee = V.extract_embeddings(model, x[0::2]).float()
                print("extract_embeddings vs the pair sum: max abs diff %.3e" % float((ee - emb).abs().max()))
                assert torch.equal(ee, emb)
            accs.append(float(np.mean(V.evaluate(emb, issame)[2])))
            roc, tarfar = V.roc_accuracy_tarfar(emb, issame)
            assert res["roc_acc"][k][r] == roc and np.array_equal(res["tarfar_runs"][k][r], tarfar)
            fars.append(tarfar)
        assert res["acc"][k] == accs
        assert res["avg_acc"][k] == sum(accs) / len(accs)
        assert np.array_equal(res["tarfar"][k], np.sum(fars, axis=0) / len(fars))
        assert 0.0 <= res["avg_acc"][k] <= 1.0
    print("avg_acc", res["avg_acc"], "tarfar", res["tarfar"].tolist())
    again = V.occlusion_sweep(model, src, issame, levels=levels, repeats=2, seed=3, batch=80)
    assert again["avg_acc"] == res["avg_acc"] and again["acc"] == res["acc"] and again["roc_acc"] == res["roc_acc"]
    assert np.array_equal(again["tarfar"], res["tarfar"])
    assert all(np.array_equal(a, b) for a, b in zip(again["tarfar_runs"], res["tarfar_runs"]))


def test_gray_sweep_through_lightcnn():
    """Plumbing only: gray 128 x 128 unnormalised inputs from 112 x 112 sources through the LightCNN MSML in f32."""
    from msml_amd import verification as V
    from msml_amd.backbones import MSML
    from oracle.fill import fill_module
    torch.manual_seed(0)
    model = fill_module(MSML("lightcnn", "unet", (1, 1, 1, 1), 8, fp16=False, fm_params=(3, 2, "sigmoid", "mul"),
                             header_type="Softmax", peer_params=dict(PEER_OFF))).cuda().eval()
    faces, issame = _pair_faces(20, 112, 8)
    res = V.occlusion_sweep(model, torch.from_numpy(faces).cuda(), issame, levels=((0, 1), (40, 41)), repeats=1,
                            fill="gauss", gray=True, out_size=128, use_norm=False, batch=16)
    assert len(res["avg_acc"]) == 2 and all(np.isfinite(a) and 0.0 <= a <= 1.0 for a in res["avg_acc"])
    assert np.isfinite(res["tarfar"]).all() and (res["tarfar"] >= 0).all() and (res["tarfar"] <= 1).all()
