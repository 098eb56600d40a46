"""GPU tests of the segmentation-branch evaluation (csrc/segeval.hip, msml_amd/segeval.py, the sweep additions of
msml_amd/verification.py) against the numpy restatement of tests/segeval_cases.py: exact integer equality everywhere.
Every kernel output is written between guard bands, and the guards and the inputs are checked afterwards."""
import numpy as np
import pytest
import torch

from tests import segeval_cases as S

pytestmark = pytest.mark.gpu
GUARD = 1024                                   # elements of FILL on either side of every output
FILL = 0x5A5A5A5A
PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
KIND = {torch.float32: 0, torch.bfloat16: 1, torch.uint8: 2, torch.int64: 3}


class Guarded:
    """An output tensor between two guard bands."""

    def __init__(self, shape, dtype):
        self.numel = int(np.prod(shape))
        self.buf = torch.full((self.numel + 2 * GUARD,), FILL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.numel].view(*shape)

    def check(self):
        assert bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.numel:] == FILL).all()), \
            "guard band written"
        return self.t.cpu().numpy()


def _untouched(pairs):
    for dev, host in pairs:
        assert torch.equal(dev.cpu().reshape(-1).view(torch.uint8), host.reshape(-1).view(torch.uint8)), "input written"


def _run_counts(pred, gt, total=None):
    """msml_seg_counts on a guarded output; pred / gt: host tensors."""
    from msml_amd._lib import call
    dp, dg = pred.cuda(), gt.cuda()
    n, h, w = gt.shape
    out = Guarded((n, 4), torch.int64)
    call("msml_seg_counts", dp, KIND[pred.dtype], dg, KIND[gt.dtype], out.t, total, n, h, w)
    got = out.check()
    _untouched(((dp, pred), (dg, gt)))
    return got


def _run_label(mask, connectivity, want_labels=True):
    from msml_amd._lib import call
    dm = mask.cuda()
    n, h, w = mask.shape[0], mask.shape[-2], mask.shape[-1]
    labels, count, status = Guarded((n, h, w), torch.int32), Guarded((n,), torch.int32), Guarded((n,), torch.int32)
    call("msml_seg_label", dm, KIND[mask.dtype], labels.t if want_labels else None, count.t, status.t, n, h, w,
         connectivity)
    got = labels.check(), count.check(), status.check()
    if not want_labels:
        assert (got[0] == FILL).all()
    _untouched(((dm, mask),))
    return got + (labels.t, count.t)


def _run_table(labels_dev, count_dev, b, cap):
    from msml_amd._lib import call
    db = b.cuda()
    n, h, w = b.shape[0], b.shape[-2], b.shape[-1]
    keep = labels_dev.clone(), count_dev.clone()
    table = Guarded((n, cap, 6), torch.int32)
    call("msml_seg_blob_table", labels_dev, count_dev, db, KIND[b.dtype], table.t, n, h, w, cap)
    got = table.check()
    assert torch.equal(keep[0], labels_dev) and torch.equal(keep[1], count_dev), "input written"
    _untouched(((db, b),))
    return got


def _index(occ, dtype):
    """A host index mask of the occluded pixels `occ`; clean pixels take several non-zero values."""
    occ = np.asarray(occ, bool)
    rng = np.random.default_rng(occ.size)
    if dtype == torch.uint8:
        v = rng.integers(1, 256, occ.shape).astype(np.uint8)
    else:
        v = rng.choice(np.array([1, -1, 255, 256, 1 << 40, -(1 << 62)], np.int64), occ.shape)
    v[occ] = 0
    return torch.from_numpy(v)


def _logits(occ, dtype, seed=0):
    """Host logits whose class rule gives `occ`: b > a exactly on the clean pixels."""
    occ = np.asarray(occ, bool)
    rng = np.random.default_rng(seed + occ.size)
    a = rng.standard_normal(occ.shape).astype(np.float32)
    gap = rng.random(occ.shape).astype(np.float32) + 0.25
    b = np.where(occ, a - gap * (rng.random(occ.shape) < 0.7), a + gap).astype(np.float32)      # some ties: occluded
    x = torch.from_numpy(np.stack([a, b], 1)).to(dtype)
    assert np.array_equal(S.logits_occluded(x.float().numpy()), occ)
    return x.contiguous()


PRED_FORMS = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8, "i64": torch.int64}


@pytest.mark.parametrize("form", sorted(PRED_FORMS))
@pytest.mark.parametrize("shape", S.COUNT_SHAPES, ids=["%dx%dx%d" % s for s in S.COUNT_SHAPES])
def test_counts_equal_the_restatement(shape, form):
    n, h, w = shape
    rng = np.random.default_rng(n * 1000 + h + w)
    p_occ, g_occ = rng.random(shape) < 0.4, rng.random(shape) < 0.3
    dtype = PRED_FORMS[form]
    pred = _logits(p_occ, dtype) if form in ("f32", "bf16") else _index(p_occ, dtype)
    want = S.counts(p_occ, g_occ)
    assert (want.sum(1) == h * w).all()
    for gdt in (torch.uint8, torch.int64):
        got = _run_counts(pred, _index(g_occ, gdt))
        assert np.array_equal(got, want), (shape, form, gdt)


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("f32", "bf16"))
def test_planted_ties_zeros_infinities_and_nan_follow_mask_index(dtype):
    from msml_amd import functional as Fh
    from msml_amd import segeval
    x = torch.from_numpy(S.planted_logits(3, 24, 40, 11)).to(dtype).contiguous()       # aligned planes: the 16-byte path
    y = torch.from_numpy(S.planted_logits(3, 5, 7, 12)).to(dtype).contiguous()         # the scalar path
    for t in (x, y):
        f = t.float().numpy()
        assert np.isnan(f).any() and np.isinf(f).any() and (f[:, 0] == f[:, 1]).any() and (f == 0).any()
        idx = Fh.mask_index(t.cuda())                                                  # uint8, 0 = occluded
        assert np.array_equal(idx.cpu().numpy(), S.index_mask(S.logits_occluded(f)))
        rng = np.random.default_rng(1)
        gt = _index(rng.random(idx.shape) < 0.5, torch.uint8)
        a = _run_counts(t, gt)
        b = segeval.mask_counts(idx.contiguous(), gt.cuda()).cpu().numpy()
        assert np.array_equal(a, b) and np.array_equal(a, S.counts(S.logits_occluded(f), gt.numpy() == 0))


def test_total_accumulates_over_three_launches_and_segmeter():
    from msml_amd import segeval
    rng = np.random.default_rng(8)
    total = Guarded((4,), torch.int64)
    total.t.zero_()
    meter = segeval.SegMeter()
    want = np.zeros(4, np.int64)
    for n, h, w in ((2, 112, 112), (3, 3, 113), (1, 5, 7)):
        p_occ, g_occ = rng.random((n, h, w)) < 0.5, rng.random((n, h, w)) < 0.2
        pred, gt = _logits(p_occ, torch.float32), _index(g_occ, torch.int64)
        got = _run_counts(pred, gt, total.t)
        want += got.sum(0)
        assert np.array_equal(got, S.counts(p_occ, g_occ))
        assert np.array_equal(meter.update(pred.cuda(), gt.cuda()).cpu().numpy(), got)
    assert np.array_equal(total.check(), want)
    m = meter.compute()
    assert (m["tp"], m["fp"], m["fn"], m["tn"]) == tuple(want) and S.same_metrics(m, S.metrics(want))
    meter.reset()
    assert meter.compute()["tn"] == 0


def _check_labels_and_table(occ, b_occ, connectivity, cap, mask_dtype=torch.uint8, b_dtype=torch.uint8):
    want_labels, want_count = S.label(occ, connectivity)
    mask = _index(occ, mask_dtype) if mask_dtype in (torch.uint8, torch.int64) else _logits(occ, mask_dtype)
    labels, count, status, dl, dc = _run_label(mask, connectivity)
    assert not status.any(), status
    assert np.array_equal(count, want_count), (count, want_count)
    assert np.array_equal(labels, want_labels)
    b = _index(b_occ, b_dtype) if b_dtype in (torch.uint8, torch.int64) else _logits(b_occ, b_dtype)
    table = _run_table(dl, dc, b, cap)
    assert np.array_equal(table, S.blob_table(want_labels, want_count, b_occ, cap))
    return labels, count, table


@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("size", S.SIZES, ids=["%dx%d" % s for s in S.SIZES])
def test_labels_and_tables_equal_the_restatement(size, connectivity):
    names, occ = S.pattern_batch(*size)
    b_occ = np.roll(occ, 1, axis=0)                    # every pattern against its neighbour in the batch
    labels, count, table = _check_labels_and_table(occ, b_occ, connectivity, 64)
    serp = names.index("serpentine")
    assert count[serp] == 1                            # the longest path ends with status 0 (checked above) in one piece
    if size == (128, 128) and connectivity == 4:
        k = names.index("checker")
        assert count[k] == 8192
        assert (table[k, :, 0] == 1).all() and (table[k, :, 2] == table[k, :, 4]).all()      # 64 rows, no zeros before
    # the same counts without a label plane
    _, count2, status2, _, _ = _run_label(_index(occ, torch.uint8), connectivity, want_labels=False)
    assert np.array_equal(count2, count) and not status2.any()
    # every image alone gets what it got in the batch; a second run gives the same bits
    for i in range(len(names)):
        l1, c1, s1, dl, dc = _run_label(_index(occ[i:i + 1], torch.uint8), connectivity)
        assert np.array_equal(l1[0], labels[i]) and c1[0] == count[i] and s1[0] == 0, names[i]
        assert np.array_equal(_run_table(dl, dc, _index(b_occ[i:i + 1], torch.uint8), 64)[0], table[i]), names[i]
    again = _check_labels_and_table(occ, b_occ, connectivity, 64)
    assert all(np.array_equal(a, b) for a, b in zip(again, (labels, count, table)))


@pytest.mark.parametrize("connectivity", (4, 8))
def test_every_mask_form_labels_alike_and_caps(connectivity):
    names, occ = S.pattern_batch(112, 112)
    b_occ = occ[::-1].copy()
    base = _check_labels_and_table(occ, b_occ, connectivity, 1024)
    for mdt, bdt in ((torch.int64, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.int64)):
        got = _check_labels_and_table(occ, b_occ, connectivity, 1024, mdt, bdt)
        assert all(np.array_equal(a, b) for a, b in zip(got, base))
    _check_labels_and_table(occ, b_occ, connectivity, 1)


def test_augment_masks_label_like_the_restatement():
    """The `msk` of data.augment(mode="train") for 8 images, int64 as it comes."""
    from msml_amd import data, segeval
    from tests import sweep_cases as W
    src = torch.from_numpy(np.concatenate([W.faces(112, 112, 21), W.faces(112, 112, 22)])[:8]).cuda()
    msk = data.augment(src, 5, 0, mode="train")[1]
    assert msk.dtype == torch.int64 and msk.shape == (8, 112, 112)
    occ = msk.cpu().numpy() == 0
    assert occ.any() and not occ.all()
    for connectivity in (4, 8):
        _check_labels_and_table(occ, np.roll(occ, 3, axis=2), connectivity, 64, torch.int64, torch.int64)
        labels, count, status = segeval.label_blobs(msk, connectivity)
        want = S.label(occ, connectivity)
        assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
        assert not status.cpu().numpy().any()


def test_blob_detection_hand_cases(monkeypatch):
    from msml_amd import segeval
    gt = np.zeros((2, 20, 20), bool)
    gt[:, 2:12, 2:12] = True                                           # one blob of 100 pixels per image
    pred = np.zeros_like(gt)
    inside = np.flatnonzero(gt[0].ravel())
    pred[0].reshape(-1)[inside[:49]] = True                            # 49 %: missed at tau = 0.5
    pred[1].reshape(-1)[inside[:50]] = True                            # 50 %: found
    dg = _index(gt, torch.uint8).cuda()
    d = segeval.blob_detection(_index(pred, torch.uint8).cuda(), dg, tau=0.5)
    assert (d["n_gt"], d["n_found"]) == (2, 1) and d["detection_rate"] == 0.5 and d["n_false"] == 0
    assert d == S.blob_detection(pred, gt, tau=0.5)
    one, dg1 = pred[1:], dg[1:].contiguous()
    assert segeval.blob_detection(_index(one, torch.uint8).cuda(), dg1, tau=0.51)["n_found"] == 0
    # a spurious predicted blob, as logits; then a min_area that filters one blob of each kind
    pred2 = gt.copy()
    pred2[:, 15:18, 15:18] = True                                      # 9 pixels, no ground truth under it
    gt2 = gt.copy()
    gt2[:, 0, 19] = True                                               # a ground-truth blob of 1 pixel, not predicted
    dg2 = _index(gt2, torch.int64).cuda()
    d = segeval.blob_detection(_logits(pred2, torch.float32).cuda(), dg2)
    assert (d["n_gt"], d["n_found"], d["n_pred"], d["n_false"]) == (4, 2, 4, 2)
    assert d["detection_rate"] == 0.5 and d["false_alarm_rate"] == 0.5 and d == S.blob_detection(pred2, gt2)
    d = segeval.blob_detection(_logits(pred2, torch.bfloat16).cuda(), dg2, min_area=10)
    assert (d["n_gt"], d["n_found"], d["n_pred"], d["n_false"]) == (2, 2, 2, 0)
    assert d == S.blob_detection(pred2, gt2, min_area=10)
    assert np.isnan(segeval.blob_detection(torch.ones_like(dg), torch.ones_like(dg))["detection_rate"])
    # overflow: 200 components of a checkerboard against cap = 64, named by its image
    checker = np.stack([gt[0], S.patterns(20, 20)["checker"]])
    with pytest.raises(RuntimeError, match="image 1 has more than cap = 64"):
        segeval.blob_detection(_index(checker, torch.uint8).cuda(), dg, connectivity=4, cap=64)
    assert segeval.blob_detection(_index(checker, torch.uint8).cuda(), dg, connectivity=4, cap=256)["n_pred"] == 201
    # a labelling status: none can be provoked, so one is planted behind the labelling
    real = segeval._label

    def planted(who, mask, connectivity, want_labels=True):
        labels, count, status = real(who, mask, connectivity, want_labels)
        status[1] = 2
        return labels, count, status
    monkeypatch.setattr(segeval, "_label", planted)
    with pytest.raises(RuntimeError, match="image 1 ended with a status"):
        segeval.blob_detection(_index(pred, torch.uint8).cuda(), dg)


@pytest.mark.parametrize("protocol", ("BB", "NB"))
def test_eval_pair_masks_are_where_eval_pairs_paints_black(protocol):
    from msml_amd import verification as V
    n = 5
    src = torch.full((n, 120, 116, 3), 255, dtype=torch.uint8, device="cuda")
    for out_size in (None, (112, 112)):
        for index0 in (0, 3):
            for lo, hi in ((0, 1), (10, 11), (40, 41), (100, 101)):
                x = V.eval_pairs(src, seed=9, index0=index0, lo=lo, hi=hi, fill="black", protocol=protocol,
                                 out_size=out_size, use_norm=True)
                m = V.eval_pair_masks(n, 120, 116, seed=9, index0=index0, lo=lo, hi=hi, protocol=protocol,
                                      out_size=out_size)
                assert m.dtype == torch.uint8 and m.is_contiguous() and tuple(m.shape) == (2 * n,) + tuple(x.shape[2:])
                assert torch.equal(m, (x[:, 0] >= 0).to(torch.uint8)), (protocol, out_size, index0, lo, hi)
                occluded = (m == 0).sum((1, 2)).cpu().numpy().reshape(n, 2)
                if (lo, hi) == (0, 1):
                    assert not occluded.any()
                else:
                    clean = np.array([protocol == "NB" and (index0 + i) % 2 == 1 for i in range(n)])
                    assert (occluded[clean] == 0).all() and (occluded[~clean] > 0).all()
    assert torch.equal(V.eval_pair_masks(2, 112, 112, lo=None, hi=None), torch.ones(4, 112, 112, dtype=torch.uint8,
                                                                                    device="cuda"))


_MODEL = {}
BLOB_NAMES = ("n_gt", "n_found", "n_pred", "n_false", "n_overflow")


def _msml(use_osb=True):
    if use_osb not in _MODEL:
        from msml_amd.backbones import MSML
        from oracle.fill import fill_module
        torch.manual_seed(0)
        kw = {} if use_osb else {"use_osb": False}
        layers = (1, 1, 1, 1) if use_osb else (0, 0, 0, 0)               # without masks: FMNone stages only
        _MODEL[use_osb] = fill_module(MSML("iresnet18", "unet", layers, 8, fp16=False,
                                           fm_params=(3, 2, "sigmoid", "mul"), header_type="AMArcFace",
                                           peer_params=dict(PEER_OFF), **kw)).cuda().eval()
    return _MODEL[use_osb]


def test_segmentation_sweep_equals_the_steps_composed_by_hand():
    """Every number of the sweep against eval_pairs -> model -> mask_index -> the restatement on the host.  On the clean
    level (0, 1) nothing is occluded, so tp = fn = 0 and iou_occ = tp / (tp + fp + fn) is NaN exactly when the branch
    marks nothing (fp = 0); the randomly initialised branch of this test marks 34 % of the pixels (false_alarm 0.3435,
    15 of its 32 rows above 1024 specks), so iou_occ is 0 there by the same formula, and both cases are asserted."""
    from msml_amd import functional as Fh
    from msml_amd import verification as V
    from tests.test_gpu_sweep import _pair_faces
    model = _msml()
    src = torch.from_numpy(_pair_faces(8, 112, 6)[0]).cuda()
    levels = ((0, 1), (40, 41))
    batch = 6
    res = V.segmentation_sweep(model, src, levels=levels, repeats=2, seed=3, batch=batch)
    assert res["levels"] == [(0, 1), (40, 41)] and [len(c) for c in res["counts"]] == [1, 2]
    for k, (lo, hi) in enumerate(levels):
        pooled_c, pooled_b = np.zeros(4, np.int64), np.zeros(5, np.int64)
        for r in range(len(res["counts"][k])):
            s = V.sweep_seed(3, k, r)
            x = V.eval_pairs(src, seed=s, lo=lo, hi=hi)                        # all 16 images at once, index0 = 0
            gt = V.eval_pair_masks(16, 112, 112, seed=s, lo=lo, hi=hi).cpu().numpy()
            pred = []
            for i0 in range(0, 16, batch):
                with torch.no_grad():
                    seg = model(x[2 * i0:2 * (i0 + batch)])[1]
                assert seg.shape[1:] == (2, 112, 112)
                pred.append(Fh.mask_index(seg).cpu().numpy())
            p_occ, g_occ = np.concatenate(pred) == 0, gt == 0
            c = S.counts(p_occ, g_occ).sum(0)
            assert np.array_equal(res["counts"][k][r], c), (k, r)
            assert S.same_metrics(res["metrics_runs"][k][r], S.metrics(c))
            b = S.blob_detection(p_occ, g_occ, tau=0.5, cap=1024, skip_overflow=True)
            assert set(res["blobs_runs"][k][r]) == set(b) and S.same_metrics(res["blobs_runs"][k][r], b), (k, r)
            pooled_c += c
            pooled_b += np.array([b[n] for n in BLOB_NAMES])
        assert S.same_metrics(res["metrics"][k], S.metrics(pooled_c))
        got = res["blobs"][k]
        assert tuple(got[n] for n in BLOB_NAMES) == tuple(pooled_b)
        assert S.same_metrics(got, {"detection_rate": S._div(pooled_b[1], pooled_b[0]),
                                    "false_alarm_rate": S._div(pooled_b[3], pooled_b[2])})
        print("level", (lo, hi), {n: res["metrics"][k][n] for n in ("pixel_acc", "iou_occ", "false_alarm")}, got)
    m0 = res["metrics"][0]                                                     # no block: nothing to find
    assert np.isnan(m0["iou_occ"]) or m0["fp"] > 0
    assert m0["tp"] == 0 and m0["fn"] == 0 and m0["false_alarm"] == m0["fp"] / (32 * 112 * 112)
    if m0["fp"] == 0:
        assert np.isnan(m0["iou_occ"])
    assert res["blobs"][0]["n_gt"] == 0 and res["blobs"][1]["n_gt"] + res["blobs"][1]["n_overflow"] == 2 * 32
    again = V.segmentation_sweep(model, src, levels=levels, repeats=2, seed=3, batch=batch)
    assert all(np.array_equal(a, b) for a, b in zip(again["counts"], res["counts"]))
    assert again["blobs_runs"][1] == res["blobs_runs"][1]


def test_segmentation_sweep_refuses_a_model_without_the_mask_branch():
    from msml_amd import verification as V
    from tests.test_gpu_sweep import _pair_faces
    src = torch.from_numpy(_pair_faces(2, 112, 6)[0]).cuda()
    with pytest.raises(ValueError, match="final_seg"):
        V.segmentation_sweep(_msml(use_osb=False), src, levels=((0, 1),), repeats=1)
    with pytest.raises(ValueError, match="final_seg"):
        V.segmentation_sweep(lambda x: (x.new_zeros(x.shape[0], 8), x.new_zeros(x.shape[0], 2, 56, 56)), src,
                             levels=((0, 1),), repeats=1)
