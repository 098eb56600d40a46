"""CPU tests of the segmentation-branch evaluation: the numpy restatement (tests/segeval_cases.py) against independent
oracles (scipy.ndimage, sklearn.metrics), the host half of msml_amd/segeval.py, and the refusals of the three entry points
of csrc/segeval.hip, which come before any launch and so need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import segeval_cases as S

STRUCTURE = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]), 8: np.ones((3, 3), int)}


@pytest.mark.parametrize("size", S.SIZES, ids=["%dx%d" % s for s in S.SIZES])
@pytest.mark.parametrize("connectivity", (4, 8))
def test_labels_equal_scipy_numbering_included(size, connectivity):
    from scipy import ndimage
    names, occ = S.pattern_batch(*size)
    for name, o in zip(names, occ):
        want, k = ndimage.label(o, structure=STRUCTURE[connectivity])
        got, count = S.label(o, connectivity)
        assert count == k and np.array_equal(got, want), (name, size, connectivity)
        # the seeds and merges the kernel issues reach the same components and the same numbers
        got2, count2 = S.kernel_merge_label(o, connectivity)
        assert count2 == k and np.array_equal(got2, want), ("kernel rule", name, size, connectivity)


def test_patterns_are_what_they_claim():
    for h, w in S.SIZES:
        p = S.patterns(h, w)
        assert S.label(p["serpentine"], 4)[1] == 1 and S.label(p["clean"], 8)[1] == 0
        assert S.label(p["occluded"], 4)[1] == 1
        if "corner_touch" in p:
            assert (S.label(p["corner_touch"], 4)[1], S.label(p["corner_touch"], 8)[1]) == (2, 1)
    p = S.patterns(128, 128)
    assert S.label(p["checker"], 4)[1] == 8192 and S.label(p["checker"], 8)[1] == 1
    assert S.label(p["rings"], 4)[1] == 32 and S.label(p["u"], 4)[1] == 1 and S.label(p["comb"], 4)[1] == 33
    assert p["serpentine"].sum() == 64 * 128 + 64
    assert S.label(p["corners"], 8)[1] == 4


@pytest.mark.parametrize("size", ((5, 7), (112, 112)), ids=("5x7", "112x112"))
@pytest.mark.parametrize("connectivity", (4, 8))
def test_table_rows_equal_scipy(size, connectivity):
    from scipy import ndimage
    names, occ = S.pattern_batch(*size)
    b = np.roll(occ, 1, axis=0)                        # the second mask: every pattern against its neighbour
    labels, count = S.label(occ, connectivity)
    cap = 64
    table = S.blob_table(labels, count, b, cap)
    for i, name in enumerate(names):
        k = int(count[i])
        rows = min(k, cap)
        assert not table[i, rows:].any()
        if rows == 0:
            continue
        idx = np.arange(1, rows + 1)
        assert np.array_equal(table[i, :rows, 0], ndimage.sum(occ[i], labels[i], idx).astype(np.int64)), name
        assert np.array_equal(table[i, :rows, 1], ndimage.sum(b[i] & occ[i], labels[i], idx).astype(np.int64)), name
        for r, sl in enumerate(ndimage.find_objects(labels[i])[:rows]):
            assert tuple(table[i, r, 2:]) == (sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1), (name, r)


def test_counts_and_metrics_equal_sklearn():
    from sklearn import metrics as M
    rng = np.random.default_rng(3)
    for n, h, w in S.COUNT_SHAPES[:4]:
        p, g = rng.random((n, h, w)) < 0.4, rng.random((n, h, w)) < 0.3
        c = S.counts(p, g)
        for i in range(n):
            tn, fp, fn, tp = M.confusion_matrix(g[i].ravel(), p[i].ravel(), labels=[False, True]).ravel()
            assert tuple(c[i]) == (tp, fp, fn, tn)
    from msml_amd import segeval
    n, h, w = 3, 40, 44
    p, g = rng.random((n, h, w)) < 0.4, rng.random((n, h, w)) < 0.3
    c = S.counts(p, g)
    for got in (segeval.metrics_from_counts(c), S.metrics(c)):
        yt, yp = g.ravel(), p.ravel()
        want = {"iou_occ": M.jaccard_score(yt, yp), "iou_clean": M.jaccard_score(~yt, ~yp),
                "precision": M.precision_score(yt, yp), "recall": M.recall_score(yt, yp),
                "dice_occ": M.f1_score(yt, yp), "pixel_acc": M.accuracy_score(yt, yp),
                "false_alarm": 1.0 - M.recall_score(~yt, ~yp)}
        for k, v in want.items():
            assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
        assert abs(got["miou"] - (want["iou_occ"] + want["iou_clean"]) / 2) <= 1e-12
        ious = [M.jaccard_score(g[i].ravel(), p[i].ravel()) for i in range(n)]
        assert got["images_defined"] == n and abs(got["image_iou_occ"] - np.mean(ious)) <= 1e-12
    # the module and the restatement agree to the bit, one image and several
    for cc in (c, c[0]):
        a, b = segeval.metrics_from_counts(cc), S.metrics(cc)
        assert S.same_metrics(a, b)
    assert segeval.metrics_from_counts(torch.from_numpy(c))["iou_occ"] == S.metrics(c)["iou_occ"]


def test_zero_denominators_give_nan_not_exceptions():
    from msml_amd import segeval
    m = segeval.metrics_from_counts(np.array([0, 0, 0, 100]))          # a clean image called clean
    assert np.isnan(m["iou_occ"]) and np.isnan(m["precision"]) and np.isnan(m["recall"]) and np.isnan(m["dice_occ"])
    assert m["iou_clean"] == 1.0 and m["miou"] == 1.0 and m["pixel_acc"] == 1.0 and m["false_alarm"] == 0.0
    m = segeval.metrics_from_counts(np.array([[0, 5, 0, 95], [0, 0, 0, 100]]))
    assert m["iou_occ"] == 0.0 and m["false_alarm"] == 5 / 200
    assert m["images_defined"] == 1 and m["image_iou_occ"] == 0.0
    m = segeval.metrics_from_counts(np.zeros((2, 4), np.int64))
    assert all(np.isnan(m[k]) for k in ("pixel_acc", "iou_occ", "iou_clean", "miou", "false_alarm", "image_iou_occ"))
    assert m["images_defined"] == 0
    assert S.same_metrics(m, S.metrics(np.zeros((2, 4), np.int64)))
    with pytest.raises(ValueError):
        segeval.metrics_from_counts(np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        segeval.metrics_from_counts(np.zeros(4))
    assert segeval.SegMeter().compute()["tp"] == 0


def test_class_rule_of_the_restatement_is_mask_index():
    from msml_amd import functional as Fh
    x = S.planted_logits(2, 9, 11, 5)
    assert np.isnan(x).any() and np.isinf(x).any() and (x[:, 0] == x[:, 1]).any()
    want = Fh.mask_index(torch.from_numpy(x)).numpy()
    assert np.array_equal(S.index_mask(S.logits_occluded(x)), want)
    ref = torch.from_numpy(x).max(1)[1].numpy()                        # train.py:357 (ties: the first index, occluded)
    ok = ~np.isnan(x).any(1)
    assert np.array_equal(want[ok], ref[ok].astype(np.uint8))


def test_blob_detection_hand_cases():
    gt = np.zeros((1, 20, 20), bool)
    gt[0, 2:12, 2:12] = True                                           # one blob of 100 pixels
    for covered, found in ((49, 0), (50, 1)):
        pred = np.zeros_like(gt)
        pred.reshape(1, -1)[0, np.flatnonzero(gt[0].ravel())[:covered]] = True
        d = S.blob_detection(pred, gt, tau=0.5)
        assert (d["n_gt"], d["n_found"], d["n_false"]) == (1, found, 0), (covered, d)
    pred = gt.copy()
    pred[0, 15:18, 15:18] = True                                       # a spurious blob of 9
    d = S.blob_detection(pred, gt)
    assert (d["n_gt"], d["n_found"], d["n_pred"], d["n_false"]) == (1, 1, 2, 1) and d["false_alarm_rate"] == 0.5
    d = S.blob_detection(pred, gt, min_area=10)                        # filters the spurious blob
    assert (d["n_pred"], d["n_false"]) == (1, 0)
    with pytest.raises(RuntimeError):
        S.blob_detection(S.patterns(20, 20)["checker"][None], gt, connectivity=4, cap=64)


def _host_ptr():
    buf = (ctypes.c_double * 64)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_refusals_need_no_gpu():
    """Every refusal comes before any launch: reached with the address of a host buffer, which a refusing call never
    dereferences."""
    from msml_amd import _lib
    lib = _lib.load()
    buf, p = _host_ptr()
    SHAPE, DTYPE, UNSUPPORTED = -1, -2, _lib.UNSUPPORTED

    def counts(pred=p, pk=0, gt=p, gk=2, out=p, total=None, N=1, H=8, W=8):
        return lib.msml_seg_counts(pred, pk, gt, gk, out, total, N, H, W, None)

    def label(mask=p, kind=2, labels=p, count=p, status=p, N=1, H=8, W=8, conn=8):
        return lib.msml_seg_label(mask, kind, labels, count, status, N, H, W, conn, None)

    def table(labels=p, count=p, b=p, kind=2, out=p, N=1, H=8, W=8, cap=64):
        return lib.msml_seg_blob_table(labels, count, b, kind, out, N, H, W, cap, None)

    def said(text):
        return text in lib.msml_last_error()

    # null pointers
    for kw in ({"pred": None}, {"gt": None}, {"out": None}):
        assert counts(**kw) == SHAPE and said(b"seg_counts: null pointer")
    for kw in ({"mask": None}, {"count": None}, {"status": None}):
        assert label(**kw) == SHAPE and said(b"seg_label: null pointer")
    for kw in ({"labels": None}, {"count": None}, {"b": None}, {"out": None}):
        assert table(**kw) == SHAPE and said(b"seg_blob_table: null pointer")
    # unknown kinds; the ground truth is an index mask
    for bad in (-1, 4, 17):
        assert counts(pk=bad) == DTYPE and said(b"pred kind")
        assert counts(gk=bad) == DTYPE and said(b"gt kind")
        assert label(kind=bad) == DTYPE and said(b"mask kind") and table(kind=bad) == DTYPE and said(b"mask kind")
    assert counts(gk=0) == DTYPE and counts(gk=1) == DTYPE
    # sides 0 and 257, N 0
    for fn, who in ((counts, b"seg_counts"), (label, b"seg_label"), (table, b"seg_blob_table")):
        for kw in ({"H": 0}, {"W": 0}, {"H": 257}, {"W": 257}):
            assert fn(**kw) == UNSUPPORTED and said(who) and said(b"outside 1..256"), (who, kw)
        assert fn(N=0) == UNSUPPORTED and said(b"N=0")
    # the labelling: H W = 16385 and beyond, connectivity 6
    assert label(H=113, W=145) == UNSUPPORTED and said(b"16385 pixels")
    assert label(H=256, W=256) == UNSUPPORTED and said(b"65536 pixels")
    for conn in (6, 0, 5, 9):
        assert label(conn=conn) == UNSUPPORTED and said(b"connectivity %d" % conn)
    # the table: cap 0 and 1025
    assert table(cap=0) == UNSUPPORTED and said(b"cap 0") and table(cap=1025) == UNSUPPORTED and said(b"cap 1025")
    # misaligned pointers
    assert counts(out=p + 4) == SHAPE and counts(total=p + 4) == SHAPE and counts(pred=p + 2, pk=0) == SHAPE
    assert label(labels=p + 2) == SHAPE and table(out=p + 1) == SHAPE and label(mask=p + 4, kind=3) == SHAPE


def test_python_value_errors():
    from msml_amd import segeval
    from msml_amd import verification as V
    logits = torch.zeros(2, 2, 8, 8)
    gt = torch.ones(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the device"):
        segeval.mask_counts(logits, gt)                                # CPU tensors
    with pytest.raises(ValueError, match="contiguous"):
        segeval.mask_counts(torch.zeros(2, 8, 8, 2).permute(0, 3, 1, 2), gt)
    with pytest.raises(ValueError, match=r"\[N\]\[2\]\[H\]\[W\]"):
        segeval.mask_counts(torch.zeros(2, 3, 8, 8), gt)
    with pytest.raises(ValueError, match="dtype"):
        segeval.mask_counts(torch.zeros(2, 2, 8, 8, dtype=torch.float64), gt)
    with pytest.raises(ValueError, match="index mask"):
        segeval.mask_counts(logits, torch.zeros(2, 2, 8, 8))           # logits as the ground truth
    with pytest.raises(ValueError, match="sides"):
        segeval.mask_counts(torch.zeros(1, 2, 8, 257), torch.ones(1, 8, 257, dtype=torch.uint8))
    with pytest.raises(ValueError):
        segeval.mask_counts(None, gt)
    with pytest.raises(ValueError, match="connectivity"):
        segeval.label_blobs(gt, connectivity=6)
    with pytest.raises(ValueError, match="cap"):
        segeval.blob_table(gt, gt, cap=0)
    with pytest.raises(ValueError, match="cap"):
        segeval.blob_table(gt, gt, cap=1025)
    with pytest.raises(ValueError, match="on the device"):
        segeval.blob_detection(gt, gt)
    with pytest.raises(ValueError, match="tau"):
        segeval.blob_totals(gt, gt, tau=1.5)
    with pytest.raises(ValueError, match="not resized"):               # a size mismatch is refused, not resized
        segeval.mask_counts(logits, torch.ones(2, 8, 12, dtype=torch.uint8))
    with pytest.raises(ValueError, match="not resized"):
        segeval.mask_counts(logits, torch.ones(3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="not resized"):
        segeval.blob_table(gt, torch.ones(2, 12, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="16384"):
        segeval.label_blobs(torch.ones(1, 129, 128, dtype=torch.uint8))
    # eval_pair_masks: eval_pairs' refusals, before anything touches the device
    for kw in ({"protocol": "XB"}, {"lo": 3, "hi": None}, {"lo": 50, "hi": 40}, {"lo": 5, "hi": 102}, {"index0": -1},
               {"n": 0}, {"out_size": (112, 110)}, {"h": 2}, {"w": 300}):
        args = dict(n=4, h=112, w=112, lo=40, hi=41)
        args.update(kw)
        with pytest.raises(ValueError, match="eval_pair_masks"):
            V.eval_pair_masks(**args)


def test_pair_masks_restatement():
    desc = np.zeros((4, 64), np.int32)
    desc[0, :5] = (3, 2, 3, 4, 5)
    desc[1, :5] = (3, 6, 0, 10, 2)                                     # cropped at the right border
    desc[2, :5] = (3, 0, 0, 1, 1)
    m = S.pair_masks(desc, 8, 8)
    assert (m == 0).sum((1, 2)).tolist() == [20, 4, 1, 0] and not m[0, 3:8, 2:6].any() and not m[1, 0:2, 6:8].any()
    nb = S.pair_masks(desc, 8, 8, "NB", index0=1)                      # images 1 (odd: clean) and 2
    assert (nb == 0).sum((1, 2)).tolist() == [0, 0, 1, 0]
