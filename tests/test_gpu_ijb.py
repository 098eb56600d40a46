"""GPU tests of the template-verification path (msml_amd/ijb.py, csrc/ijb.hip) and of roc_accuracy_tarfar against
the golden recorded from the reference (tools/make_golden_ijb.py) and the numpy / sklearn restatement of
tests/ijb_cases.py.  Bound on features and scores: ijb_cases.tolerance (8 * (R + E) * 2**-53, R = rows of the largest
template); ROC tables, kept points and counts are compared exactly, the AUC to 1e-12 relative."""
import os

import numpy as np
import pytest
import torch

from tests import ijb_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_ijb.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def gset():
    return C.make_set(**C.GOLDEN_SET)


def _chain(s, **kw):
    from msml_amd import ijb
    tf, ut = ijb.template_features(s["img_feats"], s["templates"], s["medias"], s["faceness"], **kw)
    return tf, ut, ijb.pair_scores(tf, ut, s["p1"], s["p2"])


def _report(name, got, want, tol):
    err = float(np.abs(got - want).max())
    print("%s: max abs err %.3e (bound %.3e)" % (name, err, tol))
    return err


def test_features_and_scores_match_the_golden(golden, gset):
    tf, ut, sc = _chain(gset)
    tol = C.tolerance(int(golden["max_rows"]), C.GOLDEN_SET["e"])
    assert np.array_equal(ut, golden["ut"])
    assert tf.dtype == torch.float64 and tf.is_cuda and sc.is_cuda
    assert _report("template feats", tf.cpu().numpy(), golden["tn"], tol) <= tol
    assert _report("pair scores", sc.cpu().numpy(), golden["scores"], tol) <= tol


@pytest.mark.parametrize("seed,e", [(21, 256), (22, 512)])
@pytest.mark.parametrize("mode", ["flip_face", "noflip", "noface", "single"])
def test_features_and_scores_match_the_restatement(seed, e, mode):
    from msml_amd import ijb
    s = C.make_set(seed=seed, n_img=5000, e=e, n_tmpl=400, n_ident=100, noise=1.2, n_pairs=20000)
    face = None if mode == "noface" else s["faceness"]
    flip, single, feats = mode in ("flip_face", "noface"), mode == "single", s["img_feats"]
    if single:
        feats = np.ascontiguousarray(feats[:, :e])
    tf, ut = ijb.template_features(feats, s["templates"], s["medias"], face, flip_sum=flip, single=single)
    sc = ijb.pair_scores(tf, ut, s["p1"], s["p2"])
    tn, ut_r, rows = C.pool_ref(C.input_feats(feats, face, flip, single), s["templates"], s["medias"])
    tol = C.tolerance(rows, e)
    assert np.array_equal(ut, ut_r)
    assert _report("template feats", tf.cpu().numpy(), tn, tol) <= tol
    assert _report("pair scores", sc.cpu().numpy(), C.scores_ref(tn, ut_r, s["p1"], s["p2"]), tol) <= tol


def _roc_cases(golden, gset):
    rng = np.random.default_rng(5)
    lab = gset["label"]
    one = np.zeros(5000, np.int64)
    one[1234] = 1
    neg_best = rng.standard_normal(4000)
    lab_nb = (rng.random(4000) < 0.3).astype(np.int64)
    lab_nb[np.argmax(neg_best)] = 0
    return {
        "raw": (golden["scores"], lab),
        "two_decimals": (np.round(golden["scores"], 2), lab),
        "all_equal": (np.full(3000, 0.25), (np.arange(3000) % 3 == 0).astype(np.int64)),
        "single_positive": (rng.standard_normal(5000), one),
        "best_is_negative": (neg_best, lab_nb),
    }


@pytest.mark.parametrize("case", ["raw", "two_decimals", "all_equal", "single_positive", "best_is_negative"])
def test_roc_table_on_cpu_scores(golden, gset, case):
    from msml_amd import ijb
    scores, label = _roc_cases(golden, gset)[case]
    tprs_r, auc_r, npts_r, fps_r, tps_r = C.roc_ref(scores, label)
    r = ijb.roc_points(scores, label, C.FPRS)
    keep = r["keep"].bool()
    assert r["n_points"] == npts_r
    assert np.array_equal(r["fps"][keep].cpu().numpy(), fps_r) and np.array_equal(r["tps"][keep].cpu().numpy(), tps_r)
    tprs, auc = ijb.roc_table(scores, label)
    print(case, "tprs", tprs, "auc", auc, "ref", auc_r, "points", npts_r)
    assert np.array_equal(tprs, tprs_r)
    assert abs(auc - auc_r) <= 1e-12 * abs(auc_r)
    if case == "raw":
        assert np.array_equal(tprs, golden["tprs"]) and npts_r == int(golden["n_points"])
        assert abs(auc - float(golden["auc"])) <= 1e-12 * float(golden["auc"])
    if case == "two_decimals":
        assert np.array_equal(tprs, golden["tprs_r2"]) and npts_r == int(golden["n_points_r2"])


def test_end_to_end_equals_the_golden_table(golden, gset):
    """Device scores into the device ROC; exact because the recorder proved the table does not move when every score
    moves by the tolerance."""
    from msml_amd import ijb
    out = ijb.evaluate_templates(gset["img_feats"], gset["templates"], gset["medias"], gset["p1"], gset["p2"],
                                 gset["label"], faceness=gset["faceness"])
    assert np.array_equal(out["tprs"], golden["tprs"])
    assert abs(out["auc"] - float(golden["auc"])) <= 1e-12 * float(golden["auc"])
    assert ijb.roc_points(out["scores"], gset["label"])["n_points"] == int(golden["n_points"])
    # a list of repeats is averaged: the same features twice give the same table
    two = ijb.evaluate_templates([gset["img_feats"]] * 2, gset["templates"], gset["medias"], gset["p1"], gset["p2"],
                                 gset["label"], faceness=gset["faceness"])
    assert torch.equal(two["scores"], out["scores"])
    again = ijb.evaluate_templates(None, None, None, None, None, gset["label"], scores=[out["scores"], two["scores"]])
    assert np.array_equal(again["tprs"], golden["tprs"])


def test_two_runs_are_bit_identical(gset):
    from msml_amd import ijb
    a, b = _chain(gset), _chain(gset)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    ra, rb = ijb.roc_points(a[2], gset["label"], C.FPRS), ijb.roc_points(b[2], gset["label"], C.FPRS)
    assert torch.equal(ra["fps"], rb["fps"]) and torch.equal(ra["keep"], rb["keep"])
    assert ra["auc"] == rb["auc"] and ra["nearest"] == rb["nearest"]


def test_unknown_pair_id_raises_before_launch(gset):
    from msml_amd import ijb
    tf, ut, _ = _chain(gset)
    p1 = gset["p1"].copy()
    p1[17] = int(ut.max()) + 5
    with pytest.raises(ValueError):
        ijb.pair_scores(tf, ut, p1, gset["p2"])
    p1[17] = 0                                       # below the smallest id
    with pytest.raises(ValueError):
        ijb.pair_scores(tf, ut, torch.from_numpy(p1).cuda(), gset["p2"])


def test_roc_accuracy_tarfar_equals_the_golden(golden):
    from msml_amd import verification as hv
    emb, issame = C.make_pairs(**C.GOLDEN_PAIRS)
    acc, tarfar = hv.roc_accuracy_tarfar(torch.from_numpy(emb).cuda(), issame)
    print("acc", acc, "tarfar", tarfar)
    assert acc == float(golden["sv_acc"]) and np.array_equal(tarfar, golden["sv_tarfar"])
    acc64, tarfar64 = hv.roc_accuracy_tarfar(torch.from_numpy(emb).double().cuda(), issame)
    assert acc64 == acc and np.array_equal(tarfar64, tarfar)
    bad = issame.copy()
    bad[np.flatnonzero(bad)[0]] = False              # one more different than same pair: the reference raises too
    with pytest.raises(ValueError):
        hv.roc_accuracy_tarfar(torch.from_numpy(emb).cuda(), bad)


def test_large_case_with_row_offsets_beyond_2_31_bytes():
    """200 000 images x (512 | 512) generated on the device, 20 000 templates, 2 M pairs, against the restatement.
    The features are a [:, :1024] view of a buffer with 3072 floats per row (2.4 GB), so the last rows start beyond
    2**31 bytes."""
    from msml_amd import ijb
    n, e, t, p, ld = 200000, 512, 20000, 2000000, 3072
    g = torch.Generator(device="cuda").manual_seed(3)
    buf = torch.empty(n, ld, dtype=torch.float32, device="cuda")
    feats = buf[:, :2 * e]
    feats.copy_(torch.randn(n, 2 * e, generator=g, device="cuda"))
    # uneven templates: template of image i = floor(t * u^3), every template gets its first image from the front
    u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    tid = (u ** 3 * t).long().clamp_(max=t - 1)
    tid[:t] = torch.randperm(t, generator=g, device="cuda")
    templates = (tid * 3 + 11).cpu().numpy()
    medias = torch.randint(0, 40, (n,), generator=g, device="cuda").cpu().numpy()
    face = torch.rand(n, generator=g, device="cuda") * 0.8 + 0.2
    a = torch.randint(0, t, (p,), generator=g, device="cuda").sort()[0]
    b = torch.randint(0, t, (p,), generator=g, device="cuda")
    p1, p2 = (a * 3 + 11).cpu().numpy(), (b * 3 + 11).cpu().numpy()
    assert feats[-1].data_ptr() - feats.data_ptr() > 2 ** 31
    tf, ut = ijb.template_features(feats, templates, medias, face)
    sc = ijb.pair_scores(tf, ut, p1, p2)
    x = C.input_feats(feats.cpu().numpy(), face.cpu().numpy())
    tn, ut_r, rows = C.pool_ref(x, templates, medias)
    del x
    tol = C.tolerance(rows, e)
    assert np.array_equal(ut, ut_r)
    assert _report("large template feats (R = %d)" % rows, tf.cpu().numpy(), tn, tol) <= tol
    assert _report("large pair scores", sc.cpu().numpy(), C.scores_ref(tn, ut_r, p1, p2), tol) <= tol
    label = (torch.rand(p, generator=g, device="cuda") < 0.1).cpu().numpy().astype(np.int64)
    tprs_r, auc_r, npts_r, _, _ = C.roc_ref(sc.cpu().numpy(), label)
    tprs, auc = ijb.roc_table(sc, label)
    assert np.array_equal(tprs, tprs_r) and abs(auc - auc_r) <= 1e-12 * auc_r
