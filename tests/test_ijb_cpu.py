"""CPU-side checks of the template-verification path: the numpy / sklearn restatement the GPU tests compare against
reproduces the golden recorded from the reference (tools/make_golden_ijb.py), segment_layout on hand-made cases, and
the new C entry points (declared, exported, cited, validating their arguments before any launch)."""
import os

import numpy as np
import pytest

from msml_amd import _lib, ijb
from tests import ijb_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_ijb.npz")
ENTRIES = ("msml_template_pool", "msml_template_pair_score", "msml_roc_block_counts", "msml_roc_points",
           "msml_roc_reduce", "msml_pair_cosdist", "msml_pair_cosdist_f64", "msml_rank_count")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_restatement_reproduces_the_golden(golden):
    s = C.make_set(**C.GOLDEN_SET)
    tn, ut, rows = C.pool_ref(C.input_feats(s["img_feats"], s["faceness"]), s["templates"], s["medias"])
    tol = C.tolerance(rows, C.GOLDEN_SET["e"])
    assert rows == int(golden["max_rows"]) and np.array_equal(ut, golden["ut"])
    assert np.abs(tn - golden["tn"]).max() <= tol
    sc = C.scores_ref(tn, ut, s["p1"], s["p2"])
    assert np.abs(sc - golden["scores"]).max() <= tol
    tprs, auc, npts, _, _ = C.roc_ref(golden["scores"], s["label"])
    assert np.array_equal(tprs, golden["tprs"]) and npts == int(golden["n_points"]) and auc == float(golden["auc"])
    tprs, auc, npts, _, _ = C.roc_ref(np.round(golden["scores"], 2), s["label"])
    assert np.array_equal(tprs, golden["tprs_r2"]) and npts == int(golden["n_points_r2"])
    assert auc == float(golden["auc_r2"])
    # the restated scores give the same table: the set is stable under the bound
    tprs, _, npts, _, _ = C.roc_ref(sc, s["label"])
    assert np.array_equal(tprs, golden["tprs"]) and npts == int(golden["n_points"])
    # not a degenerate curve
    assert 0.3 < golden["tprs"][0] < golden["tprs"][3] < golden["tprs"][5] < 1.0


def test_start_verification_restatement_reproduces_the_golden(golden):
    emb, issame = C.make_pairs(**C.GOLDEN_PAIRS)
    assert int(issame.sum()) * 2 == len(issame)
    acc, tarfar = C.start_verification_ref(emb, issame)
    assert acc == float(golden["sv_acc"]) and np.array_equal(tarfar, golden["sv_tarfar"])
    assert tarfar[4] == 0.0 and 0.5 < tarfar[3] <= tarfar[0] < 1.0


def test_segment_layout_hand_made():
    #            row: 0   1   2   3   4   5   6   7
    templates = [50, 7, 50, 7, 900, 50, 7, 50]
    medias = [3, 3, 1, 9, 3, 3, 3, 1]          # media 3 is used by templates 50, 7 and 900
    lay = ijb.segment_layout(templates, medias)
    assert lay.unique_templates.tolist() == [7, 50, 900]
    # template 7: media 3 -> rows 1, 6; media 9 -> row 3.  template 50: media 1 -> rows 2, 7; media 3 -> rows 0, 5.
    assert lay.order.tolist() == [1, 6, 3, 2, 7, 0, 5, 4]
    assert lay.media_start.tolist() == [0, 2, 3, 5, 7, 8]
    assert lay.template_media_start.tolist() == [0, 2, 4, 5]
    assert lay.launch.tolist() == [1, 0, 2] and lay.max_rows == 4
    assert all(a.dtype == np.int32 for a in (lay.order, lay.media_start, lay.template_media_start, lay.launch))
    one = ijb.segment_layout(np.array([4]), np.array([-2]))          # a single image
    assert one.order.tolist() == [0] and one.media_start.tolist() == [0, 1]
    assert one.template_media_start.tolist() == [0, 1] and one.unique_templates.tolist() == [4]


def test_segment_layout_drives_the_reference_pooling():
    """Walking the layout the way the kernel does (media ascending, rows in original order) gives the restatement."""
    s = C.make_set(seed=3, n_img=700, e=8, n_tmpl=60, n_ident=20, noise=1.0, n_pairs=100)
    x = C.input_feats(s["img_feats"], s["faceness"])
    lay = ijb.segment_layout(s["templates"], s["medias"])
    out = np.zeros((lay.unique_templates.size, 8))
    for t in range(out.shape[0]):
        for m in range(lay.template_media_start[t], lay.template_media_start[t + 1]):
            rows = lay.order[lay.media_start[m]:lay.media_start[m + 1]]
            assert (np.diff(rows) > 0).all() and (s["templates"][rows] == lay.unique_templates[t]).all()
            assert len(set(s["medias"][rows])) == 1
            out[t] += x[rows].sum(0) / len(rows)
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    tn, ut, rows = C.pool_ref(x, s["templates"], s["medias"])
    assert np.array_equal(ut, lay.unique_templates) and rows == lay.max_rows
    assert np.abs(out - tn).max() <= C.tolerance(rows, 8)
    assert sorted(lay.launch.tolist()) == list(range(out.shape[0]))


def test_segment_layout_rejects_bad_input():
    with pytest.raises(ValueError):
        ijb.segment_layout([], [])
    with pytest.raises(ValueError):
        ijb.segment_layout([1, 2], [1])
    with pytest.raises(ValueError):
        ijb.segment_layout([1.5, 2.0], [1, 1])


def test_unknown_pair_id_raises_on_the_host():
    with pytest.raises(ValueError, match="template id 8"):
        ijb.template_rows(np.array([3, 7, 9]), np.array([3, 8]), device="cpu")
    with pytest.raises(ValueError):
        ijb.template_rows(np.array([3, 7, 9]), np.array([12]), device="cpu")
    assert ijb.template_rows(np.array([3, 7, 9]), np.array([9, 3, 7, 9]), device="cpu").tolist() == [2, 0, 1, 2]


def test_header_entries_cite_the_reference_and_validate():
    protos = _lib.parse_header()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in protos and hasattr(lib, name), name
        assert protos[name][1][-1][1] == "stream", name
    src = open(_lib.HEADER).read()
    sect = src[src.index("template (IJB-B / IJB-C) verification"):]
    for cite in ("eval/qeval_ijbc.py:303-337", "eval/qeval_ijbc.py:343-369", "eval/qeval_ijbc.py:565-585",
                 "eval/qeval_mxnet.py:422-483", "eval/qeval_mxnet.py:461-478"):
        assert cite in sect, cite
    # argument validation happens before any launch
    assert lib.msml_template_pool(None, 1, 4, 4, 0, None, None, None, None, None, 1, None, None) == -1
    assert lib.msml_template_pool(16, 10, 6, 6, 0, None, 16, 16, 16, 16, 2, 16, None) == -1
    assert b"multiple of 4" in lib.msml_last_error()
    assert lib.msml_template_pool(16, 10, 8, 8, 1, None, 16, 16, 16, 16, 2, 16, None) == -1      # ld < 2E
    assert lib.msml_template_pair_score(16, 4, 7, 16, 16, 3, 16, None) == -1
    assert lib.msml_roc_reduce(16, 16, 5, 16, 17, 16, 16, None) == -1
    assert lib.msml_roc_block_counts(None, None, 0, None, None) == -1
    assert lib.msml_rank_count(16, 0, 16, 1, 1, 16, None) == -1
    assert lib.msml_roc_blocks(1) == 1 and lib.msml_roc_blocks(4096) == 1 and lib.msml_roc_blocks(4097) == 2
    assert lib.msml_roc_reduce_blocks(257) == 2
