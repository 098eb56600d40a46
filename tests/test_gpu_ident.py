"""GPU tests of the 1:N identification path (msml_amd/identify.py, csrc/search.hip) against the numpy restatement of
tests/ident_cases.py.

Bounds.  f64 scores: E * 2^-52 * |p| |g| (recursive summation of E products, E * 2^-53, doubled for the restatement's
own rounding): 1.1e-13 at E = 512 on unit rows.  f32 scores: (E + 2) * 2^-24 * |p| |g| (E products, plus the rounding
of both inputs to f32): 3.1e-5 at E = 512.  Integer data is exact in both types.  Indices are compared exactly
wherever the reference gaps exceed the bound (asserted on the CPU first) or the data is exact."""
import numpy as np
import pytest
import torch

from tests import ident_cases as C

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]


def _search(p, g, k, splits=None, dtype=torch.float64):
    from msml_amd import identify
    s, i = identify.search_topk(p, g, k=k, splits=splits, dtype=dtype)
    assert s.is_cuda and i.is_cuda and s.dtype == dtype and i.dtype == torch.int32
    assert tuple(s.shape) == tuple(i.shape) == (p.shape[0], k)
    return s, i


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("splits", [1, 2])
def test_lane_maps_on_exact_integer_data(dtype, splits):
    """P != G and asymmetric data: a transposed or mis-rowed C/D read cannot pass; every score is an exact integer."""
    rng = np.random.default_rng(11)
    p, g = C.integer_rows(rng, 70, 36), C.integer_rows(rng, 75, 36)
    want_s, want_i = C.topk_ref(p, g, 32)
    s, i = _search(p, g, 32, splits, dtype)
    assert np.array_equal(s.cpu().numpy().astype(np.float64), want_s)
    assert np.array_equal(i.cpu().numpy(), want_i)            # ties included: ascending gallery row
    assert (np.diff(want_s, axis=1) == 0).any()


@pytest.mark.parametrize("n", range(len(C.EDGE_SHAPES)), ids=["%dx%dx%d_k%d_s%s" % c for c in C.EDGE_SHAPES])
def test_edge_shapes_f64(n):
    P, G, E, k, splits = C.EDGE_SHAPES[n]
    rng = np.random.default_rng(100 + n)
    p, g = C.unit_rows(rng, P, E), C.unit_rows(rng, G, E)
    full = C.scores_full(p, g)
    gap = C.min_gap(full, k)
    assert gap > 1e-9, gap
    want_s, want_i = C.topk_ref(p, g, k, full)
    s, i = _search(p, g, k, splits)
    tol = E * 2.0 ** -52
    err = float(np.abs(s.cpu().numpy() - want_s).max())
    print("P %d G %d E %d k %d splits %s: max score err %.3e (bound %.3e), min gap %.2e" % (P, G, E, k, splits, err, tol, gap))
    assert np.array_equal(i.cpu().numpy(), want_i)            # every position
    assert err <= tol


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_bit_identity_across_splits_and_runs(dtype):
    rng = np.random.default_rng(21)
    p = torch.from_numpy(C.unit_rows(rng, 130, 132)).cuda()
    g = torch.from_numpy(C.unit_rows(rng, 450, 132)).cuda()
    first = _search(p, g, 32, 1, dtype)
    for splits in (1, 2, 3, 7):
        s, i = _search(p, g, 32, splits, dtype)
        assert torch.equal(s, first[0]) and torch.equal(i, first[1]), splits


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_duplicated_gallery_rows_come_back_in_row_order(dtype):
    """Equal rows give equal bits whatever their tile or split, so they tie and list in ascending row order."""
    rng = np.random.default_rng(22)
    base = C.unit_rows(rng, 40, 64)
    g = base[np.arange(200) % 40]                             # row r == row r + 40 == ... (5 copies, 4 column tiles)
    p = C.unit_rows(rng, 67, 64)
    for splits in (1, 4):
        s, i = _search(p, g, 20, splits, dtype)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        grp = i.reshape(67, 4, 5)
        assert (s.reshape(67, 4, 5) == s.reshape(67, 4, 5)[:, :, :1]).all()
        assert (np.diff(grp, axis=2) == 40).all() and (grp[:, :, 0] < 40).all()
        if dtype == torch.float64:                            # the 4 best distinct rows (f32 may swap near ties)
            assert np.array_equal(grp[:, :, 0], C.topk_ref(p, base, 4)[1])


def test_f32_on_random_data():
    P, G, E, k = 130, 200, 512, 32
    rng = np.random.default_rng(23)
    p, g = C.unit_rows(rng, P, E), C.unit_rows(rng, G, E)
    full = C.scores_full(p, g)
    want_s, _ = C.topk_ref(p, g, k, full)
    tol = (E + 2) * 2.0 ** -24
    for splits in (1, 3):
        s, i = _search(p, g, k, splits, torch.float32)
        s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy()
        assert i.min() >= 0 and i.max() < G
        err = float(np.abs(s - np.take_along_axis(full, i.astype(np.int64), 1)).max())
        print("f32 splits %d: max err against the f64 dot of the returned index %.3e (bound %.3e)" % (splits, err, tol))
        assert err <= tol
        assert (np.diff(s, axis=1) <= 0).all()                # non-increasing
        assert all(len(set(row)) == k for row in i.tolist())  # distinct
        assert (s[:, -1] >= want_s[:, -1] - tol).all()


@pytest.fixture(scope="module")
def e2e():
    probe, p_sub, gallery, g_sub = C.make_identification(**C.END_TO_END)
    full = C.scores_full(probe, gallery)
    return probe, p_sub, gallery, g_sub, full, C.metrics_ref(full, C.mate_rows_ref(p_sub, g_sub), 10)


def _same_metrics(got, want, tol):
    assert np.array_equal(got["mate_rank"].cpu().numpy(), want["mate_rank"])
    assert (got["n_mated"], got["n_nonmated"]) == (want["n_mated"], want["n_nonmated"])
    assert np.array_equal(got["cmc_count"], want["cmc_count"]) and np.array_equal(got["tpir_count"], want["tpir_count"])
    assert np.array_equal(got["cmc"], want["cmc"]) and np.array_equal(got["tpir"], want["tpir"])
    assert np.array_equal(got["fpir_achieved"], want["fpir_achieved"])
    assert np.abs(got["thresholds"] - want["thresholds"]).max() <= tol


def test_identify_end_to_end(e2e):
    from msml_amd import identify
    probe, p_sub, gallery, g_sub, full, want = e2e
    got = identify.identify(probe, p_sub, gallery, g_sub)
    assert got["topk_scores"].shape == (130, 10) and got["mate_rank"].is_cuda
    _same_metrics(got, want, C.END_TO_END["e"] * 2.0 ** -52)
    assert 0.3 < got["cmc"][0] < 0.95 and 0.1 < got["tpir"][1] < 0.9
    # inputs already on the device, another k, closed set only
    got = identify.identify(torch.from_numpy(probe).cuda(), p_sub, torch.from_numpy(gallery).cuda(), g_sub,
                            ranks=(1, 20), fpirs=(), k=25, splits=3)
    want = C.metrics_ref(full, C.mate_rows_ref(p_sub, g_sub), 25, (1, 20), ())
    _same_metrics({**got, "thresholds": np.zeros(1)}, {**want, "thresholds": np.zeros(1)}, 0.0)


def test_identify_templates_equals_identify_on_the_gathered_rows(e2e):
    from msml_amd import identify
    probe, p_sub, gallery, g_sub, _, _ = e2e
    rng = np.random.default_rng(31)
    feats = np.concatenate([gallery, probe])[(order := rng.permutation(430))]
    where = np.argsort(order)                                  # row of feats holding original row j
    ut = np.sort(rng.choice(np.arange(10, 5000), 430, replace=False)).astype(np.int64)
    tf = torch.from_numpy(feats).cuda()
    got = identify.identify_templates(tf, ut, ut[where[:300]], g_sub, ut[where[300:]], p_sub)
    want = identify.identify(probe, p_sub, gallery, g_sub)
    assert torch.equal(got["topk_scores"], want["topk_scores"]) and torch.equal(got["topk_index"], want["topk_index"])
    assert torch.equal(got["mate_rank"], want["mate_rank"])
    for key in ("cmc", "tpir", "thresholds", "fpir_achieved"):
        assert np.array_equal(got[key], want[key]), key
    with pytest.raises(ValueError):
        identify.identify_templates(tf, ut, np.array([1]), g_sub[:1], ut[where[300:]], p_sub)


def test_distractor_ranks(e2e):
    from msml_amd import identify
    _, _, gallery, _, _, _ = e2e
    rng = np.random.default_rng(32)
    mate = C.unit_rows(rng, 90, 128)
    probe = mate + 3.0 / np.sqrt(128) * rng.standard_normal((90, 128))
    probe /= np.linalg.norm(probe, axis=1, keepdims=True)
    want, ms = C.distractor_ranks_ref(probe, mate, gallery, 10)
    # no distractor score within the bound of a mate score: the ranks are decided
    assert np.abs(C.scores_full(probe, gallery) - ms[:, None]).min() > 1e-9
    got = identify.distractor_ranks(probe, mate, gallery, k=10)
    assert np.array_equal(got["rank"].cpu().numpy(), want) and got["rank"].dtype == torch.int32
    assert got["rank1"] == float((want == 0).mean()) and 0.2 < got["rank1"] < 0.95
    assert np.abs(got["mate_scores"].cpu().numpy() - ms).max() <= 128 * 2.0 ** -52
    assert (want == 10).any() or want.max() >= 3                # the cap or deep ranks occur


def test_refusals_on_the_device():
    from msml_amd import identify
    p, g = np.ones((3, 8)), np.ones((6, 8))
    bad = p.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        identify.search_topk(bad, g, k=2)
    bad[1, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        identify.search_topk(p, np.r_[g, bad], k=2, dtype=torch.float32)
    with pytest.raises(ValueError):
        identify.search_topk(p, g, k=7)                        # k > G
    with pytest.raises(ValueError):
        identify.search_topk(p, np.ones((6, 12)), k=2)         # channel counts differ
    with pytest.raises(ValueError):
        identify.search_topk(np.ones((3, 6)), np.ones((6, 6)), k=2)   # E % 4 != 0
    with pytest.raises(ValueError):
        identify.search_topk(np.ones(8), g, k=2)               # not [rows][E]
    s, i = identify.search_topk(p, g, k=6)                     # all scores tie: ascending rows
    assert i.cpu().tolist() == [list(range(6))] * 3 and (s == 8.0).all()
