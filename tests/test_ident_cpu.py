"""CPU-side checks of the 1:N identification path: the numpy restatement (tests/ident_cases.py) on a hand-made case,
mate_rows and identification_metrics of msml_amd/identify.py on CPU arrays against it, their refusals, and the C entry
points of csrc/search.hip (declared, exported, stream last, refusing bad arguments before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

from msml_amd import _lib, identify
from tests import ident_cases as C

ENTRY = "msml_search_topk"

# 3 probes x 4 gallery rows; probe 0 ties on rows 1 and 3, probe 2 ties 0.0 with -0.0 on rows 0 and 2
HAND = np.array([[0.5, 0.9, 0.1, 0.9],
                 [0.2, 0.1, 0.8, 0.3],
                 [0.0, -0.5, -0.0, -0.7]])


def _full_as_search(full):
    """A probe / gallery pair whose score matrix is `full`: identity gallery."""
    return full, np.eye(full.shape[1])


def test_hand_made_case_with_a_tie():
    p, g = _full_as_search(HAND)
    s, i = C.topk_ref(p, g, 3)
    assert i.tolist() == [[1, 3, 0], [2, 3, 0], [0, 2, 1]]
    assert s.tolist() == [[0.9, 0.9, 0.5], [0.8, 0.3, 0.2], [0.0, -0.0, -0.5]]
    mate = np.array([3, 0, -1], np.int32)               # probe 0: the mate ties with row 1 and comes second
    want = C.metrics_ref(HAND, mate, 3, ranks=(1, 2, 3), fpirs=(0.0,))
    assert want["mate_rank"].tolist() == [1, 2, -1] and want["cmc"].tolist() == [0.0, 0.5, 1.0]
    assert want["thresholds"].tolist() == [0.0] and want["tpir_count"].tolist() == [0]
    got = identify.identification_metrics(s, i, mate, ranks=(1, 2, 3), fpirs=(0.0,))
    assert got["mate_rank"].tolist() == [1, 2, -1] and got["mate_rank"].dtype == torch.int32
    assert got["cmc"].tolist() == [0.0, 0.5, 1.0] and (got["n_mated"], got["n_nonmated"]) == (2, 1)
    assert got["thresholds"].tolist() == [0.0] and got["fpir_achieved"].tolist() == [0.0]
    # the mate outside the list: rank k
    got = identify.identification_metrics(s[:, :1], i[:, :1], mate, ranks=(1,), fpirs=())
    assert got["mate_rank"].tolist() == [1, 1, -1] and got["cmc"].tolist() == [0.0]
    assert got["thresholds"].size == 0 and got["tpir"].size == 0


def test_mate_rows():
    g = np.array([40, 7, 19, 1000], np.int64)
    assert identify.mate_rows(np.array([19, 8, 1000, 7, 40, -3]), g).tolist() == [2, -1, 3, 1, 0, -1]
    assert identify.mate_rows(np.array([19]), g).dtype == np.int32
    assert identify.mate_rows(torch.tensor([7, 5000]), torch.from_numpy(g)).tolist() == [1, -1]
    with pytest.raises(ValueError, match="subject 7"):
        identify.mate_rows(np.array([1]), np.array([7, 3, 7]))
    with pytest.raises(ValueError):
        identify.mate_rows(np.array([1.0, 2.0]), g)
    with pytest.raises(ValueError):
        identify.mate_rows(np.array([1]), np.array([1.5, 2.5]))
    with pytest.raises(ValueError):
        identify.mate_rows(np.array([1]), np.array([], np.int64))


def _seeded(seed, integer):
    rng = np.random.default_rng(seed)
    p_n, g_n, e = 90, 140, 16
    if integer:
        gallery = C.integer_rows(rng, g_n, e, -2, 2)
        subjects = rng.permutation(g_n * 3)[:g_n]
        row, is_mated = rng.integers(0, g_n, p_n), rng.random(p_n) < 0.6
        probe = np.where(is_mated[:, None], gallery[row] + C.integer_rows(rng, p_n, e, -1, 1),
                         C.integer_rows(rng, p_n, e, -2, 2))
        return probe, np.where(is_mated, subjects[row], 10 ** 6 + np.arange(p_n)), gallery, subjects
    return C.make_identification(seed, p_n, g_n, e, 0.6, 1.5)


@pytest.mark.parametrize("seed,integer", [(1, False), (2, False), (3, True), (4, True)])
@pytest.mark.parametrize("as_numpy", [False, True])
def test_metrics_on_cpu_arrays_equal_the_restatement(seed, integer, as_numpy):
    probe, p_sub, gallery, g_sub = _seeded(seed, integer)
    full = C.scores_full(probe, gallery)
    k, ranks, fpirs = 12, (1, 3, 12), (0.0, 0.05, 0.3)
    mate = identify.mate_rows(p_sub, g_sub)
    assert np.array_equal(mate, C.mate_rows_ref(p_sub, g_sub))
    s, i = C.topk_ref(probe, gallery, k, full)
    if integer:                                         # ties inside the lists and at the thresholds
        assert (np.diff(s, axis=1) == 0).any()
    want = C.metrics_ref(full, mate, k, ranks, fpirs)
    args = (s, i, mate) if as_numpy else (torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(mate))
    got = identify.identification_metrics(*args, ranks=ranks, fpirs=fpirs)
    assert np.array_equal(got["mate_rank"].numpy(), want["mate_rank"])
    assert (got["n_mated"], got["n_nonmated"]) == (want["n_mated"], want["n_nonmated"])
    for key in ("cmc_count", "tpir_count", "cmc", "tpir", "thresholds", "fpir_achieved"):
        assert np.array_equal(got[key], want[key]), key
    assert (got["fpir_achieved"] <= np.array(fpirs)).all()
    assert 0 < got["cmc"][0] <= got["cmc"][1] <= got["cmc"][2] <= 1.0


def test_metrics_refusals():
    s, i = C.topk_ref(*_full_as_search(HAND), 3)
    mate = np.array([3, 0, -1], np.int32)
    with pytest.raises(ValueError):
        identify.identification_metrics(s, i, mate, ranks=(1, 4), fpirs=())          # max(ranks) > k
    with pytest.raises(ValueError):
        identify.identification_metrics(s, i, np.array([-1, -1, -1]), ranks=(1,), fpirs=())   # nobody is mated
    with pytest.raises(ValueError):
        identify.identification_metrics(s, i, np.array([3, 0, 1]), ranks=(1,), fpirs=(0.1,))   # no non-mated probe
    identify.identification_metrics(s, i, np.array([3, 0, 1]), ranks=(1,), fpirs=())           # closed set: fine
    with pytest.raises(ValueError):
        identify.identification_metrics(s, i, mate, ranks=(1,), fpirs=(1.0,))
    with pytest.raises(ValueError):
        identify.identification_metrics(s, i, mate, ranks=(1,), fpirs=(-0.1,))
    with pytest.raises(ValueError):
        identify.identification_metrics(s, i[:2], mate, ranks=(1,), fpirs=())
    with pytest.raises(ValueError):
        identify.identification_metrics(s, i, mate[:2], ranks=(1,), fpirs=())


def test_search_topk_refuses_before_touching_the_device():
    """k and dtype are checked first, so these raise on a machine without a GPU too."""
    p, g = np.zeros((2, 8)), np.zeros((5, 8))
    for k in (0, 33, -1):
        with pytest.raises(ValueError, match="outside 1..32"):
            identify.search_topk(p, g, k=k)
    with pytest.raises(ValueError, match="dtype"):
        identify.search_topk(p, g, k=1, dtype=torch.bfloat16)


def test_end_to_end_generator_is_not_degenerate():
    probe, p_sub, gallery, g_sub = C.make_identification(**C.END_TO_END)
    mate = C.mate_rows_ref(p_sub, g_sub)
    m = C.metrics_ref(C.scores_full(probe, gallery), mate, 10)
    print("cmc(1) %.3f  tpir@0.1 %.3f  mated %d / %d" % (m["cmc"][0], m["tpir"][1], m["n_mated"], len(mate)))
    assert 0.3 < m["cmc"][0] < 0.95 and 0.1 < m["tpir"][1] < 0.9
    assert m["cmc"][0] < m["cmc"][2] and m["n_nonmated"] >= 30


def test_edge_shape_sets_have_no_near_ties():
    """The GPU test demands exact index equality at every position of these sets; that needs the gaps of the first
    k + 1 reference scores of every row far above the f64 error bound (1.1e-13 at E = 512)."""
    for n, (p, g, e, k, _) in enumerate(C.EDGE_SHAPES):
        rng = np.random.default_rng(100 + n)
        gap = C.min_gap(C.scores_full(C.unit_rows(rng, p, e), C.unit_rows(rng, g, e)), k)
        print(p, g, e, k, "min gap %.2e" % gap)
        assert gap > 1e-9


def test_entries_declared_exported_and_validating():
    protos = _lib.parse_header()
    lib = _lib.load()
    for name in (ENTRY, "msml_search_topk_splits", "msml_search_topk_workspace"):
        assert name in protos and hasattr(lib, name), name
    assert protos[ENTRY][1][-1][1] == "stream"
    assert protos["msml_search_topk_workspace"][0] is ctypes.c_size_t
    src = open(_lib.HEADER).read()
    sect = src[src.index("1:N identification"):]
    assert "datasets/benchmarks/get_list.py:138-208" in sect and "datasets/benchmarks/get_list.py:100-135" in sect
    assert "MSML_F64" in src and _lib.F64 == 3

    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    a += -a % 16
    F32, F64 = _lib.F32, _lib.F64

    def run(P=8, G=40, E=8, k=5, splits=1, dtype=F64, probe=a, gallery=a, scores=a, index=a, ws=a, ws_bytes=1 << 20):
        return lib.msml_search_topk(probe, P, gallery, G, E, k, splits, dtype, scores, index, ws, ws_bytes, None)

    assert run(E=6) == -1 and b"multiple of 4" in lib.msml_last_error()
    assert run(E=0) == -1
    assert run(k=0) == -1 and b"outside 1..32" in lib.msml_last_error()
    assert run(k=33) == -1
    assert run(G=4, k=5) == -1 and b"exceeds" in lib.msml_last_error()
    for null in ("probe", "gallery", "scores", "index"):
        assert run(**{null: None}) == -1, null
        assert b"null pointer" in lib.msml_last_error()
    assert run(splits=2, ws=None) == -1
    need = lib.msml_search_topk_workspace(8, 5, 2)
    assert need == 2 * 8 * 5 * 12                        # splits * P * k entries, never P x G
    assert run(splits=2, ws_bytes=need - 1) == -1 and b"workspace" in lib.msml_last_error()
    assert run(splits=0) == -1 and run(splits=65536) == -1
    assert run(dtype=_lib.BF16) == -1 and run(P=0) == -1 and run(G=0, k=1) == -1
    assert run(probe=a + 8) == -1 and b"aligned" in lib.msml_last_error()
    assert lib.msml_search_topk_workspace(8, 5, 1) == 0
    # the default split count: at least one, never more than column tiles, more for few probes than for many
    few, many = lib.msml_search_topk_splits(64, 1000000, 10), lib.msml_search_topk_splits(19600, 1772, 10)
    assert lib.msml_search_topk_splits(1, 1, 1) == 1 and lib.msml_search_topk_splits(5, 64, 8) == 1
    assert 1 <= many <= 28 and many < few <= 15625 and few * 1 >= 256
    assert lib.msml_search_topk_splits(0, 10, 1) == 0


def test_both_call_routes_reach_the_new_entries():
    """The fast-call binding wraps the three entries (the size_t one included) and gives the answers of ctypes."""
    import __graft_entry__ as ge
    assert ge.build_fastabi()
    fa = _lib._fastabi()
    assert fa, "msml_amd/_msml_fastabi.so did not load"
    lib = _lib.load()
    assert fa.msml_search_topk_workspace(1000, 10, 7) == lib.msml_search_topk_workspace(1000, 10, 7) == 840000
    assert fa.msml_search_topk_workspace(3000000, 32, 1000) == 3000000 * 32 * 1000 * 12        # beyond 32 bits
    assert fa.msml_search_topk_splits(3530, 1000000, 10) == lib.msml_search_topk_splits(3530, 1000000, 10)
    assert fa.msml_search_topk(None, 1, None, 1, 4, 1, 1, _lib.F64, None, None, None, 0, None) == -1
    assert _lib.call_status(ENTRY, None, 1, None, 1, 4, 1, 1, _lib.F64, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.msml_last_error()
