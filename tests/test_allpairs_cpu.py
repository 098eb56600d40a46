"""CPU-side checks of the all-pairs verification path: the radix restatement against sort-and-index, the host side of
msml_amd/allpairs.py (subject coding, pair counts, the narrowing walk, shared ranges, the collect switch, the final
cross-check) on a numpy backend against the full-matrix restatement of tests/allpairs_cases.py, every refusal, and the
C entry points of csrc/allpairs.hip (declared, exported, refusing bad arguments before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

from msml_amd import _lib, allpairs
from tests import allpairs_cases as C

ENTRY = "msml_allpairs_pass"
NP_OF = {torch.float32: np.float32, torch.float64: np.float64}


def test_keys_order_as_scores_and_come_back():
    x = np.array([-np.inf, -3.5, -1e-300, -0.0, 0.0, 1e-300, 0.25, 7.0, np.inf])
    k = C.key64(x)
    assert k.dtype == np.uint64 and k[3] == k[4] == 1 << 63 and (np.diff(k.astype(object)) >= 0).all()
    assert np.array_equal(k, allpairs.score_keys(x))
    assert [allpairs.key_score(v, 64) for v in k] == (x + 0.0).tolist()
    x32 = np.array([-2.0, -0.0, 0.0, 1.5, 3.0], np.float32)
    k = C.key32(x32)
    assert k.dtype == np.uint32 and k.tolist() == sorted(k.tolist()) and k[1] == k[2] == 1 << 31
    assert np.array_equal(k, allpairs.score_keys(x32))
    assert [allpairs.key_score(v, 32) for v in k] == [-2.0, 0.0, 0.0, 1.5, 3.0]


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("cap", [1, 64, 1 << 20])
def test_radix_select_equals_sort_and_index(width, cap):
    rng = np.random.default_rng(width + cap)
    s = np.concatenate([rng.standard_normal(5000) * 0.1, rng.integers(-3, 4, 3000).astype(np.float64), [0.0, -0.0]])
    keys = C.key32(s.astype(np.float32)) if width == 32 else C.key64(s)
    order = np.sort(keys)[::-1]
    deep = 0
    for a in (0, 1, 17, 2999, 5000, 7999, len(s) - 1):
        key, above, levels = C.radix_select_ref(keys, a, width, 12, cap)
        assert key == int(order[a]) and above == int((keys > order[a]).sum()) <= a, (a, cap)
        deep = max(deep, levels)
    if cap == 1:
        assert deep == (width + 11) // 12               # tied keys narrow down to a single key
    if cap == 1 << 20:
        assert deep == 0                                # everything fits: sorted at once


def _case(kind, seed, symmetric):
    if kind == "integer":
        probe, ps, gallery, gs = C.integer_case(seed, 40, 55, 16)
        if symmetric:
            gallery, gs = None, None
    else:
        x, ids = C.make_verification(seed, 40, 16, 2.0)
        probe, ps, gallery, gs = (x, ids, None, None) if symmetric else C.split_rows(x, ids)
    full = probe @ (probe if symmetric else gallery).T
    return probe, ps, gallery, gs, full


def _same(got, want):
    assert (got["n_genuine"], got["n_impostor"]) == (want["n_genuine"], want["n_impostor"])
    for key in ("thresholds", "far_count", "tar_count", "far_achieved", "tar"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    assert got["far_count"].dtype == got["tar_count"].dtype == np.int64 and got["thresholds"].dtype == np.float64


FARS = (0.0, 1e-3, 1e-2, 1e-1, 0.5, 0.999)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("kind", ["integer", "real"])
@pytest.mark.parametrize("cap", [1, 64, 1 << 20])
def test_roc_on_a_numpy_backend_equals_the_restatement(kind, symmetric, dtype, cap):
    probe, ps, gallery, gs, full = _case(kind, 5, symmetric)
    scores = full.astype(NP_OF[dtype])                  # the score matrix the backend serves, in the type of the run
    want = C.allpairs_ref(scores.astype(np.float64), ps, gs, FARS, symmetric)
    if kind == "integer":                               # ties at the thresholds: fewer false accepts than the position
        assert (want["far_count"] < np.floor(np.array(FARS) * want["n_impostor"])).any()
    be = C.NumpyBackend(scores, ps, gs, symmetric)
    got = allpairs.all_pairs_roc(probe, ps, gallery, gs, fars=FARS, dtype=dtype, collect_cap=cap, backend=be)
    _same(got, want)
    assert (got["far_count"] <= np.floor(np.array(FARS) * got["n_impostor"])).all()
    assert got["passes"] == len(be.log) and be.log[-1][0] == "count"
    kinds = [c[0] for c in be.log]
    width = 32 if dtype == torch.float32 else 64
    if cap == 1 << 20:                                  # all impostors fit: one collect of the whole key space
        assert be.log[:-1] == [("collect", (0, 0))]
    else:                                               # pass 1 is one histogram for all targets
        assert be.log[0] == ("hist", ((0, 0),), 12)
    if cap == 1 and kind == "integer":                  # tied scores: down to single keys, the last level narrower
        assert any(c[0] == "hist" and c[2] == width % 12 and c[1][0][1] == width - width % 12 for c in be.log)
    for c in be.log:                                    # a pass takes what its LDS histogram holds
        if c[0] == "hist":
            assert 1 <= len(c[1]) <= allpairs.HIST_BINS >> c[2] and len(set(c[1])) == len(c[1])


def test_passes_grow_as_the_cap_shrinks_and_targets_share_ranges():
    probe, ps, gallery, gs, full = _case("real", 6, False)
    seen = []
    for cap in (1 << 20, 64, 1):
        be = C.NumpyBackend(full, ps, gs, False)
        got = allpairs.all_pairs_roc(probe, ps, gallery, gs, fars=FARS, collect_cap=cap, backend=be)
        seen.append(got["passes"])
    assert seen[0] == 2 and seen[0] < seen[1] < seen[2], seen
    be = C.NumpyBackend(full, ps, gs, False)            # two equal targets: one range, one histogram, one collect
    got = allpairs.all_pairs_roc(probe, ps, gallery, gs, fars=(0.01, 0.01), collect_cap=4, backend=be)
    assert got["thresholds"][0] == got["thresholds"][1]
    assert all(len(c[1]) == 1 for c in be.log if c[0] == "hist") and [c[0] for c in be.log].count("collect") == 1

    class Many(C.NumpyBackend):                         # a backend that collects all ranges in one pass is asked once
        def collect_many(self, ranges):
            self.calls = getattr(self, "calls", 0) + 1
            return [self.collect(r) for r in ranges]

    one, many = C.NumpyBackend(full, ps, gs, False), Many(full, ps, gs, False)
    a = allpairs.all_pairs_roc(probe, ps, gallery, gs, fars=FARS, collect_cap=64, backend=one)
    b = allpairs.all_pairs_roc(probe, ps, gallery, gs, fars=FARS, collect_cap=64, backend=many)
    n_collect = [c[0] for c in one.log].count("collect")
    assert many.calls == 1 and n_collect > 1 and b["passes"] == a["passes"] - n_collect + 1
    assert np.array_equal(a["thresholds"], b["thresholds"]) and np.array_equal(a["tar_count"], b["tar_count"])


def test_a_lying_backend_is_caught():
    probe, ps, gallery, gs, full = _case("real", 7, False)

    class Lying(C.NumpyBackend):
        def count(self, thresholds):
            gen, imp = super().count(thresholds)
            return gen, imp + 1

    with pytest.raises(RuntimeError, match="count pass"):
        allpairs.all_pairs_roc(probe, ps, gallery, gs, fars=(0.01,), backend=Lying(full, ps, gs, False))

    class Short(C.NumpyBackend):
        def hist(self, ranges, bits):
            out = super().hist(ranges, bits)
            out[0, out[0].argmax()] -= 1
            return out

    with pytest.raises(RuntimeError, match="histogram"):
        allpairs.all_pairs_roc(probe, ps, gallery, gs, fars=(0.01,), collect_cap=1, backend=Short(full, ps, gs, False))


def test_counts_at_caller_thresholds():
    probe, ps, gallery, gs, full = _case("integer", 8, False)
    thr = (-1e9, -3.0, 0.0, 2.5, 1e9)
    gen_m, imp_m = C.pair_masks(ps, gs, False)
    got = allpairs.all_pairs_counts(probe, ps, gallery, gs, thresholds=thr, backend=C.NumpyBackend(full, ps, gs, False))
    assert got["genuine_above"].tolist() == [int((full[gen_m] > t).sum()) for t in thr]
    assert got["impostor_above"].tolist() == [int((full[imp_m] > t).sum()) for t in thr]
    assert got["genuine_above"][0] == got["n_genuine"] and got["impostor_above"][-1] == 0
    none = allpairs.all_pairs_counts(probe, ps, gallery, gs, backend=C.NumpyBackend(full, ps, gs, False))
    assert none["genuine_above"].size == 0 and none["impostor_above"].dtype == np.int64


def test_subject_codes_and_pair_counts():
    ps, gs = np.array([40, 7, 7, 1000, -3]), np.array([7, 40, 40, 5, 7, 2 ** 40])
    pc, gc, n_gen, n_imp = allpairs.subject_codes(ps, gs)
    assert pc.dtype == gc.dtype == np.int32 and min(pc.min(), gc.min()) == 0 and max(pc.max(), gc.max()) == 5
    assert np.array_equal(pc[:, None] == gc[None, :], ps[:, None] == gs[None, :])
    assert n_gen == int((ps[:, None] == gs[None, :]).sum()) == 6 and n_imp == 30 - 6
    pc, gc, n_gen, n_imp = allpairs.subject_codes(torch.from_numpy(ps))
    assert gc is None and (n_gen, n_imp) == (1, 9)
    rng = np.random.default_rng(9)
    for sym in (False, True):
        a, b = rng.integers(0, 12, 70), rng.integers(3, 15, 90)
        gen_m, imp_m = C.pair_masks(a, b, sym)
        _, _, n_gen, n_imp = allpairs.subject_codes(a, None if sym else b)
        assert (n_gen, n_imp) == (int(gen_m.sum()), int(imp_m.sum()))
        assert isinstance(n_gen, int) and isinstance(n_imp, int)
    # counts beyond 2^32 stay exact: 100 000 rows of one subject against 100 000 rows of it and of another
    _, _, n_gen, n_imp = allpairs.subject_codes(np.zeros(100000, np.int64), np.r_[np.zeros(50000, np.int64), np.ones(50000, np.int64)])
    assert (n_gen, n_imp) == (5 * 10 ** 9, 5 * 10 ** 9)
    with pytest.raises(ValueError):
        allpairs.subject_codes(np.array([1.5, 2.0]))


def test_refusals_before_any_launch():
    probe, ps, gallery, gs, full = _case("real", 5, False)
    be = C.NumpyBackend(full, ps, gs, False)
    roc = allpairs.all_pairs_roc

    def bad(match, *args, **kw):
        kw.setdefault("backend", be)
        with pytest.raises(ValueError, match=match):
            roc(*args, **kw)
        assert not be.log                               # nothing ran

    nan = probe.copy()
    nan[3, 5] = np.nan
    bad("NaN or infinity", nan, ps, gallery, gs)
    inf = gallery.copy()
    inf[0, 0] = -np.inf
    bad("NaN or infinity", probe, ps, torch.from_numpy(inf), gs)
    bad("multiple of 4", probe[:, :6], ps, gallery[:, :6], gs)
    bad("channels", probe[:, :8], ps, gallery, gs)
    bad(r"\[rows\]\[E\]", probe[0], ps, gallery, gs)
    bad("fit int32", np.broadcast_to(np.zeros((1, 4), np.float32), (2 ** 31 - 1, 4)), ps, gallery[:, :4], gs)
    bad("one subject id per", probe, ps[:-1], gallery, gs)
    bad("one subject id per", probe, ps, gallery, np.r_[gs, 1])
    bad("come together", probe, ps, gallery, None)
    bad("come together", probe, ps, None, gs)
    bad("must be integers", probe, ps.astype(np.float64), gallery, gs)
    bad("needs both", probe, np.arange(len(ps)), gallery, np.arange(len(gs)) + 1000)      # no genuine pair
    bad("needs both", probe, np.zeros(len(ps), int), gallery, np.zeros(len(gs), int))      # no impostor pair
    bad("needs both", probe[:1], ps[:1])                                                   # symmetric, one row
    bad(r"outside \[0, 1\)", probe, ps, gallery, gs, fars=(0.5, 1.0))
    bad(r"outside \[0, 1\)", probe, ps, gallery, gs, fars=(-1e-9,))
    bad(r"outside \[0, 1\)", probe, ps, gallery, gs, fars=(float("nan"),))
    bad("at most 16", probe, ps, gallery, gs, fars=(0.1,) * 17)
    bad("dtype", probe, ps, gallery, gs, dtype=torch.bfloat16)
    bad("collect_cap", probe, ps, gallery, gs, collect_cap=0)
    with pytest.raises(ValueError, match="at most 16"):
        allpairs.all_pairs_counts(probe, ps, gallery, gs, thresholds=(0.1,) * 17, backend=be)
    with pytest.raises(ValueError, match="NaN"):
        allpairs.all_pairs_counts(probe, ps, gallery, gs, thresholds=(float("nan"),), backend=be)
    with pytest.raises(ValueError, match="dtype"):
        allpairs.all_pairs_counts(probe, ps, gallery, gs, thresholds=(0.1,), dtype=torch.float16, backend=be)
    assert not be.log
    # 16 targets are taken
    assert roc(probe, ps, gallery, gs, fars=tuple(np.linspace(0, 0.9, 16)), backend=be)["thresholds"].size == 16


def test_entries_declared_exported_and_validating():
    protos = _lib.parse_header()
    lib = _lib.load()
    for name in (ENTRY, "msml_allpairs_splits"):
        assert name in protos and hasattr(lib, name), name
    assert protos[ENTRY][1][-1][1] == "stream" and len(protos[ENTRY][1]) == 23
    src = open(_lib.HEADER).read()
    sect = src[src.index("all-pairs verification"):]
    assert "datasets/benchmarks/get_list.py:138-208" in sect
    for name, v in (("MSML_ALLPAIRS_HIST", allpairs.HIST), ("MSML_ALLPAIRS_COLLECT", allpairs.COLLECT),
                    ("MSML_ALLPAIRS_COUNT", allpairs.COUNT)):
        assert "%s = %d" % (name, v) in sect

    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    a += -a % 16
    one = (ctypes.c_ulonglong * 16)()
    zero = (ctypes.c_int * 16)()
    thr = (ctypes.c_double * 16)()
    F32, F64 = _lib.F32, _lib.F64

    def run(P=8, G=40, E=8, dtype=F64, sym=0, mode=allpairs.HIST, n_ranges=1, prefix=one, bits=zero, b=12, probe=a,
            pcode=a, gallery=a, gcode=a, hist=a, cand=a, cand_count=a, cap=8, thr=thr, n_thr=1, counts=a, splits=1):
        return lib.msml_allpairs_pass(probe, P, pcode, gallery, G, gcode, E, dtype, sym, mode, n_ranges, prefix, bits, b,
                                      hist, cand, cand_count, cap, thr, n_thr, counts, splits, None)

    err = lib.msml_last_error
    for mode in (allpairs.HIST, allpairs.COLLECT, allpairs.COUNT):
        assert run(mode=mode, E=6) == -1 and b"multiple of 4" in err()
        assert run(mode=mode, E=0) == -1 and run(mode=mode, P=0) == -1 and run(mode=mode, G=2 ** 31) == -1
        for null in ("probe", "gallery", "pcode", "gcode"):
            assert run(mode=mode, **{null: None}) == -1 and b"null pointer" in err(), null
        assert run(mode=mode, probe=a + 8) == -1 and b"aligned" in err()
        assert run(mode=mode, gcode=a + 2) == -1 and b"misaligned" in err()
        assert run(mode=mode, dtype=_lib.BF16) == -1 and b"dtype" in err()
        assert run(mode=mode, splits=0) == -1 and run(mode=mode, splits=65536) == -1
        assert run(mode=mode, sym=1) == -1 and run(mode=mode, sym=2, G=8) == -1        # symmetric needs G == P
    assert run(mode=3) == -1 and b"mode" in err()
    assert run(hist=None) == -1 and run(hist=a + 4) == -1 and run(prefix=None) == -1 and run(bits=None) == -1
    assert run(n_ranges=0) == -1 and run(n_ranges=17) == -1
    assert run(n_ranges=3) == -1 and b"exceed" in err()                                # 3 << 12 bins > 8192
    assert run(b=0) == -1 and run(b=14) == -1
    deep = (ctypes.c_int * 16)(60)
    assert run(bits=deep, b=12) == -1 and b"key bits" in err()                         # 60 + 12 > 64
    assert run(bits=(ctypes.c_int * 16)(24), b=12, dtype=F32) == -1                    # 24 + 12 > 32
    assert run(bits=(ctypes.c_int * 16)(-1)) == -1
    assert run(bits=(ctypes.c_int * 16)(4), prefix=(ctypes.c_ulonglong * 16)(16)) == -1 and b"does not fit" in err()
    assert run(mode=allpairs.COLLECT, n_ranges=17) == -1 and run(mode=allpairs.COLLECT, n_ranges=0) == -1
    assert run(mode=allpairs.COLLECT, cand=None) == -1 and run(mode=allpairs.COLLECT, cand_count=None) == -1
    assert run(mode=allpairs.COLLECT, cap=0) == -1 and run(mode=allpairs.COLLECT, cand_count=a + 4) == -1
    assert run(mode=allpairs.COUNT, n_thr=17) == -1 and b"thresholds" in err()
    assert run(mode=allpairs.COUNT, n_thr=0) == -1 and run(mode=allpairs.COUNT, thr=None) == -1
    assert run(mode=allpairs.COUNT, counts=None) == -1 and run(mode=allpairs.COUNT, counts=a + 4) == -1
    assert run(mode=allpairs.COUNT, thr=(ctypes.c_double * 16)(float("nan"))) == -1 and b"NaN" in err()
    # the default split count follows the search's
    assert lib.msml_allpairs_splits(3530, 1000000) == lib.msml_search_topk_splits(3530, 1000000, 10)
    assert lib.msml_allpairs_splits(1, 1) == 1 and lib.msml_allpairs_splits(0, 10) == 0
    assert lib.msml_allpairs_splits(10, 2 ** 31) == 0


def test_both_call_routes_reach_the_new_entries():
    import __graft_entry__ as ge
    assert ge.build_fastabi()
    fa = _lib._fastabi()
    assert fa, "msml_amd/_msml_fastabi.so did not load"
    lib = _lib.load()
    assert fa.msml_allpairs_splits(3530, 1000000) == lib.msml_allpairs_splits(3530, 1000000) >= 1
    args = (None, 1, None, None, 1, None, 4, _lib.F64, 0, 0, 1, None, None, 12, None, None, None, 0, None, 0, None, 1)
    assert fa.msml_allpairs_pass(*args, None) == -1
    assert _lib.call_status(ENTRY, *args, None) == -1 and b"null pointer" in lib.msml_last_error()


def test_real_valued_gpu_cases_keep_their_margin():
    """The GPU test compares counts exactly on these cases; that needs every other reference score further from a
    threshold than the f64 error of a dot product (6e-14 at E = 512 on unit rows)."""
    for cfg in C.REAL_CONFIGS:
        x, ids = C.make_verification(**cfg)
        for sym in (False, True):
            probe, ps, gallery, gs = (x, ids, x, ids) if sym else C.split_rows(x, ids)
            full = probe @ gallery.T
            want = C.allpairs_ref(full, ps, gs, C.REAL_FARS, sym)
            margin = C.threshold_margin(full, ps, gs, want["thresholds"], sym)
            print(cfg["seed"], "sym" if sym else "asym", full.shape, "margin %.2e" % margin, want["tar"])
            assert margin > 1e-9 and 0 < want["tar"][1] <= want["tar"][3] < 1
