"""GPU tests of the all-pairs verification path (msml_amd/allpairs.py, csrc/allpairs.hip) against the full-matrix
numpy restatement of tests/allpairs_cases.py.

Bounds.  Integer rows give exact scores in f32 and f64 (every partial sum is an integer below 2^24), so thresholds and
counts are compared exactly.  Real-valued unit rows in f64: a dot product over E <= 512 channels is off by at most
E * 2^-53 * |p| |g|, about 6e-14, doubled for the restatement's own rounding: |tau - tau_ref| <= 1e-12; the counts are
exact as long as no other reference score lies that close to a threshold, which each test asserts on its own data (the
margins are 2e-6 and more).  There is no real-valued exactness test in f32: its rounding is of the size of the gaps."""
import functools

import numpy as np
import pytest
import torch

from tests import allpairs_cases as C

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
DT_IDS = ["f64", "f32"]
INT_CASES = [(p, g, e, False) for p, g, e in C.INT_SHAPES] + [(130, 130, 128, True)]
INT_IDS = ["%dx%dx%d%s" % (p, g, e, "_sym" if s else "") for p, g, e, s in INT_CASES]


@functools.lru_cache(maxsize=None)
def _int_case(n):
    """(probe, ps, gallery or None, gs or None, full, reference) of integer case n, computed once."""
    p, g, e, sym = INT_CASES[n]
    probe, ps, gallery, gs = C.integer_case(40 + n, p, g, e)
    if sym:
        gallery, gs = None, None
    full = probe @ (probe if sym else gallery).T
    return probe, ps, gallery, gs, full, C.allpairs_ref(full, ps, gs, C.INT_FARS, sym)


@functools.lru_cache(maxsize=None)
def _real_case(n, sym):
    x, ids = C.make_verification(**C.REAL_CONFIGS[n])
    probe, ps, gallery, gs = (x, ids, None, None) if sym else C.split_rows(x, ids)
    full = probe @ (probe if sym else gallery).T
    return probe, ps, gallery, gs, full, C.allpairs_ref(full, ps, gs, C.REAL_FARS, sym)


def _roc(probe, ps, gallery, gs, **kw):
    from msml_amd import allpairs
    return allpairs.all_pairs_roc(probe, ps, gallery, gs, **kw)


def _same(got, want, tol=0.0):
    assert (got["n_genuine"], got["n_impostor"]) == (want["n_genuine"], want["n_impostor"])
    for key in ("far_count", "tar_count", "far_achieved", "tar"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    assert got["thresholds"].dtype == np.float64 and got["far_count"].dtype == np.int64
    err = float(np.abs(got["thresholds"] - want["thresholds"]).max())
    assert err <= tol, err


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", range(len(INT_CASES)), ids=INT_IDS)
def test_integer_rows_equal_the_restatement_exactly(n, dtype):
    """Edge shapes: one row, one short of a tile, one past it, P != G (70 x 75 tells the two C/D lane maps apart: a
    transposed or mis-rowed read pairs the wrong subject codes), several tiles with E = 512; the diagonal in the
    symmetric case.  Many ties, at the thresholds too."""
    probe, ps, gallery, gs, full, want = _int_case(n)
    got = _roc(probe, ps, gallery, gs, fars=C.INT_FARS, dtype=dtype, collect_cap=16)
    print(INT_IDS[n], "thresholds", got["thresholds"], "far", got["far_count"], "tar", got["tar_count"], "passes", got["passes"])
    _same(got, want)
    assert (got["far_count"] <= np.floor(np.array(C.INT_FARS) * got["n_impostor"])).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [3, 5], ids=["70x75", "130_sym"])
def test_same_result_for_every_cap_split_and_run(n, dtype):
    probe, ps, gallery, gs, full, want = _int_case(n)
    dev = [torch.from_numpy(probe).cuda(), ps, None if gallery is None else torch.from_numpy(gallery).cuda(), gs]
    passes = {}
    for cap in (1, 64, 1 << 20):
        for splits in (1, 3, 7, None):
            for run in range(2 if splits is None else 1):
                got = _roc(*dev, fars=C.INT_FARS, dtype=dtype, collect_cap=cap, splits=splits)
                _same(got, want)
                assert passes.setdefault(cap, got["passes"]) == got["passes"]
    print("passes by cap", passes)
    width = 32 if dtype == torch.float32 else 64
    assert passes[1 << 20] == 2 < passes[64]                       # collect + count; then the levels come in
    assert passes[1] >= (width + 11) // 12 + 1                     # tied scores: every level down to single keys ran


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_threshold_has_the_bits_of_search_topk(dtype):
    """f = 0: tau is the largest impostor score, and so is the best subject-mismatched entry of the top-k lists (every
    probe has at most 3 genuine rows, k = 32).  Real-valued rows: the two kernels must round alike."""
    from msml_amd import identify
    probe, ps, gallery, gs, full, _ = _real_case(0, False)
    assert (ps[:, None] == gs[None, :]).sum(1).max() < 32
    s, i = identify.search_topk(probe, gallery, k=32, dtype=dtype)
    s, i = s.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    best = np.where(gs[i] != ps[:, None], s, -np.inf).max()
    for splits in (1, 5):
        got = _roc(probe, ps, gallery, gs, fars=(0.0,), dtype=dtype, splits=splits, collect_cap=1)
        tau = got["thresholds"].astype(s.dtype)
        assert tau.astype(np.float64)[0] == got["thresholds"][0]   # exactly the score widened
        assert tau.tobytes() == np.array([best], s.dtype).tobytes(), (tau, best)
        assert got["far_count"][0] == 0


@pytest.mark.parametrize("sym", [False, True], ids=["asym", "sym"])
@pytest.mark.parametrize("n", [0, 1], ids=["seed11_e128", "seed12_e512"])
def test_real_valued_rows_f64(n, sym):
    probe, ps, gallery, gs, full, want = _real_case(n, sym)
    assert full.shape == [(94, 142), (236, 236), (50, 75), (125, 125)][2 * n + sym]
    margin = C.threshold_margin(full, ps, gs, want["thresholds"], sym)
    assert margin > 1e-9, margin                                   # no other score near a threshold: counts are decided
    passes = []
    for cap in (1 << 20, 64, 1):
        got = _roc(probe, ps, gallery, gs, fars=C.REAL_FARS, collect_cap=cap)
        err = float(np.abs(got["thresholds"] - want["thresholds"]).max())
        print("seed %d %s cap %d: max |tau - tau_ref| %.3e (bound 1e-12), margin %.2e, passes %d, tar %s"
              % (C.REAL_CONFIGS[n]["seed"], "sym" if sym else "asym", cap, err, margin, got["passes"], got["tar"]))
        _same(got, want, 1e-12)
        passes.append(got["passes"])
    assert passes[0] == 2 < passes[1] < passes[2], passes          # the smaller the cap, the deeper the walk


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_counts_at_caller_thresholds(dtype):
    from msml_amd import allpairs
    for n in (4, 5):
        probe, ps, gallery, gs, full, _ = _int_case(n)
        gen_m, imp_m = C.pair_masks(ps, gs, gallery is None)
        thr = (-1e9, -40.5, -1.0, 0.0, 0.5, 33.0, 1e9) + tuple(range(100, 109)) if n == 4 else (-1e9, 0.0, 12.0)
        got = allpairs.all_pairs_counts(probe, ps, gallery, gs, thresholds=thr, dtype=dtype, splits=2)
        assert got["genuine_above"].tolist() == [int((full[gen_m] > t).sum()) for t in thr]
        assert got["impostor_above"].tolist() == [int((full[imp_m] > t).sum()) for t in thr]
        assert got["genuine_above"][0] == got["n_genuine"] and got["impostor_above"][0] == got["n_impostor"]
        assert 0 < got["impostor_above"][3 if n == 4 else 1] < got["n_impostor"]


def test_histogram_flushes_inside_a_long_split():
    """A workgroup adds into u32 bins in LDS and flushes them into the u64 table every 2^19 column tiles, before a bin
    could overflow.  That takes a split of more than 2^19 tiles to reach: one probe row against 2^25 + 70 short gallery
    rows in ONE split, compared with the default split count and with the bins numpy makes of the same scores."""
    from msml_amd import allpairs
    G = (1 << 19) * 64 + 70
    gen = torch.Generator(device="cuda").manual_seed(3)
    g = torch.randint(-4, 5, (G, 4), device="cuda", generator=gen).to(torch.float32)
    gcode = torch.randint(0, 3, (G,), device="cuda", generator=gen).to(torch.int32)
    p = torch.tensor([[1.0, 2.0, -1.0, 3.0]], device="cuda")
    pcode = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = allpairs.HipBackend(p, pcode, g, gcode, torch.float32, splits=1).hist([(0, 0)], 12)
    many = allpairs.HipBackend(p, pcode, g, gcode, torch.float32).hist([(0, 0)], 12)
    scores = (g * p[0]).sum(1)                                     # exact on integers; element-wise, no BLAS call
    keys = C.key32(scores.cpu().numpy())[(gcode != 0).cpu().numpy()]
    want = np.bincount((keys >> np.uint32(20)).astype(np.int64), minlength=4096)
    assert np.array_equal(one[0], want) and np.array_equal(many[0], want)
    assert int(want.sum()) == keys.size > 1 << 24 and (want > 0).sum() > 20


def test_entry_point_refusals_are_status_returns():
    from msml_amd import _lib, allpairs
    x = torch.zeros(64, 8, dtype=torch.float64, device="cuda")
    code = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(4096 + 8, dtype=torch.int64, device="cuda")
    prefix, bits, thr = np.zeros(16, np.uint64), np.zeros(16, np.int32), np.zeros(17, np.float64)

    def run(probe=x, pcode=code, gallery=x, gcode=code, E=8, dtype=_lib.F64, mode=allpairs.HIST, hist=out, n_thr=1,
            counts=out):
        return _lib.call_status("msml_allpairs_pass", probe, 64, pcode, gallery, 64, gcode, E, dtype, 0, mode, 1,
                                prefix.ctypes.data, bits.ctypes.data, 12, hist, out, out, 8, thr.ctypes.data, n_thr,
                                counts, 1)

    for null in ("probe", "pcode", "gallery", "gcode", "hist"):
        assert run(**{null: None}) == -1, null
    assert run(mode=allpairs.COUNT, counts=None) == -1
    assert run(probe=x.data_ptr() + 8) == -1 and run(gcode=code.data_ptr() + 2) == -1
    assert run(hist=out.data_ptr() + 4) == -1
    assert run(dtype=_lib.BF16) == -1 and run(E=6) == -1
    assert run(mode=allpairs.COUNT, n_thr=17) == -1
    assert b"thresholds" in _lib.load().msml_last_error()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                      # nothing was launched
    assert run() == 0 and run(mode=allpairs.COUNT) == 0             # the same arguments, valid: accepted
    torch.cuda.synchronize()
