"""tests/conv_cases.py on the CPU: the float64 restatement of the conv formula is torch's (F.conv2d / F.conv_transpose2d in
float64, the only place torch's conv is trusted) at every case shape; every case takes the route its table entry names
(the dispatch conditions restated in Python against msml_conv2d_kernel and the *_applies queries, host functions); every
exactness condition of the integer data holds for every case, so that the f64 result rounded once passes both checks;
every mutant fails the check named for it; and the gap the older tests leave is recorded.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from msml_amd import _lib
from tests import conv_cases as C

CASES = C.cases()
SHAPES = {}
for _c in CASES:
    SHAPES.setdefault((C._xin(_c) is not None,) + tuple(_c[5:22]), _c)


# ------------------------------------------------------------------------------------------- the case table
def test_every_case_takes_the_route_of_its_table_entry():
    assert 70 <= len(CASES)
    for c in CASES:
        inst, _ = C.route(c)
        assert inst == c.inst, (c.name, inst)
        if c.entry != "deconv4_bwd_data":
            assert C.kernel_name(c).startswith(c.kernel), (c.name, C.kernel_name(c))
        assert c.c0 <= c.c0p and c.c1 <= c.c1p and c.cout <= c.coutp and c.N * c.P * c.Q < 2 ** 24
        assert c.statdef in ("f32", "stored")
        with C.switched(c):
            if c.entry == "bnin":
                assert _lib.value("msml_conv2d_bnin_applies", c.c0p, c.coutp, c.N, c.H, c.W, c.P, c.Q, c.R, c.S, c.stride, c.ph,
                                  c.pw, int(c.stats is not None)) == 1, c.name
            if c.entry == "bnin_acc":
                assert _lib.value("msml_conv2d_bnin_acc_applies", c.c0p, c.coutp, c.N, c.H, c.W, c.P, c.Q, c.R, c.S, c.stride,
                                  c.ph, c.pw) == (3 if c.inst.startswith("k_conv_halo_p") else 1), c.name
        # tensors of the largest case stay under about 40 MB
        assert max(c.N * c.H * c.W * max(c.c0p, c.c1p), c.N * c.P * c.Q * c.coutp) * 2 <= 40e6, c.name
    for c in C.REFUSED:
        assert C.route(c)[0] == C.UNSUPPORTED, c.name
    r = {c.name: c for c in C.REFUSED}
    q = r["refused_bnin_9x13"]
    assert _lib.value("msml_conv2d_bnin_applies", q.c0p, q.coutp, q.N, q.H, q.W, q.P, q.Q, 3, 3, 1, 1, 1, 0) == 0
    q = r["refused_bnin_64"]
    assert _lib.value("msml_conv2d_bnin_applies", q.c0p, q.coutp, q.N, q.H, q.W, q.P, q.Q, 3, 3, 1, 1, 1, 1) == 0
    q = r["refused_bnin_acc_9x13"]
    assert _lib.value("msml_conv2d_bnin_acc_applies", q.c0p, q.coutp, q.N, q.H, q.W, q.P, q.Q, 3, 3, 1, 1, 1) == 0


def test_the_case_list_sits_on_the_thresholds_of_the_dispatch_source():
    by = {c.name: c for c in CASES}
    tiles = lambda c, gh, gw: c.N * C.cdiv(gh, 14) * C.cdiv(gw, 14)
    assert _lib.value("msml_conv_tile_m", 64) == C.tile_m(64) == 256 and _lib.value("msml_conv_tile_m", 128) == C.tile_m(128) == 128
    assert [_lib.value("msml_conv_tile_n", n) for n in (32, 64, 128, 384)] == [C.tile_n(n) for n in (32, 64, 128, 384)]
    # persistent loops: more tiles than workgroups
    assert tiles(by["ws_n17_56_plain"], 56, 56) == 272 > C.CUS
    assert tiles(by["s2r_fwd_n65_56_acc"], 28, 28) == 260 and tiles(by["s2r_bwd_n65_28"], 28, 28) == 260
    assert tiles(by["halop_n515_acc"], 14, 14) == 515 >= 2 * C.CUS and 515 % C.CUS == 3
    c = by["halop_n90_27x40_acc"]
    assert tiles(c, 27, 40) == 540 and c.H % 14 and c.W % 14
    assert not C.halo_persist_shape(c._replace(N=85))                    # 510 tiles: one round short
    # the 70 % rule, both sides
    assert C._real70(2, 13, 27) and not C._real70(1, 9, 13) and not C._real70(42, 7, 7)
    # row-mode statistics need as many rows as workgroups (conv_ws.hip:471, conv_halo.hip:976)
    assert not C.ws_applies(by["ws_n2_13x27_rows"], True) and C.ws_applies(by["ws_n2_13x27_rows"], False)
    assert C.ws_applies(by["ws_n1_28_rows"], True) and C.ws_applies(by["ws_n3_14_rows_bias"], True)
    assert C.halo_applies(by["halo_b_rows"], True) and C.cdiv(2 * 13 * 27, 128) == 6 > tiles(by["halo_b_rows"], 13, 27) == 4
    # k_conv_r32 (conv_r32.hip:266-283): strips of 7 rows, 2060 units, the grid capped at 2 * 256
    c, rs = by["r32_n1030_8_plain"], 14
    while rs > 4 and c.N * C.cdiv(c.H, rs) < 8 * C.CUS:
        rs = (rs + 1) // 2
    assert rs == 7 and c.N * C.cdiv(c.H, rs) == 2060 and (2060 + 3) // 4 > 2 * C.CUS
    c = by["r32_n1_60x62_plain"]
    assert 2304 + 4 * (3 * (c.W + 2) * 64 + c.W * 64) + 1024 > 64 * 1024
    assert by["r32_n2_9x63_plain"].W == 63 and by["r32_n1_2x8_plain"].W == 8 and by["r32_n1_2x8_plain"].H == 2
    # k_conv_pw (conv_pw.hip:303-319): the first M whose units exceed cus * pw_wgs_per_cu workers
    need = lambda m: C.cdiv(C.cdiv(C.cdiv(m, 32), 2), 4)
    assert _lib.get_option("MSML_PW_WGS_PER_CU") == 4
    assert need(262144) == 1024 and need(262145) == 1025 > 4 * C.CUS
    c = by["pw_64x64_n1_512x513"]
    assert need(c.N * c.H * c.W) == 1026
    assert {(c.c0p, c.coutp) for c in CASES if c.inst.startswith("k_conv_pw")} == {(32, 64), (64, 32), (64, 64), (64, 128), (128, 64)}
    assert {c.inst.split(", ")[2] for c in CASES if c.inst.startswith("k_conv_pw")} == {"PLAIN", "ADD", "STATS", "BNB"}
    assert all((c.N * c.H * c.W) % 32 == 105 % 32 for c in CASES if c.family == "pw" and c.H == 7)
    # k_conv_halo2: the first N that passes fill7 / fill4, with a partly filled last mosaic
    c = by["h2_m7_n318_plain"]
    assert C.halo2_tiling(c) == 2 and C.halo2_tiling(c._replace(N=316)) == 0 and c.N % 4 == 2
    assert C.halo2_tiling(by["h2_m7_n317_plain"]) == 2 and 317 % 4 == 1
    c = by["h2_m7_n158_bwd"]
    assert C.halo2_tiling(c) == 2 and C.halo2_tiling(c._replace(N=156)) == 0 and c.N % 4 == 2
    c = by["h2_m4_n236_plain"]
    assert C.halo2_tiling(c) == 3 and C.halo2_tiling(c._replace(N=234)) == 0 and c.N % 6 == 2
    assert C.halo2_tiling(by["fast_7x7_n5_256"]) == 0 and C.halo2_tiling(by["fast_4x4_n7_512"]) == 0
    # k_conv_line: 224 / H lines per tile; H = 28: a partial last tile; grids of 2 and 1 workgroups per CU
    assert C.cdiv(28, 224 // 28) == 4 and 28 % (224 // 28) == 4
    assert by["line_32x32_1x7_n130_28"].N * 4 == 520 > 2 * C.CUS and 7 * 32 * 32 * 2 + 2 * 288 * 32 * 2 <= 76 * 1024
    assert by["line_64x32_7x1_n65_28"].N * 4 == 260 > C.CUS and 7 * 32 * 64 * 2 + 2 * 288 * 64 * 2 > 76 * 1024
    assert {(c.c0p, c.coutp, c.R, c.H) for c in CASES if c.family == "line" and c.N == 1} == \
        {(a, b, r, h) for (a, b) in ((64, 32), (32, 32), (32, 64)) for r in (7, 1) for h in (28, 56)}
    # k_conv_fast: the small-M tile from M = 2048 on under conv_small_m_wgs = 200, the big tile off by default
    assert _lib.get_option("MSML_CONV_SMALL_M_WGS") == 200 and _lib.get_option("MSML_CONV_BIG_TILE") == 0
    c = by["fast_small_n128_512_4"]
    assert c.N * c.P * c.Q == 2048 and C.route(c._replace(N=127))[0] == "k_conv_fast<bf16, 128 x 128>"
    assert by["fast_n41_64_7_rows"].N * 49 < 2048 <= by["fast_small_n42_64_7_acc"].N * 49
    assert (by["fast_2seg_n2_64+18_9"].c0p // 32 * 9) % 2 == 0
    assert {c.stride for c in CASES if c.family in ("fast", "igemm")} == {1, 2, 4}
    assert {c.dtype for c in CASES if c.family == "igemm"} == {C.FF, C.BF, C.BB}
    assert {c.c0p for c in CASES if c.family == "igemm"} >= {8, 24}
    # every mutant names a case of the list
    for m, (name, checks) in C.MUTANTS.items():
        assert name in by and checks, m
    assert len(C.MUTANTS) >= 12


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", list(SHAPES.values()), ids=C.case_id)
def test_restatement_is_torchs_conv(case):
    c = case
    d, acc, mag = C.reference(c, "random")
    xs, w = C.operands(c, d)
    x = torch.cat(xs, 3).permute(0, 3, 1, 2).contiguous()
    if c.tr:
        op = (c.P - ((c.H - 1) * c.stride - 2 * c.ph + c.R), c.Q - ((c.W - 1) * c.stride - 2 * c.pw + c.S))
        want = F.conv_transpose2d(x, w.permute(1, 0, 2, 3).contiguous(), None, c.stride, (c.ph, c.pw), op)
    else:
        want = F.conv2d(x, w, None, c.stride, (c.ph, c.pw))
    want = want.permute(0, 2, 3, 1)
    assert want.shape == acc.shape == (c.N, c.P, c.Q, c.cout)
    assert bool((acc - want).abs().le(1e-13 * mag + 1e-300).all()), float((acc - want).abs().max())
    assert bool((mag >= acc.abs()).all())
    C.forget()


# ------------------------------------------------------------------------------------------- the exactness conditions
def _dyadic_sum_is_exact(t, what, name):
    """sum |t| over the pixels, in units of the quantum of t, stays below 2^24: every f32 partial sum of every order is exact."""
    q = C.quantum(t)
    assert float(t.abs().sum(0).max()) / q < 2.0 ** 24, (name, what, float(t.abs().sum(0).max()) / q)


@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_exact_data_meets_every_condition_and_the_f64_result_passes_both_checks(case):
    c = case
    want = C.expect(c, "exact")
    d, acc, mag = C.reference(c, "exact")
    xs, w = C.operands(c, d)
    # 1. every reduction is exact: integers, sum |x w| <= 256, the weights cover every position and every tap
    assert float(mag.max()) <= 256, float(mag.max())
    assert all(torch.equal(x, x.round()) for x in xs) and torch.equal(w, w.round()) and float(w.abs().max()) == 1
    assert max(float(x.abs().max()) for x in xs) <= C.xmax(c)
    nz = w != 0
    assert int(nz.reshape(c.cout, -1).sum(1).max()) <= C.nnz_per_row(c) <= max(85, 256 // C.xmax(c))
    assert bool(nz.any(0).all()), "a (c, r, s) position is zero in every reduction row"
    assert bool(nz.any(1).all()), "a reduction row misses a tap"
    assert torch.equal(acc, acc.round()) and torch.equal(acc.float().bfloat16().double(), acc)
    # 2. pad channels: the inputs' hold 7, the output's must come out 0
    for k, cr in (("x0", c.c0), ("x1", c.c1)):
        if d[k] is not None and d[k].shape[3] > cr:
            assert bool((d[k][..., cr:] == C.PAD).all())
    assert bool((want["out"][..., c.cout:] == 0).all())
    assert not bool(torch.isnan(want["out"].float()).any())
    # 4. the value before the last rounding has at most 24 significant bits (exact in f32 whatever the grouping)
    assert torch.equal(want["final"].float().double(), want["final"])
    # 3. statistics and bnbwd sums are exact in every order
    if c.stats:
        e = C.epilogue(c, d, acc, mag)
        v = e["pre"].reshape(-1, c.coutp)
        _dyadic_sum_is_exact(v, "sum", c.name)
        _dyadic_sum_is_exact(v * v, "sum of squares", c.name)
        assert torch.equal(want["stats"].float().double(), want["stats"])
    if C._bnb(c):
        for k in ("bn_scale", "bn_invstd") + (("bn_alpha",) if c.alpha else ()):
            m, _ = torch.frexp(d[k][:c.cout].abs())
            assert bool((m == 0.5).all()), k                         # powers of two
        assert torch.equal(d["bn_mean"], d["bn_mean"].round()) and torch.equal(d["bn_shift"], d["bn_shift"].round())
        dy, x = want["out"].double().reshape(-1, c.coutp), d["bn_x"].double().reshape(-1, c.coutp)
        z = x * d["bn_scale"].double() + d["bn_shift"].double()
        al = d["bn_alpha"].double() if c.alpha else torch.ones(c.coutp, dtype=torch.float64)
        g = torch.where(z <= 0, dy * al, dy)
        xh = (x - d["bn_mean"].double()) * d["bn_invstd"].double()
        for what, t in (("g", g[:, :c.cout]), ("g * xhat", (g * xh)[:, :c.cout]), ("dy * min(z, 0)", (dy * z.clamp(max=0))[:, :c.cout])):
            _dyadic_sum_is_exact(t, what, c.name)
        assert torch.equal(want["bnb"].float().double(), want["bnb"]) and bool((want["bnb"][:, c.cout:] == 0).all())
    if C._xin(c):
        m, _ = torch.frexp(d["in_scale"][:c.c0].abs())
        assert bool((m == 0.5).all()) and torch.equal(d["in_shift"], d["in_shift"].round())
        x = d["x0"].double() * d["in_scale"].double() + d["in_shift"].double()
        if c.alpha:
            x = torch.where(x < 0, x * d["in_alpha"].double(), x)
        assert torch.equal(x[..., :c.c0], xs[0])                     # no rounding anywhere in the input BatchNorm
    if c.entry == "bnin_acc":
        acc_in, count, gamma, beta = C.bnin_acc_operands(c, d, "exact")
        s, ss = acc_in.sum(0)
        mean = s / count
        invstd = (1.0 / torch.sqrt(ss / count - mean * mean + float(torch.tensor(C.EPS, dtype=torch.float32)))).float()
        assert bool((invstd == 2.0).all()) and torch.equal(mean, mean.round())
        scale = gamma * invstd
        assert torch.equal(scale, d["in_scale"]) and torch.equal(beta - mean.float() * scale, d["in_shift"])
    # the float64 result, rounded once, passes the exact check ...
    got = dict(out=C.stored(c, want["final"]), stats=want.get("stats"), bnb=want.get("bnb"))
    if c.stats:
        got["stats"] = want["stats"].float().double()
    if C._bnb(c):
        got["bnb"] = want["bnb"].float().double()
    assert C.exact_failures(c, want, got) == []
    # ... and, on random data, the budget check
    want = C.expect(c, "random")
    got = dict(out=C.stored(c, want["final"]))
    if c.stats:
        got["stats"] = want["stats"].float().double()
    if C._bnb(c):
        got["bnb"] = C.bnb_sums(c, want["d"], got["out"])[0].float().double()
    ratios = C.budget_ratios(c, want, got)
    assert max(ratios.values()) <= 1.0, ratios
    C.forget()


# ------------------------------------------------------------------------------------------- the mutants
@pytest.mark.parametrize("mutant", sorted(C.MUTANTS))
def test_each_mutant_fails_its_check(mutant):
    name, checks = C.MUTANTS[mutant]
    c = C.find(name)
    for kind in ("exact", "random"):
        want = C.expect(c, kind)
        got = C.expect(c, kind, mutant=mutant)
        if kind == "exact" and "exact" in checks:
            bad = C.exact_failures(c, want, got)
            assert bad, mutant
            print("%s on %s, exact data: %s" % (mutant, name, "; ".join(bad)))
        if kind == "random" and "budget" in checks:
            ratios = C.budget_ratios(c, want, got)
            print("%s on %s, random data: worst error / budget %s" % (mutant, name, ratios))
            assert max(ratios.values()) > 1.0, (mutant, ratios)
    C.forget()


def test_two_mutants_that_integer_data_cannot_see():
    """An integer accumulator of at most 256 IS a bf16 value, and integer statistics of stored integers are the statistics of
    the f32 values: rounding the accumulator to bf16 and taking the statistics from the stored tensor change no bit of the
    exact data -- and with scale and alpha powers of two a rounding in front of them commutes with them.  Both
    mutants are caught by the budget on random data (C.MUTANTS)."""
    for mutant in ("accumulator_rounded_to_bf16", "statistics_other_definition"):
        c = C.find(C.MUTANTS[mutant][0])
        assert C.MUTANTS[mutant][1] == ("budget",)
        assert C.exact_failures(c, C.expect(c, "exact"), C.expect(c, "exact", mutant=mutant)) == []
    C.forget()


def test_the_gap_the_old_bound_leaves():
    """128 -> 128 @ 14 x 14, N = 1, random data: a kernel that loses ONE product of one output element, and one that rounds its
    accumulator to bf16 before the bias, stay inside 1.5e-2 * max|ref|, the bound of tests/test_gpu_conv.py; both lie outside
    the derived budget, and the lost product changes a stored bit of the exact data."""
    for mutant in ("one_product_lost", "accumulator_rounded_to_bf16"):
        c = C.find(C.MUTANTS[mutant][0])
        want, got = C.expect(c, "random"), C.expect(c, "random", mutant=mutant)
        err = float((got["out"].double() - want["final"]).abs().max())
        old = 1.5e-2 * float(want["final"].abs().max())
        ratio = C.budget_ratios(c, want, got)["out"]
        print("%s on %s: max error %.4f, old bound %.4f, worst error / budget %.1f" % (mutant, c.name, err, old, ratio))
        assert 0 < err <= old and ratio > 1.0, (mutant, err, old, ratio)
    c = C.find("halo_a_plain")
    assert C.exact_failures(c, C.expect(c, "exact"), C.expect(c, "exact", mutant="one_product_lost"))
    C.forget()


# ------------------------------------------------------------------------------------------- the refusals
def test_the_refusals_need_no_gpu():
    """Each entry point returns MSML_ERR_UNSUPPORTED before any launch: reached with the address of a host buffer, which a
    refusing call never dereferences."""
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    used = ctypes.c_int(-7)
    for c in C.REFUSED:
        shape = (c.N, c.H, c.W, c.P, c.Q, c.R, c.S, c.stride, c.ph, c.pw)
        if c.entry == "bnin":
            rc = lib.msml_conv2d_bnin(p, c.c0p, p, p, None, p, C.kop(c), p, c.coutp, p if c.stats else None, *shape, None)
        elif c.entry == "bnin_acc":
            rc = lib.msml_conv2d_bnin_acc(p, c.c0p, p, 1.0, p, p, None, None, 0.1, 1e-5, p, None, p, p, C.kop(c), p, c.coutp, p,
                                          *shape, None)
        else:
            rc = lib.msml_conv2d_bnbwd(p, c.c0p, p, C.kop(c), p, c.coutp, *shape, c.tr, p, p, p, None, p, p, p, 1 << 30,
                                       ctypes.byref(used), None)
            assert used.value == -7
        assert rc == _lib.UNSUPPORTED, (c.name, rc, lib.msml_last_error())
