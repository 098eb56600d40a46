"""tests/stem_bwd_cases.py on the CPU: the float64 restatement of the stems' backward-data is the input gradient of
torch's conv on every case, and each mutant (a tap transposed, stride-2 parity off by one, a pad channel of dy read, the
last row band dropped) fails the checks the kernel has to pass -- exact equality on integer data, the derived budget on
random data.  No GPU (the band query is a host function of the library)."""
import numpy as np
import pytest
import torch

from tests import stem_bwd_cases as S

CASES = S.cases()
DTYPES = (torch.bfloat16, torch.float32)


def test_case_list_reaches_every_branch():
    assert {c.N for c in CASES} == {1, 3}
    assert {(c.C, c.R, c.stride) for c in CASES} >= {(3, 3, 1), (3, 3, 2), (1, 3, 2), (1, 5, 1)}
    assert {(c.Cout, c.ldy) for c in CASES} == {(32, 32), (64, 64), (96, 128)}
    assert max(c.W for c in CASES) == 128
    assert any(c.H == S.band(c) + 1 for c in CASES), "no case with a second row band of one row"
    for key in ((3, 1), (3, 2), (5, 1)):                 # (R, stride): three bands or more, the last one partial
        assert any((c.R, c.stride) == key and c.H > 2 * S.band(c) and c.H % S.band(c) for c in CASES), key
    # a wave with a second tile (the prefetch): more than 8 tiles of 32 pixels in one band's output rows
    assert any((min(c.H, S.band(c)) + c.R - 1) // c.stride * S.out_size(c.W, c.R, c.stride) > 8 * 32 for c in CASES)
    s2 = [c for c in CASES if c.stride == 2]
    assert {c.H % 2 for c in s2} == {0, 1} and {c.W % 2 for c in s2} == {0, 1}
    for m in S.MUTANTS:
        assert any(S.applies(m, c) for c in CASES), m


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_restatement_is_the_conv_input_gradient(case):
    for dt in DTYPES:
        dy, w = S.operands(*S.random_data(case, dt))
        got = S.adjoint_f64(dy, w, case)
        g = torch.from_numpy(dy[..., :case.Cout]).permute(0, 3, 1, 2).contiguous()
        want = torch.nn.grad.conv2d_input((case.N, case.C, case.H, case.W), torch.from_numpy(w), g, stride=case.stride,
                                          padding=case.R // 2).numpy()
        mag = S.adjoint_f64(dy, w, case, absolute=True)
        assert got.shape == want.shape
        assert np.all(np.abs(got - want) <= 1e-13 * mag + 1e-300), float(np.abs(got - want).max())
        assert np.all(mag >= np.abs(got))


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_each_mutant_fails(mutant):
    n = 0
    for case in CASES:
        if not S.applies(mutant, case):
            continue
        for dt in DTYPES:
            dy, w = S.operands(*S.exact_data(case, dt))
            assert not np.array_equal(S.adjoint_f64(dy, w, case, mutant), S.adjoint_f64(dy, w, case)), (mutant, case, "exact")
            dy, w = S.operands(*S.random_data(case, dt))
            want, mag = S.adjoint_f64(dy, w, case), S.adjoint_f64(dy, w, case, absolute=True)
            got = S.adjoint_f64(dy, w, case, mutant).astype(np.float32)       # what a kernel would store
            assert S.worst_ratio(got, want, mag, case) > 1.0, (mutant, case, "random")
            n += 1
    assert n >= 2


def test_refusals_need_no_gpu():
    """Every refusal comes before any launch: reached here with the address of a host buffer, which a refusing call
    never dereferences."""
    import ctypes
    from msml_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def rc(N=1, C=3, H=8, W=8, Cout=64, ldy=64, R=3, S=3, stride=1, pad=1, dy=p, w=p, dx=p, dtype=_lib.BF16, P=None, Q=None):
        P = (H + 2 * pad - R) // max(stride, 1) + 1 if P is None else P
        Q = (W + 2 * pad - S) // max(stride, 1) + 1 if Q is None else Q
        return lib.msml_stem_bwd_data(dy, w, dx, N, C, H, W, P, Q, Cout, ldy, R, S, stride, pad, dtype, None)
    assert rc(W=129) == -1 and b"W <= 128" in lib.msml_last_error()
    assert rc(R=5, S=5, pad=2) == -1                     # R*S*C = 75 > 32
    assert rc(stride=3) == -1 and rc(stride=0) == -1
    assert rc(dy=None) == -1 and rc(w=None) == -1 and rc(dx=None) == -1
    assert b"null" in lib.msml_last_error()
    assert rc(dy=p + 2) == -1                            # misaligned
    assert rc(C=2) == -1 and rc(R=3, S=5) == -1 and rc(pad=0) == -1
    assert rc(Cout=48, ldy=64) == -1 and rc(Cout=160, ldy=160) == -1 and rc(Cout=64, ldy=32) == -1 and rc(ldy=68) == -1
    assert rc(P=9) == -1 and rc(Q=7) == -1 and rc(N=0) == -1
    assert rc(dtype=7) == -2                             # MSML_ERR_DTYPE
    assert lib.msml_stem_bwd_data_band(3, 112, 129, 64, 3, 1) == 0
    assert lib.msml_stem_bwd_data_band(3, 112, 112, 64, 3, 1) >= 3


def test_the_budget_holds_for_an_f32_sum_and_exact_data_is_exact():
    """The f64 result rounded once to f32 is far inside the budget, and the integer data keep every partial sum below
    2^24 (so any f32 summation order gives the f64 result)."""
    for case in CASES:
        dy, w = S.operands(*S.random_data(case, torch.bfloat16))
        want, mag = S.adjoint_f64(dy, w, case), S.adjoint_f64(dy, w, case, absolute=True)
        assert S.worst_ratio(want.astype(np.float32), want, mag, case) < 0.01
        dy, w = S.operands(*S.exact_data(case, torch.bfloat16))
        assert float(S.adjoint_f64(dy, w, case, absolute=True).max()) < 2.0 ** 24
        assert np.array_equal(dy[..., :case.Cout], np.round(dy[..., :case.Cout])) and np.array_equal(w, np.round(w))
