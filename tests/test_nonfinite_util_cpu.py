"""tests/nonfinite_util.py on CPU emulations of the kernels' arithmetic (f32 accumulation, ONE rounding to the stored 16-bit format), without a GPU:

  * an honest GEMM row, LayerNorm row and softmax row pass assert_no_swallow, assert_isolated and check_overflow, with an inf and with a NaN in the input;
  * the faults a hand-written kernel produces are caught, each by the helper meant for it: a pack that saturates to 65504 (check_overflow), nan_to_num
    on one output (assert_no_swallow), a row maximum taken with fmax followed by a select that zeroes the NaN probability (assert_no_swallow), one
    element of a neighbouring unit changed by one ulp (assert_isolated), an inf moved one position (check_overflow, exact or not)."""
import pytest
import torch

from nonfinite_util import assert_all_finite_within, assert_isolated, assert_no_swallow, check_overflow, element_bound, floor_bound, pow2_scale
from util import elem_bound, h16r

BF16, F16 = torch.bfloat16, torch.float16
DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
POISONS = pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
M, N, K, I0 = 96, 80, 72, 37


def _operands(dt, seed=1):
    g = torch.Generator().manual_seed(seed)
    return h16r(torch.randn(M, K, generator=g) * 0.5, dt), h16r(torch.randn(N, K, generator=g) * 0.1, dt)


def _gemm(A, B, dt):
    """the emulated kernel: f32 products and sums, one rounding"""
    return (A @ B.t()).to(dt)


def _gemm64(A, B):
    return A.double() @ B.double().t()


def _row_mask(rows, i):
    m = torch.zeros(rows, 1, dtype=torch.bool)
    m[i] = True
    return m


def _ln(x, w, b, dt):
    mean = x.mean(1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(1, keepdim=True) + 1e-5).rsqrt()
    return ((x - mean) * rstd * w + b).to(dt)


def _softmax(s, dt, rowmax=lambda s: s.max(-1, keepdim=True).values, select=False):
    p = torch.exp(s - rowmax(s))
    if select:
        p = torch.where(p == p, p, torch.zeros_like(p))
    return (p / p.sum(-1, keepdim=True)).to(dt)


# ---------------------------------------------------------------------------------------------
# honest emulations pass
# ---------------------------------------------------------------------------------------------
@DTS
@POISONS
def test_honest_gemm_row_propagates_and_stays_in_its_row(dt, poison):
    A, B = _operands(dt)
    clean = _gemm(A, B, dt)
    Ap = A.clone()
    Ap[I0, K - 1] = poison
    got = _gemm(Ap, B, dt)
    assert assert_no_swallow(got, _gemm64(Ap, B), f"gemm row {dt}") == 0
    assert_isolated(got, clean, _row_mask(M, I0), f"gemm row {dt}")
    Bp = B.clone()
    Bp[11, 0] = poison
    got = _gemm(A, Bp, dt)
    assert assert_no_swallow(got, _gemm64(A, Bp), f"gemm column {dt}") == 0
    assert_isolated(got, clean, _row_mask(N, 11).t(), f"gemm column {dt}")
    # an f32 output: the reference is not rounded
    assert assert_no_swallow(Ap @ B.t(), _gemm64(Ap, B), "gemm row f32") == 0


@DTS
@POISONS
def test_honest_layernorm_row(dt, poison):
    g = torch.Generator().manual_seed(2)
    x, w, b = torch.randn(5, 256, generator=g) * 2 + 0.5, 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    clean = _ln(x, w, b, dt)
    xp = x.clone()
    xp[3, 17] = poison
    got = _ln(xp, w, b, dt)
    ref = torch.nn.functional.layer_norm(xp.double(), (256,), w.double(), b.double(), 1e-5)
    assert not torch.isfinite(ref[3]).any() and torch.isfinite(ref[:3]).all()
    assert_no_swallow(got, ref, f"layernorm {dt}")
    assert_isolated(got, clean, _row_mask(5, 3), f"layernorm {dt}")


@DTS
@POISONS
def test_honest_softmax_row(dt, poison):
    g = torch.Generator().manual_seed(3)
    s = torch.randn(6, 72, generator=g) * 3
    clean = _softmax(s, dt)
    sp = s.clone()
    sp[4, 71] = poison
    got = _softmax(sp, dt)
    ref = torch.softmax(sp.double(), -1)
    assert not torch.isfinite(ref[4]).any()
    assert_no_swallow(got, ref, f"softmax {dt}")
    assert_isolated(got, clean, _row_mask(6, 4), f"softmax {dt}")


def _overflow_case():
    A, B = _operands(F16, 4)
    A = A * pow2_scale(_gemm64(A, B))
    ref = _gemm64(A, B)
    bound = elem_bound(ref, A.double().abs() @ B.double().abs().t(), K, F16)
    return A, B, ref, bound


def test_honest_overflow_is_exact_and_bf16_holds_the_range():
    A, B, ref, bound = _overflow_case()
    got = _gemm(A, B, F16)
    assert check_overflow(got, ref, element_bound(bound), "gemm fp16") == 0
    check_overflow(got, ref, floor_bound(1.25, F16), "gemm fp16, floor bound")
    assert check_overflow(got, ref, element_bound(bound), "gemm fp16, inexact mode", exact=False) == 0
    assert_all_finite_within(_gemm(A, B, BF16), ref, elem_bound(ref, A.double().abs() @ B.double().abs().t(), K, BF16), "gemm bf16")


def test_sixteen_bit_intermediate_passes_only_the_inexact_mode():
    """a kernel that packs an intermediate to fp16 (as the attention backward packs dS): an overflow of the intermediate is an inf or NaN where the
    reference is finite — spurious, counted, and no fault; the exact mode rejects it"""
    A, B, ref, bound = _overflow_case()
    got = _gemm(A, B, F16).float()
    fin = torch.isfinite(got).nonzero()
    i, j = (int(v) for v in fin[0])
    got[i, j] = float("nan")
    assert check_overflow(got, ref, element_bound(bound), "spurious NaN", exact=False) == 1
    with pytest.raises(AssertionError, match="NaN"):
        check_overflow(got, ref, element_bound(bound), "spurious NaN")
    assert assert_no_swallow(got.to(F16), ref, "spurious NaN") == 1


def test_a_case_that_does_not_overflow_is_refused():
    A, B = _operands(F16, 4)
    with pytest.raises(AssertionError, match="must overflow in part"):
        check_overflow(_gemm(A, B, F16), _gemm64(A, B), floor_bound(), "no overflow")


# ---------------------------------------------------------------------------------------------
# injected faults
# ---------------------------------------------------------------------------------------------
def test_saturating_pack_is_caught():
    A, B, ref, bound = _overflow_case()
    bad = (A @ B.t()).clamp(-65504.0, 65504.0).to(F16)
    for exact in (True, False):
        with pytest.raises(AssertionError):
            check_overflow(bad, ref, element_bound(bound), "saturating pack", exact=exact)
    with pytest.raises(AssertionError, match="came out finite"):
        assert_no_swallow(bad, ref, "saturating pack")
    # the same pack on an inf input
    Ap, B = _operands(F16)
    Ap[I0, K - 1] = float("inf")
    with pytest.raises(AssertionError, match=rf"{N} of {N} .*\({I0}, 0\)"):
        assert_no_swallow((Ap @ B.t()).clamp(-65504.0, 65504.0).to(F16), _gemm64(Ap, B), "saturating pack, inf input")


@DTS
def test_nan_to_num_on_one_output_is_caught(dt):
    A, B = _operands(dt)
    A[I0, K - 1] = float("nan")
    bad = _gemm(A, B, dt)
    bad[I0, 5] = torch.nan_to_num(bad[I0, 5])
    with pytest.raises(AssertionError, match=rf"1 of {N} .*\({I0}, 5\)"):
        assert_no_swallow(bad, _gemm64(A, B), "nan_to_num")


@DTS
def test_fmax_and_select_that_drop_a_nan_are_caught(dt):
    g = torch.Generator().manual_seed(3)
    s = torch.randn(6, 72, generator=g) * 3
    s[4, 71] = float("nan")
    fmax = _fmax_rows
    bad = _softmax(s, dt, rowmax=fmax, select=True)
    assert torch.isfinite(bad.float()).all()                      # the NaN score is gone: the row looks healthy
    with pytest.raises(AssertionError, match=r"72 of 72 .*\(4, 0\)"):
        assert_no_swallow(bad, torch.softmax(s.double(), -1), "fmax + select")
    # fmax alone is harmless as long as the NaN probability reaches the row sum: the whole row is NaN again
    assert assert_no_swallow(_softmax(s, dt, rowmax=fmax), torch.softmax(s.double(), -1), "fmax alone") == 0


def _fmax_rows(t):
    m = t[..., :1]
    for j in range(1, t.shape[-1]):
        m = torch.fmax(m, t[..., j:j + 1])
    return m


@DTS
def test_one_ulp_in_a_neighbouring_unit_is_caught(dt):
    A, B = _operands(dt)
    clean = _gemm(A, B, dt)
    A[I0, K - 1] = float("inf")
    bad = _gemm(A, B, dt)
    bits = bad.view(torch.int16)
    bits[I0 + 1, 9] += 1
    with pytest.raises(AssertionError, match=rf"1 elements outside .*\({I0 + 1}, 9\)"):
        assert_isolated(bad, clean, _row_mask(M, I0), "one ulp")
    f32 = (A @ B.t())
    f32c = f32.clone()
    f32.view(torch.int32)[0, 0] += 1
    with pytest.raises(AssertionError, match=r"\(0, 0\)"):
        assert_isolated(f32, f32c, _row_mask(M, I0), "one ulp, f32")
    with pytest.raises(AssertionError, match="covers the whole output"):
        assert_isolated(bad, clean, torch.ones(M, 1, dtype=torch.bool), "empty check")


def test_an_inf_moved_one_position_is_caught():
    A, B, ref, bound = _overflow_case()
    good = _gemm(A, B, F16).float()
    inf = torch.isinf(good)
    cand = (inf[:, :-1] & ~inf[:, 1:]).nonzero()                   # an inf whose right neighbour is finite
    i, j = (int(v) for v in cand[0])
    bad = good.clone()
    bad[i, j], bad[i, j + 1] = ref[i, j].clamp(-6e4, 6e4).float(), good[i, j]
    with pytest.raises(AssertionError, match="exactly where"):
        check_overflow(bad, ref, element_bound(bound), "moved inf")
    with pytest.raises(AssertionError, match="came out finite"):
        check_overflow(bad, ref, element_bound(bound), "moved inf", exact=False)
    with pytest.raises(AssertionError, match=rf"\({i}, {j}\)"):
        assert_no_swallow(bad.to(F16), ref, "moved inf")
