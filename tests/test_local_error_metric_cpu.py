"""The element and row bounds of tests/util.py (elem_bound, assert_elementwise, row_err) on a CPU emulation of the kernels' rounding points:
f32 accumulation and ONE rounding to the stored 16-bit format; for the attention, the roundings of util.attn_model.

Two things are proven here, without a GPU:
  * an honest result stays within the bounds (worst element about 0.9 of the bf16 bound, as round-to-nearest predicts; a sliver of the f32 bound),
    in fp16's subnormal range too;
  * local faults of the kind hand-written tile kernels produce are flagged, although each PASSES the whole-tensor assertion the suite used alone
    until now.  Every test prints the Frobenius value (util.rel) and today's limit next to err / bound, so the output documents the gap.
"""
import pytest
import torch

from util import TANH_ABS, assert_elementwise, assert_rows_within, attn_model, attn_out_bound, attn_ref64, elem_bound, h16r, rel, row_err, worst_rows

F32_TOL, BF16_TOL, GRAD_TOL = 1e-5, 2.5e-3, 1e-2          # today's whole-tensor limits (tests/test_ops_gpu.py)
BF16, F16 = torch.bfloat16, torch.float16


def _operands(M, N, K, seed, dt=BF16, sa=0.5, sb=0.1):
    g = torch.Generator().manual_seed(seed)
    A = h16r(torch.randn(M, K, generator=g) * sa, dt)
    B = h16r(torch.randn(N, K, generator=g) * sb, dt)
    bias = torch.randn(N, generator=g)
    return A, B, bias


def _gemm_tanh(A, B, bias, dt):
    """the emulated kernel (f32 matmul, bias, tanh, one rounding), the fp64 reference and its element bound"""
    out = h16r(torch.tanh(A @ B.t() + bias), dt)
    pre = A.double() @ B.double().t() + bias.double()
    ref = torch.tanh(pre)
    mag = (A.double().abs() @ B.double().abs().t() + bias.double().abs()) * (1 - ref ** 2)
    return out, ref, elem_bound(ref, mag, A.shape[1], dt, extra_abs=TANH_ABS)


@pytest.fixture(scope="module")
def tanh_case():
    A, B, bias = _operands(1024, 768, 192, 1)
    return (A, B, bias) + _gemm_tanh(A, B, bias, BF16)


def _flagged(out, ref, bound, what, today, limit, tile=(256, 256), passes_today=True):
    """the fault fails the element bound — and (passes_today: the faults of the table in the module docstring's second point) passes the whole-tensor
    assertion; prints both figures"""
    if passes_today:
        assert today <= limit, f"{what}: the fault no longer passes today's metric ({today:.3e} > {limit:.1e}): it documents nothing"
    with pytest.raises(AssertionError) as e:
        assert_elementwise(out, ref, bound, what, tile=tile)
    msg = str(e.value)
    print(f"{what}: Frobenius {today:.3e} {'passes' if today <= limit else 'fails'} today's {limit:.1e}; {msg[len(what) + 2:]}")
    return msg


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
def test_honest_gemm_is_within_the_element_bound(dt):
    A, B, bias = _operands(1000, 200, 328, 2, dt)
    out, ref, bound = _gemm_tanh(A, B, bias, dt)
    w16 = assert_elementwise(out, ref, bound, f"bias + tanh -> {dt}", tile=(256, 256))
    acc = A @ B.t()
    ref32 = A.double() @ B.double().t()
    w32 = assert_elementwise(acc, ref32, elem_bound(ref32, A.double().abs() @ B.double().abs().t(), 328), "f32 output")
    plain = assert_elementwise(h16r(acc, dt), ref32, elem_bound(ref32, A.double().abs() @ B.double().abs().t(), 328, dt), f"{dt} output")
    print(f"honest {dt}: worst element uses {w16:.3f} of the bound (bias + tanh), {plain:.3f} (plain), {w32:.4f} of the f32 bound")
    assert w16 <= 1.0 and 0.5 <= plain <= 1.0 and w32 <= 0.1                 # the 16-bit bound is TIGHT: half an ulp at the bottom of a binade


def test_fp16_bound_admits_an_honest_result_in_the_subnormal_range():
    """operands scaled so that the outputs reach about 1e-6 (fp16's smallest normal is 6.1e-5, its subnormal spacing 6e-8): the relative term alone
    would reject the honest rounding there, the 2^-25 term admits it"""
    g = torch.Generator().manual_seed(3)
    A = h16r(torch.randn(256, 64, generator=g) * 2.0 ** -10, F16)
    B = h16r(torch.randn(128, 64, generator=g) * 2.0 ** -12, F16)
    out = h16r(A @ B.t(), F16)
    ref = A.double() @ B.double().t()
    mag = A.double().abs() @ B.double().abs().t()
    assert 3e-7 <= ref.abs().median().item() <= 3e-6 and ref.abs().max().item() < 6.1e-5
    w = assert_elementwise(out, ref, elem_bound(ref, mag, 64, F16), "fp16 subnormal outputs")
    no_sub = ((out.double() - ref).abs() / (2.0 ** -11 * ref.abs() + (2 * 64 + 8) * 2.0 ** -24 * mag)).max().item()
    print(f"fp16 outputs of median magnitude {ref.abs().median().item():.1e}: worst {w:.3f} of the bound; {no_sub:.1f} x without the subnormal term")
    assert w <= 1.0 < no_sub


def test_swapped_neighbours_are_flagged(tanh_case):
    A, B, bias, out, ref, bound = tanh_case
    bad = out.clone()
    bad[517, 300], bad[517, 301] = out[517, 301], out[517, 300]
    msg = _flagged(bad, ref, bound, "two neighbouring elements swapped, bias + tanh -> bf16, 1024x768x192", rel(bad, ref), BF16_TOL)
    assert "2 of" in msg and ("(5, 44)" in msg or "(5, 45)" in msg)          # row 517 = 2 * 256 + 5, columns 300 / 301 = 256 + 44 / 45


def test_block_off_by_two_percent_is_flagged(tanh_case):
    A, B, bias, out, ref, bound = tanh_case
    bad = out.clone()
    bad[256:288, 512:544] *= 1.02
    _flagged(bad, ref, bound, "a 32x32 block off by 2 %, bias + tanh -> bf16, 1024x768x192", rel(bad, ref), BF16_TOL)


def test_elements_without_bias_at_the_tile_corner_are_flagged(tanh_case):
    A, B, bias, out, ref, bound = tanh_case
    bad = out.clone()
    bad[1023, 760:] = h16r(torch.tanh(A[1023] @ B[760:].t()), BF16)
    msg = _flagged(bad, ref, bound, "8 elements without bias at the last row / last columns", rel(bad, ref), BF16_TOL)
    assert "(255, " in msg


def test_row_that_lost_its_last_k_step_is_flagged(tanh_case):
    A, B, bias, out, ref, bound = tanh_case
    bad = out.clone()
    bad[700] = h16r(torch.tanh(A[700, :184] @ B[:, :184].t() + bias), BF16)
    _flagged(bad, ref, bound, "one row that lost its last 8 of K = 192", rel(bad, ref), BF16_TOL, passes_today=False)


def test_duplicated_row_is_flagged(tanh_case):
    A, B, bias, out, ref, bound = tanh_case
    bad = out.clone()
    bad[255] = out[254]
    msg = _flagged(bad, ref, bound, "row 255 a copy of row 254", rel(bad, ref), BF16_TOL, passes_today=False)
    assert "(255, " in msg


def test_one_f32_element_off_by_half_a_percent_is_flagged():
    M, N, K = 4096, 2304, 768
    A, B, _ = _operands(M, N, K, 4)
    out = A @ B.t()
    ref = A.double() @ B.double().t()
    bound = elem_bound(ref, A.double().abs() @ B.double().abs().t(), K)
    w = assert_elementwise(out, ref, bound, "honest f32 output 4096x2304x768")
    i, j = 4095, 2303
    assert ref[i, j].abs() > 0.1 * ref.abs().mean()          # (not an element that happens to be zero)
    out[i, j] *= 1.005
    _flagged(out, ref, bound, f"one f32 element off by 0.5 % (honest worst {w:.4f} of the bound), 4096x2304x768", rel(out, ref), F32_TOL)


# ---------------------------------------------------------------------------------------------
# attention: element bound of the forward, row bound of the gradients against the fp64 model with the kernels' roundings
# ---------------------------------------------------------------------------------------------
def _attn_emulated(qkv, do, B, N, H, scale, dt):
    """the emulated kernels: f32 arithmetic, and a forward that differs from util.attn_model where the kernels do — the keys come in tiles of 64, the
    probabilities are rounded to 16 bits under the RUNNING maximum of the tiles seen so far, and the accumulator and the normaliser are rescaled
    whenever that maximum moves (the online softmax).  The backward starts from this forward's stored out / lse, as enh_attention_backward does."""
    r = lambda t: t.to(dt).float()
    q, k, v = qkv.float().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    m = torch.full((B, H, N, 1), float("-inf"))
    l, o = torch.zeros(B, H, N, 1), torch.zeros(B, H, N, 64)
    for t in range(0, N, 64):
        s = (q @ k[:, :, t:t + 64].transpose(-1, -2)) * scale
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha, e = torch.exp(m - m_new), torch.exp(s - m_new)
        l, o, m = l * alpha + e.sum(-1, keepdim=True), o * alpha + r(e) @ v[:, :, t:t + 64], m_new
    out = r(o / l).permute(0, 2, 1, 3).reshape(B, N, H * 64)
    lse = (m + torch.log(l)).squeeze(-1)
    return (out, lse) + attn_model(qkv, do, B, N, H, scale, dt, compute=torch.float32, out=out, lse=lse)[2:]


@pytest.fixture(scope="module")
def attn_case():
    B, N, H, scale = 2, 1024, 3, 0.125
    g = torch.Generator().manual_seed(5)
    qkv = h16r(torch.randn(B, N, 3 * H * 64, generator=g) * 1.5, BF16)
    do = h16r(torch.randn(B, N, H * 64, generator=g), BF16)
    ref = attn_ref64(qkv, do, B, N, H, scale)
    emu = _attn_emulated(qkv, do, B, N, H, scale, BF16)
    model = attn_model(qkv, do, B, N, H, scale, BF16, out=emu[0], lse=emu[1])      # as tests/test_elementwise_gpu.py: started from the stored out / lse
    own = attn_model(qkv, do, B, N, H, scale, BF16)                                 # ... and from the model's own forward (printed, not asserted)
    return H, ref, model, emu, own


def test_honest_attention_is_within_the_bounds(attn_case):
    H, (ref, lse_ref, pav, grads), model, emu, own = attn_case
    w = assert_elementwise(emu[0], ref, attn_out_bound(ref, pav, BF16), "attention forward, emulated")
    assert (emu[1].double() - lse_ref).abs().max().item() <= 1e-4
    print(f"honest attention forward (probabilities rounded under the running maximum): worst element {w:.3f} of the bound; "
          f"worst output row: emulation {worst_rows(emu[0], ref, H):.2e}, model {worst_rows(own[0], ref, H):.2e}")
    for name, e, m, o, r_ in zip(("dq", "dk", "dv"), emu[2:], model[2:], own[2:], grads):
        wm, wo = worst_rows(m, r_, H), worst_rows(o, r_, H)
        we = assert_rows_within(e, r_, H, 2 * wm, f"emulated {name}")
        print(f"  {name}: worst row of the emulation {we:.2e}, of the model {wm:.2e}: ratio {we / wm:.2f}  (of the model with its own forward {wo:.2e}: {we / wo:.2f})")


def test_unwritten_row_in_a_later_head_is_flagged(attn_case):
    """a NaN row (what a row the kernels never write looks like in a NaN-filled buffer) in head 1 of dk: Python's max() over the heads would drop it
    (max([1.0, nan, 1.0]) == 1.0); worst_rows gives nan, which no `<=` admits, and assert_rows_within names the row"""
    H, (ref, lse_ref, pav, grads), model, emu, own = attn_case
    bad = emu[3].clone()
    bad[1, 1023, 64:128] = float("nan")
    w = worst_rows(bad, grads[1], H)
    assert w != w and not (w <= 2 * worst_rows(model[3], grads[1], H))
    with pytest.raises(AssertionError, match="batch 1, token 1023, head 1"):
        assert_rows_within(bad, grads[1], H, 1.0, "dk with an unwritten row")
    bad = emu[4].clone()
    bad[0, 3, 150] = float("inf")                              # one element of head 2 of dv
    with pytest.raises(AssertionError, match="batch 0, token 3, head 2"):
        assert_rows_within(bad, grads[2], H, 1.0, "dv with an overflowed element")


def test_halved_dq_row_and_zeroed_dk_row_are_flagged(attn_case):
    H, (ref, lse_ref, pav, grads), model, emu, own = attn_case
    # a row of average norm is 1 / sqrt(6144 rows) = 1.3e-2 of its tensor: the faults that slip under 1e-2 sit in rows somewhat below the average (0.8
    # and 0.6 of the RMS row norm here), which is where the row metric lands for them
    for name, t, factor, size in (("dq", 2, 0.5, 0.8), ("dk", 3, 0.0, 0.6)):
        r_ = grads[t - 2]
        norms = r_[..., 64:128].norm(dim=-1)
        b, n = divmod(int((norms / norms.pow(2).mean().sqrt() - size).abs().argmin()), norms.shape[1])
        bad = emu[t].clone()
        bad[b, n, 64:128] *= factor
        today = rel(bad, r_)
        we, wm = worst_rows(bad, r_, H), worst_rows(model[t], r_, H)
        print(f"one whole {name} row (b, n, h) {'halved' if factor else 'zeroed'}, B=2 N=1024 H=3: Frobenius {today:.3e} passes today's {GRAD_TOL:.0e}; "
              f"worst row {we:.2f} = {we / wm:.0f} x the model's {wm:.2e} (limit 2 x)")
        assert today <= GRAD_TOL and we > 2 * wm


def test_row_err_is_normalised_by_the_tensor_not_the_row():
    ref = torch.ones(4, 64)
    ref[3] *= 1e-3
    x = ref.clone()
    x[3] *= 1.5                                               # 50 % of a tiny row: nothing against the tensor's scale
    x[0, 0] += 0.8
    e = row_err(x, ref, 64)
    rms = (3 * 64 + 64e-6) ** 0.5 / 2
    assert e.shape == (4,) and abs(e[0].item() - 0.8 / rms) < 1e-6 and e[3].item() < 1e-3 and e[1].item() == 0.0


def test_assert_elementwise_reports_nan_and_zero_bounds():
    ref = torch.zeros(2, 8)
    assert assert_elementwise(torch.zeros(2, 8), ref, torch.zeros(2, 8), "exact zeros") == 0.0
    out = torch.zeros(2, 8)
    out[1, 3] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 16 .* \(1, 3\)"):
        assert_elementwise(out, ref, torch.ones(2, 8), "nan")
