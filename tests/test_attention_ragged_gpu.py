"""The fused attention at token counts that are no multiple of 64 (the tail kernels: csrc/attention_tail.hip, x3_tail.hip, attention_kernels.h).

An (image, head) attends over its own keys 0 .. N-1 and nothing else: the ragged last tile is staged with clamped rows, its keys >= N get probability
exactly 0, and every store is guarded per lane.  Shapes (B, N, H) and what each one catches:
    (2, 40, 2)    one ragged tile, wave 1 with 8 live rows, waves 2-3 idle, leakage from the next image
    (2, 100, 2)   one full plus one ragged tile
    (1, 129, 2)   odd N, a second workgroup with ONE live query / key, a one-row tail tile
    (2, 136, 1)   eight-row tail
    (2, 196, 3)   224 px / patch 16: three full tiles plus four rows
    (1, 784, 2)   224 px / patch 8: twelve tiles plus 16 rows (odd / even ring stage)
    (1, 1, 1)     a single token
each for plain and pre-scaled q, bf16 and fp16, with the limits of tests/test_elementwise_gpu.py::_check_attention (the project's numbers, not new ones):
out within util.attn_out_bound per element, lse rel <= 1e-5 and abs <= 1e-4, every row of dq / dk / dv finite in a NaN-prefilled dqkv and within
ATT_MARGIN = 2 x the worst row of util.attn_model fed the kernel's stored out / lse.  The fp64 reference of a case is computed once and shared.
"""
import pytest
import torch

from util import SUB16, assert_elementwise, assert_rows_within, attn_model, attn_out_bound, attn_ref64, bf16_floor, h16r, rel, worst_rows

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
LOG2E = 1.4426950408889634
ATT_MARGIN = 2.0          # tests/test_elementwise_gpu.py
RAGGED_SHAPES = [(2, 40, 2), (2, 100, 2), (1, 129, 2), (2, 136, 1), (2, 196, 3), (1, 784, 2), (1, 1, 1)]
GUARD_ROWS = 64           # rows behind every tensor of the guard case
SENTINEL = 12345.0        # finite, representable in bf16 / fp16 / f32, never produced by these inputs
_CACHE = {}


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _spiked_qkv_ragged(g, B, N, H):
    """the layout of tests/test_elementwise_gpu.py::_spiked_qkv (keys dominating a row: key 300 of head 0 aligned with query 5, a staircase for query 70 of
    head 1, each step beating everything before it) with the LAST step moved to key N - 3, inside the ragged tile: the rescale branch runs in the
    masked tile"""
    assert N % 64 >= 3 and N > 320
    qkv = torch.randn(B, N, 3 * H * 64, generator=g)
    qkv[0, 5, :64] *= 6.0
    qkv[0, 300, H * 64:H * 64 + 64] = qkv[0, 5, :64] * 1.5
    qv = qkv[0, 70, 64:128].clone()
    for key, gain in ((100, 2.0), (130, 4.0), (200, 7.0), (N - 3, 11.0)):
        qkv[0, key, H * 64 + 64:H * 64 + 128] = qv * gain
    return qkv


def _case(B, N, H, pre, dt, spiked=False):
    """inputs and the fp64 reference, once per (shape, convention, format) — as tests/test_elementwise_gpu.py::_att_case"""
    key = (B, N, H, pre, dt, spiked)
    if key not in _CACHE:
        scale = 0.125
        g = torch.Generator().manual_seed(0 if spiked else B * 100 + N + H)
        qkv = h16r(_spiked_qkv_ragged(g, B, N, H) if spiked else torch.randn(B, N, 3 * H * 64, generator=g) * 1.5, dt)
        do = h16r(torch.randn(B, N, H * 64, generator=g), dt)
        qdev, qref = qkv, qkv.double()
        if pre:       # include/enh_hip.h q_prescaled: the q third holds dt(q * scale * log2e); the reference is taken on the UNSCALED values those bits represent
            qdev = qkv.clone()
            qdev[..., :H * 64] = h16r(qkv[..., :H * 64] * (scale * LOG2E), dt)
            qref = qdev.double().clone()
            qref[..., :H * 64] /= (scale * LOG2E)
        ref, lse_ref, pav, grads = attn_ref64(qref, do, B, N, H, scale)
        _CACHE[key] = dict(scale=scale, qref=qref, do64=do, qd=qdev.to(dt), do=do.to(dt), ref=ref, lse=lse_ref, bound=attn_out_bound(ref, pav, dt), grads=grads)
    return _CACHE[key]


def _guarded(t, fill):
    """`t` at the FRONT of a larger allocation whose remainder — GUARD_ROWS rows of t's last axis — holds `fill`; returns (view of the front, the whole allocation)"""
    n_guard = GUARD_ROWS * t.shape[-1]
    whole = torch.empty(t.numel() + n_guard, dtype=t.dtype, device="cuda")
    whole[:t.numel()] = t.reshape(-1).cuda()
    whole[t.numel():] = fill
    return whole[:t.numel()].view(t.shape), whole


def _check(C, B, N, H, pre, dt, spiked=False, fam=(0, 0, 0), guard=False):
    c = _case(B, N, H, pre, dt, spiked)
    what = f"ragged attention {'spiked ' if spiked else ''}{'guarded ' if guard else ''}family {fam} B={B} N={N} H={H} {'prescaled' if pre else 'plain'} {dt}"
    nan = float("nan")
    out0 = torch.full((B, N, H * 64), nan, dtype=dt)
    lse0, dqkv0 = torch.full((B, H, N), nan), torch.full((B, N, 3 * H * 64), nan, dtype=dt)
    if guard:
        # inputs: the 64 rows behind them hold NaN bit patterns (an over-read that reaches arithmetic poisons the result); outputs: a finite sentinel
        # behind them (an over-write changes its bits).  Nothing here faults: every allocation covers what a 64-row over-run would touch.
        (qd, _), (do, _) = _guarded(c["qd"], nan), _guarded(c["do"], nan)
        (out, out_w), (lse, lse_w), (dqkv, dqkv_w) = _guarded(out0, SENTINEL), _guarded(lse0, SENTINEL), _guarded(dqkv0, SENTINEL)
        delta, delta_w = _guarded(torch.full((B, H, N), nan), SENTINEL)
    else:
        qd, do, out, lse, dqkv = c["qd"].cuda(), c["do"].cuda(), out0.cuda(), lse0.cuda(), dqkv0.cuda()
        delta = torch.empty(B, H, N, device="cuda")
    try:
        C.attention_set_kernel(*fam)
        C.attention_forward(qd, B, N, H, c["scale"], out, lse, q_prescaled=pre)
        if guard:       # the backward reads out: NaN behind it from here on (the sentinel was compared first)
            torch.cuda.synchronize()
            assert bool((out_w[out.numel():] == SENTINEL).all()) and bool((lse_w[lse.numel():] == SENTINEL).all()), what + ": the forward wrote past out / lse"
            out_w[out.numel():] = nan
        C.attention_backward(qd, out, do, lse, B, N, H, c["scale"], dqkv, delta, q_prescaled=pre)
        torch.cuda.synchronize()
    finally:
        C.attention_set_kernel(0, 0, 0)
    if guard:
        for name, view, whole in (("lse", lse, lse_w), ("dqkv", dqkv, dqkv_w), ("delta", delta, delta_w)):
            assert bool((whole[view.numel():] == SENTINEL).all()), f"{what}: wrote past {name}"
    w = assert_elementwise(out, c["ref"], c["bound"], what + " out", tile=(64, 64))
    e_lse = (lse.double().cpu() - c["lse"]).abs().max().item()
    r_lse = rel(lse, c["lse"])
    got = dqkv.float().cpu().view(B, N, 3, H * 64).unbind(2)
    model = attn_model(c["qref"], c["do64"], B, N, H, c["scale"], dt, out=out, lse=lse)
    names = ("dq", "dk", "dv")
    if N == 1:
        # One key: P = 1, so dS = P (dP - delta) and with it dq and dk are exactly 0 in exact arithmetic, and the row metric (normalised by the
        # reference's row norms) has nothing to divide by.  The kernels form dP = dO . v on the matrix pipe and delta = dO . out in a chain of f32
        # multiply-adds; out = v here, so the two are f32 sums of the SAME 64 products in two orders, each within gamma_64 of the exact sum:
        # |dS| <= 2 (2 * 64 + 8) 2^-24 sum_d |dO_d| |v_d|   (the constant of util.elem_bound, once per sum), and |dq_d| <= |dS| |k_d| scale,
        # |dk_d| <= |dS| |q_d| scale, plus the rounding of the store (fp16: values this small are subnormal, util.SUB16).
        # dv = P^T dO with P = exp2(s - lse) = 1 up to the f32 error of lse and exp2 (1e-6 at most), which rounds to exactly 1 in either 16-bit format
        # (half an ulp at 1 is 2^-9 / 2^-12): dv is dO, bit for bit — what util.attn_model gives too (its worst row is 0, so a ratio has no meaning here).
        q, k, v = c["qref"].view(B, N, 3, H * 64).unbind(2)
        ds = (2 * (2 * 64 + 8) * 2.0 ** -24) * (c["do64"].double().abs() * v.abs()).view(B, N, H, 64).sum(-1, keepdim=True).expand(B, N, H, 64).reshape(B, N, H * 64)
        for n, t, other in (("dq", got[0], k), ("dk", got[1], q)):
            assert_elementwise(t, torch.zeros_like(ds), ds * other.abs() * c["scale"] * (1 + 2.0 ** -8) + SUB16.get(dt, 0.0), f"{what} {n} (exactly 0 in exact arithmetic)")
        assert torch.equal(got[2].double(), c["do64"].double()) and torch.equal(model[4].double(), c["do64"].double()), f"{what} dv is not dO"
        names, got, model = (), (), model[:2]
    model_rows = [worst_rows(m, r_, H) for m, r_ in zip(model[2:], c["grads"])]
    assert all(m == m and m > 0 for m in model_rows), (what, model_rows)
    rows = [assert_rows_within(t, r_, H, ATT_MARGIN * m, f"{what} {n}") for n, t, r_, m in zip(names, got, c["grads"], model_rows)]
    ratios = [k / m for k, m in zip(rows, model_rows)]
    print(f"{what}: out max err / bound {w:.3f}, lse max abs {e_lse:.1e} rel {r_lse:.1e}, worst gradient row kernel / model "
          + " ".join(f"{n} {k:.2e} / {m:.2e} = {r_:.2f}" for n, k, m, r_ in zip(names, rows, model_rows, ratios)))
    assert r_lse <= 1e-5 and e_lse <= 1e-4, (what, r_lse, e_lse)
    assert not any(not (r_ <= ATT_MARGIN) for r_ in ratios), (what, ratios)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", RAGGED_SHAPES)
def test_ragged_attention_every_element_and_row(C, B, N, H, pre, dt):
    _check(C, B, N, H, pre, dt)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", [(2, 40, 2), (2, 196, 3)])
def test_ragged_attention_reads_and_writes_nothing_outside_its_tensors(C, B, N, H, pre, dt):
    """qkv, out and dout at the front of larger allocations: NaN bit patterns in the 64 rows behind the inputs, a finite sentinel behind out / lse / delta /
    dqkv.  The results still meet the bounds (no over-read value reached the arithmetic) and the sentinels keep their bits (no over-write)."""
    _check(C, B, N, H, pre, dt, guard=True)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
def test_ragged_attention_spiked_scores_in_the_masked_tile(C, pre):
    """N = 500: seven full tiles and 52 keys; the last step of the staircase is key 497, so the reference is raised inside the masked tile"""
    _check(C, 1, 500, 2, pre, BF16, spiked=True)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", [(2, 100, 2), (2, 196, 3)])
def test_ragged_attention_is_bit_reproducible_across_launches(C, B, N, H, pre):
    """as tests/test_ops_gpu.py::test_attention_is_bit_reproducible_across_launches: five launches with unrelated work in between, identical bits"""
    g = torch.Generator(device="cuda").manual_seed(B + N + H)
    qkv = (torch.randn(B, N, 3 * H * 64, device="cuda", generator=g) * 1.2).to(BF16)
    do = torch.randn(B, N, H * 64, device="cuda", generator=g).to(BF16)
    runs = []
    for rep in range(5):
        out = torch.full((B, N, H * 64), float("nan"), dtype=BF16, device="cuda")
        lse = torch.full((B, H, N), float("nan"), device="cuda")
        dqkv = torch.full_like(qkv, float("nan")); delta = torch.full((B, H, N), float("nan"), device="cuda")
        if rep % 2:
            torch.empty(1 << 24, device="cuda").normal_()        # unrelated work between the launches (other cache / clock state)
        C.attention_forward(qkv, B, N, H, 0.125, out, lse, q_prescaled=pre)
        C.attention_backward(qkv, out, do, lse, B, N, H, 0.125, dqkv, delta, q_prescaled=pre)
        torch.cuda.synchronize()
        runs.append((out, lse, dqkv, delta))
    for k, name in enumerate(("out", "lse", "dqkv", "delta")):
        it = torch.int16 if k in (0, 2) else torch.int32
        assert not bool(torch.isnan(runs[0][k]).any()), f"{name}: an element was never written"
        for r in runs[1:]:
            assert torch.equal(runs[0][k].view(it), r[k].view(it)), f"{name}: {(runs[0][k] != r[k]).sum().item()} elements differ between two launches on the same input"


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
def test_ragged_attention_ignores_the_kernel_family(C, pre):
    """enh_attention_set_kernel selects among the ALIGNED kernels; a ragged N runs its tail form under any selection and still meets the bounds"""
    _check(C, 2, 100, 2, pre, BF16, fam=(1, 1, 1))


@pytest.mark.parametrize("B,N,H", [(2, 100, 2), (1, 196, 2)])
def test_ragged_attention_x3_vs_fp64(C, B, N, H):
    """tests/test_x3_gpu.py::test_attention_x3_vs_fp64 at ragged N, same limits: 3e-5 on the recombined output, lse 1e-4 absolute, the hi plane within
    1.15 x the bf16 rounding floor; rows the kernel must write are NaN-prefilled"""
    torch.manual_seed(3)
    qkv = torch.randn(B, N, 3 * H * 64, device="cuda")
    qkv[..., :H * 64] *= 2.0       # scores with some spread
    hi = torch.empty(B * N, 3 * H * 64, dtype=BF16, device="cuda"); lo = torch.empty_like(hi)
    C.split2(qkv.view(B * N, -1), hi, lo)
    out3 = torch.full((B * N, 3 * H * 64), float("nan"), dtype=BF16, device="cuda")
    out16 = torch.full((B * N, H * 64), float("nan"), dtype=BF16, device="cuda")
    lse = torch.full((B, H, N), float("nan"), device="cuda")
    C.attention_forward_x3(hi, lo, B, N, H, 0.125, out3, out16, lse)
    q, k, v = (t.view(B, N, H, 64).permute(0, 2, 1, 3).double() for t in qkv.chunk(3, dim=-1))
    s = q @ k.transpose(-1, -2) * 0.125
    ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * N, H * 64)
    D = H * 64
    got = out3[:, :D].float() + out3[:, D:2 * D].float()
    e, e_lse = rel(got, ref), (lse.double() - torch.logsumexp(s, -1)).abs().max().item()
    print(f"ragged attention x3 B={B} N={N} H={H}: out rel {e:.2e}, lse abs {e_lse:.1e}, hi plane {rel(out16, ref):.2e} (bf16 floor {bf16_floor(ref):.2e})")
    assert bool(torch.isfinite(out3.float()).all()) and bool(torch.isfinite(lse).all())
    assert e <= 3e-5
    assert e_lse <= 1e-4
    assert torch.equal(out3[:, :D], out3[:, 2 * D:]) and torch.equal(out16, out3[:, :D])
    assert rel(out16, ref) <= 1.15 * bf16_floor(ref)
