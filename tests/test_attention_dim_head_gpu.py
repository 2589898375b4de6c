"""The fused attention at head widths 32, 96 and 128 (csrc/attention_dh.h; enh_attention_forward_dh / enh_attention_backward_dh and their f32 forms).

Shapes (B, N, H), for every D, both operand formats and both q conventions, with scale = D^-0.5 — and what each one catches:
    (2, 64, 2)    one aligned tile, second image / head offsets
    (1, 192, 2)   three tiles (both ring stages, odd count), a second workgroup of 64 live queries
    (2, 40, 2)    one ragged tile, a wave with 8 live rows, idle waves, leakage from the next image
    (1, 129, 2)   a workgroup with ONE live query / key, a one-row tile
    (2, 196, 3)   H = 3 (head offsets 3 D), three tiles plus four rows
    (1, 1, 1)     a single token
Limits as tests/test_attention_ragged_gpu.py::_check with 64 -> D (attn_dh_util.py: the helpers of util.py with a D argument): out within attn_out_bound
per element, lse rel <= 1e-5 and abs <= 1e-4, NaN-prefilled out / lse / dqkv finite afterwards, every dq / dk / dv row within ATT_MARGIN = 2 x the
worst row of the CPU model fed the kernel's stored out / lse.  The fp64 reference of a case is computed once and shared."""
import os
import sys

import pytest
import torch

from attn_dh_util import assert_rows_within, attn_model, attn_out_bound, attn_ref64, worst_rows
from util import SUB16, assert_elementwise, h16r, rel

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
LOG2E = 1.4426950408889634
ATT_MARGIN = 2.0          # tests/test_elementwise_gpu.py
WIDTHS = [32, 96, 128]
SHAPES = [(2, 64, 2), (1, 192, 2), (2, 40, 2), (1, 129, 2), (2, 196, 3), (1, 1, 1)]
GUARD_ROWS = 64           # rows behind every tensor of the guard case
SENTINEL = 12345.0        # finite, representable in bf16 / fp16 / f32, never produced by these inputs
_CACHE = {}


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _spiked_qkv(g, B, N, H, D):
    """tests/test_attention_ragged_gpu.py::_spiked_qkv_ragged with 64 -> D: key 300 of head 0 aligned with query 5, a staircase for query 70 of head 1,
    each step beating everything before it, the last step at key N - 3 inside the ragged tile (the rescale branch runs in the masked tile)"""
    assert N % 64 >= 3 and N > 320 and H >= 2
    qkv = torch.randn(B, N, 3 * H * D, generator=g)
    qkv[0, 5, :D] *= 6.0
    qkv[0, 300, H * D:H * D + D] = qkv[0, 5, :D] * 1.5
    qv = qkv[0, 70, D:2 * D].clone()
    for key, gain in ((100, 2.0), (130, 4.0), (200, 7.0), (N - 3, 11.0)):
        qkv[0, key, H * D + D:H * D + 2 * D] = qv * gain
    return qkv


def _case(D, B, N, H, pre, dt, spiked=False):
    """inputs and the fp64 reference, once per (width, shape, convention, format)"""
    key = (D, B, N, H, pre, dt, spiked)
    if key not in _CACHE:
        scale = D ** -0.5
        g = torch.Generator().manual_seed(0 if spiked else D * 1000 + B * 100 + N + H)
        qkv = h16r(_spiked_qkv(g, B, N, H, D) if spiked else torch.randn(B, N, 3 * H * D, generator=g) * 1.5, dt)
        do = h16r(torch.randn(B, N, H * D, generator=g), dt)
        qdev, qref = qkv, qkv.double()
        if pre:       # include/enh_hip.h q_prescaled: the q third holds dt(q * scale * log2e); the reference is taken on the UNSCALED values those bits represent
            qdev = qkv.clone()
            qdev[..., :H * D] = h16r(qkv[..., :H * D] * (scale * LOG2E), dt)
            qref = qdev.double().clone()
            qref[..., :H * D] /= (scale * LOG2E)
        ref, lse_ref, pav, grads = attn_ref64(qref, do, B, N, H, D, scale)
        _CACHE[key] = dict(scale=scale, qref=qref, do64=do, qd=qdev.to(dt), do=do.to(dt), ref=ref, lse=lse_ref, bound=attn_out_bound(ref, pav, dt, D), grads=grads)
    return _CACHE[key]


def _guarded(t, fill):
    """`t` at the FRONT of a larger allocation whose remainder — GUARD_ROWS rows of t's last axis — holds `fill`; returns (view of the front, the whole allocation)"""
    n_guard = GUARD_ROWS * t.shape[-1]
    whole = torch.empty(t.numel() + n_guard, dtype=t.dtype, device="cuda")
    whole[:t.numel()] = t.reshape(-1).cuda()
    whole[t.numel():] = fill
    return whole[:t.numel()].view(t.shape), whole


def _check(C, D, B, N, H, pre, dt, spiked=False, guard=False):
    c = _case(D, B, N, H, pre, dt, spiked)
    what = f"attention dim_head {D} {'spiked ' if spiked else ''}{'guarded ' if guard else ''}B={B} N={N} H={H} {'prescaled' if pre else 'plain'} {dt}"
    nan = float("nan")
    out0 = torch.full((B, N, H * D), nan, dtype=dt)
    lse0, dqkv0 = torch.full((B, H, N), nan), torch.full((B, N, 3 * H * D), nan, dtype=dt)
    if guard:
        # inputs: the 64 rows behind them hold NaN bit patterns (an over-read that reaches arithmetic poisons the result); outputs: a finite sentinel
        # behind them (an over-write changes its bits).  Nothing here faults: every allocation covers what a 64-row over-run would touch.
        (qd, _), (do, _) = _guarded(c["qd"], nan), _guarded(c["do"], nan)
        (out, out_w), (lse, lse_w), (dqkv, dqkv_w) = _guarded(out0, SENTINEL), _guarded(lse0, SENTINEL), _guarded(dqkv0, SENTINEL)
        delta, delta_w = _guarded(torch.full((B, H, N), nan), SENTINEL)
    else:
        qd, do, out, lse, dqkv = c["qd"].cuda(), c["do"].cuda(), out0.cuda(), lse0.cuda(), dqkv0.cuda()
        delta = torch.empty(B, H, N, device="cuda")
    C.attention_forward(qd, B, N, H, c["scale"], out, lse, q_prescaled=pre, dim_head=D)
    if guard:       # the backward reads out: NaN behind it from here on (the sentinel was compared first)
        torch.cuda.synchronize()
        assert bool((out_w[out.numel():] == SENTINEL).all()) and bool((lse_w[lse.numel():] == SENTINEL).all()), what + ": the forward wrote past out / lse"
        out_w[out.numel():] = nan
    C.attention_backward(qd, out, do, lse, B, N, H, c["scale"], dqkv, delta, q_prescaled=pre, dim_head=D)
    torch.cuda.synchronize()
    if guard:
        for name, view, whole in (("lse", lse, lse_w), ("dqkv", dqkv, dqkv_w), ("delta", delta, delta_w)):
            assert bool((whole[view.numel():] == SENTINEL).all()), f"{what}: wrote past {name}"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dqkv.float()).all()), what + ": an element was never written"
    w = assert_elementwise(out, c["ref"], c["bound"], what + " out", tile=(64, D))
    e_lse = (lse.double().cpu() - c["lse"]).abs().max().item()
    r_lse = rel(lse, c["lse"])
    got = dqkv.float().cpu().view(B, N, 3, H * D).unbind(2)
    model = attn_model(c["qref"], c["do64"], B, N, H, D, c["scale"], dt, out=out, lse=lse)
    names = ("dq", "dk", "dv")
    if N == 1:
        # One key: P = 1, so dS = P (dP - delta) and with it dq and dk are exactly 0 in exact arithmetic, and the row metric has nothing to divide by.
        # The kernels form dP = dO . v on the matrix pipe and delta = dO . out in a chain of f32 multiply-adds; out = v here, so the two are f32 sums of
        # the SAME D products in two orders, each within gamma_D of the exact sum: |dS| <= 2 (2 D + 8) 2^-24 sum_d |dO_d| |v_d| (the constant of
        # util.elem_bound, once per sum), |dq_d| <= |dS| |k_d| scale, |dk_d| <= |dS| |q_d| scale, plus the rounding of the store.
        # dv = P^T dO with P = 1 after the 16-bit rounding: dv is dO, bit for bit — what the model gives too.
        q, k, v = c["qref"].view(B, N, 3, H * D).unbind(2)
        ds = (2 * (2 * D + 8) * 2.0 ** -24) * (c["do64"].double().abs() * v.abs()).view(B, N, H, D).sum(-1, keepdim=True).expand(B, N, H, D).reshape(B, N, H * D)
        for n, t, other in (("dq", got[0], k), ("dk", got[1], q)):
            assert_elementwise(t, torch.zeros_like(ds), ds * other.abs() * c["scale"] * (1 + 2.0 ** -8) + SUB16.get(dt, 0.0), f"{what} {n} (exactly 0 in exact arithmetic)")
        assert torch.equal(got[2].double(), c["do64"].double()) and torch.equal(model[4].double(), c["do64"].double()), f"{what} dv is not dO"
        names, got, model = (), (), model[:2]
    model_rows = [worst_rows(m, r_, H, D) for m, r_ in zip(model[2:], c["grads"])]
    assert all(m == m and m > 0 for m in model_rows), (what, model_rows)
    rows = [assert_rows_within(t, r_, H, D, ATT_MARGIN * m, f"{what} {n}") for n, t, r_, m in zip(names, got, c["grads"], model_rows)]
    ratios = [k / m for k, m in zip(rows, model_rows)]
    print(f"{what}: out max err / bound {w:.3f}, lse max abs {e_lse:.1e} rel {r_lse:.1e}, worst gradient row kernel / model "
          + " ".join(f"{n} {k:.2e} / {m:.2e} = {r_:.2f}" for n, k, m, r_ in zip(names, rows, model_rows, ratios)))
    assert r_lse <= 1e-5 and e_lse <= 1e-4, (what, r_lse, e_lse)
    assert not any(not (r_ <= ATT_MARGIN) for r_ in ratios), (what, ratios)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", SHAPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_every_element_and_row(C, D, B, N, H, pre, dt):
    _check(C, D, B, N, H, pre, dt)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", [(2, 40, 2), (2, 196, 3)])
@pytest.mark.parametrize("D", WIDTHS)
def test_reads_and_writes_nothing_outside_its_tensors(C, D, B, N, H, pre, dt):
    """qkv, out and dout at the front of larger allocations: NaN bit patterns in the 64 rows behind the inputs, a finite sentinel behind out / lse / delta /
    dqkv.  The results still meet the bounds (no over-read value reached the arithmetic) and the sentinels keep their bits (no over-write)."""
    _check(C, D, B, N, H, pre, dt, guard=True)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("D", [128, 32])
def test_spiked_scores_in_the_masked_tile(C, D, pre):
    """N = 500: seven full tiles and 52 keys; the last step of the staircase is key 497, so the reference is raised inside the masked tile"""
    _check(C, D, 1, 500, 2, pre, BF16, spiked=True)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", [(2, 100, 2), (1, 192, 2)])
@pytest.mark.parametrize("D", WIDTHS)
def test_bit_reproducible_across_launches(C, D, B, N, H, pre):
    """five launches with unrelated work in between, identical bits (dQ and dK/dV are separate kernels without atomics)"""
    g = torch.Generator(device="cuda").manual_seed(D + B + N + H)
    qkv = (torch.randn(B, N, 3 * H * D, device="cuda", generator=g) * 1.2).to(BF16)
    do = torch.randn(B, N, H * D, device="cuda", generator=g).to(BF16)
    scale = D ** -0.5
    runs = []
    for rep in range(5):
        out = torch.full((B, N, H * D), float("nan"), dtype=BF16, device="cuda")
        lse = torch.full((B, H, N), float("nan"), device="cuda")
        dqkv = torch.full_like(qkv, float("nan")); delta = torch.full((B, H, N), float("nan"), device="cuda")
        if rep % 2:
            torch.empty(1 << 24, device="cuda").normal_()        # unrelated work between the launches (other cache / clock state)
        C.attention_forward(qkv, B, N, H, scale, out, lse, q_prescaled=pre, dim_head=D)
        C.attention_backward(qkv, out, do, lse, B, N, H, scale, dqkv, delta, q_prescaled=pre, dim_head=D)
        torch.cuda.synchronize()
        runs.append((out, lse, dqkv, delta))
    for k, name in enumerate(("out", "lse", "dqkv", "delta")):
        it = torch.int16 if k in (0, 2) else torch.int32
        assert not bool(torch.isnan(runs[0][k]).any()), f"{name}: an element was never written"
        for r in runs[1:]:
            assert torch.equal(runs[0][k].view(it), r[k].view(it)), f"{name}: {(runs[0][k] != r[k]).sum().item()} elements differ between two launches on the same input"


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("N", [64, 48])
def test_width_64_through_the_new_entry_points_is_the_old_call(C, N, pre, dt):
    """D = 64 forwards to enh_attention_forward / enh_attention_backward (aligned kernels at N = 64, tail forms at N = 48): identical bits"""
    B, H, scale = 2, 2, 0.125
    g = torch.Generator(device="cuda").manual_seed(N)
    qkv = (torch.randn(B, N, 3 * H * 64, device="cuda", generator=g) * 1.2).to(dt)
    do = torch.randn(B, N, H * 64, device="cuda", generator=g).to(dt)
    L, p, s, d = C.lib(), C._p, C._stream(), C._dt(qkv)
    res = []
    for new in (False, True):
        out = torch.full((B, N, H * 64), float("nan"), dtype=dt, device="cuda")
        lse = torch.full((B, H, N), float("nan"), device="cuda")
        dqkv = torch.full_like(qkv, float("nan")); delta = torch.full((B, H, N), float("nan"), device="cuda")
        if new:
            assert L.enh_attention_forward_dh(p(qkv), B, N, H, 64, scale, int(pre), p(out), p(lse), d, s) == 0
            label = L.enh_last_kernel()
            assert L.enh_attention_backward_dh(p(qkv), p(out), p(do), p(lse), B, N, H, 64, scale, int(pre), p(dqkv), p(delta), d, s) == 0
        else:
            C.attention_forward(qkv, B, N, H, scale, out, lse, q_prescaled=pre)
            old_label = L.enh_last_kernel()
            C.attention_backward(qkv, out, do, lse, B, N, H, scale, dqkv, delta, q_prescaled=pre)
        torch.cuda.synchronize()
        res.append((out, lse, dqkv, delta))
    assert label == old_label and b"attn_dh" not in label, (label, old_label)
    for k, name in enumerate(("out", "lse", "dqkv", "delta")):
        it = torch.int16 if k in (0, 2) else torch.int32
        assert not bool(torch.isnan(res[0][k]).any()), name
        assert torch.equal(res[0][k].view(it), res[1][k].view(it)), name
    # the keyword of the binding takes the same road
    out = torch.full((B, N, H * 64), float("nan"), dtype=dt, device="cuda"); lse = torch.empty(B, H, N, device="cuda")
    C.attention_forward(qkv, B, N, H, scale, out, lse, q_prescaled=pre, dim_head=64)
    assert torch.equal(out.view(torch.int16), res[0][0].view(torch.int16))


@pytest.mark.parametrize("D", [80, 0, 256])
def test_an_unsupported_width_is_the_librarys_shape_error(C, D):
    """no launch, no fault: every output keeps its prefill"""
    B, N, H = 1, 64, 1
    w = max(D, 16)
    qkv = torch.zeros(B, N, 3 * H * w, dtype=BF16, device="cuda"); do = torch.zeros(B, N, H * w, dtype=BF16, device="cuda")
    out = torch.full((B, N, H * w), 7.0, dtype=BF16, device="cuda"); lse = torch.full((B, H, N), 7.0, device="cuda")
    dqkv = torch.full_like(qkv, 7.0); delta = torch.full((B, H, N), 7.0, device="cuda")
    L, p, s = C.lib(), C._p, C._stream()
    E_SHAPE = -2      # include/enh_hip.h ENH_E_SHAPE
    assert L.enh_attention_forward_dh(p(qkv), B, N, H, D, 0.125, 0, p(out), p(lse), 0, s) == E_SHAPE
    assert b"dim_head must be 32, 64, 96 or 128" in L.enh_last_error()
    assert L.enh_attention_backward_dh(p(qkv), p(out), p(do), p(lse), B, N, H, D, 0.125, 0, p(dqkv), p(delta), 0, s) == E_SHAPE
    q32 = qkv.float(); o32 = out.float(); d32 = dqkv.float()
    assert L.enh_attention_forward_f32_dh(p(q32), B, N, H, D, 0.125, p(o32), p(lse), s) == E_SHAPE
    assert L.enh_attention_backward_f32_dh(p(q32), p(o32), p(do.float()), p(lse), B, N, H, D, 0.125, p(d32), p(delta), s) == E_SHAPE
    with pytest.raises(RuntimeError, match="dim_head must be 32, 64, 96 or 128"):
        C.attention_forward(qkv, B, N, H, 0.125, out, lse, dim_head=D)
    with pytest.raises(RuntimeError, match="dim_head must be 32, 64, 96 or 128"):
        C.attn_bwd(q32, o32, do.float(), lse, B, N, H, 0.125, d32, delta, dim_head=D)
    torch.cuda.synchronize()
    for t in (out, lse, dqkv, delta, o32, d32):
        assert bool((t == 7.0).all())


@pytest.mark.parametrize("dt,tag", [(BF16, "BF16"), (F16, "F16")])
def test_the_timing_label_is_a_kernel_symbol_of_the_library(C, dt, tag):
    """enh_last_kernel() after a D = 96 forward: the label KernelTimer records, and exactly one symbol of the built library (read as tests/test_isa_kernel_labels.py does)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_lint
    if not os.path.exists(isa_lint.LLVM + "/llvm-objdump"):
        pytest.skip("needs the ROCm llvm tools")
    B, N, H, D = 1, 40, 1, 96
    qkv = torch.randn(B, N, 3 * H * D, device="cuda").to(dt)
    out = torch.empty(B, N, H * D, dtype=dt, device="cuda"); lse = torch.empty(B, H, N, device="cuda")
    timer = C.KernelTimer()
    C.TIMER = timer
    try:
        C.attention_forward(qkv, B, N, H, D ** -0.5, out, lse, dim_head=D)
    finally:
        C.TIMER = None
    torch.cuda.synchronize()
    label = C.lib().enh_last_kernel().decode()
    assert label == f"attn_dh_fwd_kernel<96, {tag}>" and list(timer.records) == [label], (label, list(timer.records))
    hits = [n for n in isa_lint.kernel_stats() if n.startswith(label + "(") or n.startswith("void " + label + "(")]
    assert len(hits) == 1, (label, hits)


@pytest.mark.parametrize("B,N,H", SHAPES)
@pytest.mark.parametrize("D", WIDTHS)
def test_f32_kernels_against_fp64(C, D, B, N, H):
    """the exact-mode kernels (one thread per row, csrc/exact_f32.hip) at the new widths: out, lse and the three gradients within 1e-5"""
    c = _case(D, B, N, H, False, BF16)
    qkv, do = c["qref"].float().cuda(), c["do64"].float().cuda()
    nan = float("nan")
    out = torch.full((B, N, H * D), nan, device="cuda"); lse = torch.full((B, H, N), nan, device="cuda")
    dqkv = torch.full((B, N, 3 * H * D), nan, device="cuda"); delta = torch.full((B, H, N), nan, device="cuda")
    C.attn_fwd(qkv, B, N, H, c["scale"], out, lse, dim_head=D)
    C.attn_bwd(qkv, out, do, lse, B, N, H, c["scale"], dqkv, delta, dim_head=D)
    torch.cuda.synchronize()
    errs = dict(out=rel(out, c["ref"]), lse=rel(lse, c["lse"]))
    for n, t, r_ in zip(("dq", "dk", "dv"), dqkv.view(B, N, 3, H * D).unbind(2), c["grads"]):
        assert bool(torch.isfinite(t).all()), n
        errs[n] = rel(t, r_) if float(r_.abs().max()) > 0 else float(t.abs().max())      # (one token: dq = dk = 0 exactly, in the reference and here)
    print(f"f32 attention dim_head {D} B={B} N={N} H={H}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v <= 1e-5 for v in errs.values()), errs
