"""Timing labels are the kernels that ran: KernelTimer takes the label of a GEMM / attention-forward call from the library (enh_last_kernel(), which
composes it from the launch record that indexed the kernel tables), and this file pins, per call, the symbol a profiler reports for it.

Shapes are the smallest at which each choice of csrc/gemm.hip gemm_plan is taken on a 256-CU device:
  K = 72            no multiple of 64                                  -> the register-staged gemm_kernel
  128 x 128 x 128   no whole 256-tiles                                 -> gemm_pipe2_kernel
  3584 x 3584       14 x 14 = 196 tiles >= 3/4 of 256 CUs               -> the 256 x 256 family; its persistent form from 3 K stages (K = 192),
                    the A-in-registers form w256r at an even number >= 6 of K stages (K = 384) in the bf16 / bias + tanh / f32 / x3 split modes
  512 x 512, K = 32768 tokens, accumulate, workspace: 4 tiles x 64 K slices of 8 stages = one round of 256 workgroups -> gemm_w256_kernel, mode 6
  attention N = 64 / 48: the aligned kernels / the tail forms
If the device's CU budget makes a default choose otherwise, the case prints enh_gemm_h16_variant_mode for its shape and fails.

EXPECTED holds full symbols (template arguments, no parameter list).  The "default" entries are what the hand-written label code of the binding
printed for these calls before the library named its kernels; the entries marked (*) are calls that code labelled wrongly (it could not see
enh_gemm_set_kernel(8) in the split call, nor that fewer than 8 workgroups run the static schedule, nor a scheduler set behind its back) and are
read off csrc/gemm.hip.  tests/test_isa_kernel_labels.py checks every entry against the built library's symbol table.
Every GEMM result is also held to util.elem_bound against a.double() @ b.double().T, so a launch that did nothing cannot pass."""
import threading

import pytest
import torch

from util import TANH_ABS, assert_elementwise, attn_out_bound, attn_ref64, elem_bound, h16r

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
LOG2E = 1.4426950408889634
BIG = 3584

EXPECTED = {
    "fwd_k72": "gemm_kernel<F16, false, false>",
    "fwd_k128": "gemm_pipe2_kernel<F16, false, false>",
    "h16_k192": "gemm_w256p_kernel<F16, false, false, 1, true>",
    "h16_k384": "gemm_w256r_kernel<F16, false, 1, true>",
    "bias_tanh": "gemm_w256r_kernel<F16, false, 2, true>",
    "f32_bias_res": "gemm_w256p_kernel<F16, false, false, 4, true>",
    "bf16_trans_b": "gemm_w256r_kernel<BF16, true, 1, true>",
    "dtanh_colsum": "gemm_w256p_kernel<F16, false, true, 3, true>",
    "wgrad_ws": "gemm_w256_kernel<F16, true, true, 6>",
    "split2_k384": "gemm_w256r_kernel<BF16, false, 8, true>",
    "split2_k576": "gemm_w256p_kernel<BF16, false, false, 8, true>",
    "split3_tanh": "gemm_w256r_kernel<BF16, false, 9, true>",
    "attn_n64_pre_fp16": "attn_fwd_pre_kernel<F16>",
    "attn_n64_pre_bf16": "attn_fwd_pre_kernel<BF16>",
    "attn_n64_plain_fp16": "attn_fwd_kernel<F16>",
    "attn_n64_plain_bf16": "attn_fwd_kernel<BF16>",
    "attn_n48_pre_fp16": "attn_fwd_tail_pre_kernel<F16>",
    "attn_n48_pre_bf16": "attn_fwd_tail_pre_kernel<BF16>",
    "attn_n48_plain_fp16": "attn_fwd_tail_kernel<F16>",
    "attn_n48_plain_bf16": "attn_fwd_tail_kernel<BF16>",
    # (*) read off csrc/gemm.hip
    "w256p_forced_split2": "gemm_w256p_kernel<BF16, false, false, 8, true>",      # enh_gemm_set_kernel(8): no A-in-registers form, 64 workgroups
    "one_workgroup": "gemm_w256r_kernel<F16, false, 1, false>",                    # enh_gemm_set_kernel(9), one tile: fewer than 8 workgroups -> static
    "static_scheduler": "gemm_w256r_kernel<F16, false, 1, false>",                 # enh_gemm_set_scheduler(0)
}

_CACHE = {}


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _operands(M, N, K, dt, k_major=False):
    """seeded a [M][K], b [N][K] (k_major: both stored [K][.], the weight-gradient layout) on the device, with base = a b^T and mag = |a| |b|^T in
    fp64, once per shape and format"""
    key = (M, N, K, dt, k_major)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(M + N + K)
        a = (torch.randn(M, K, generator=g) * (0.1 if k_major else 1.0)).to(dt).cuda()
        b = torch.randn(N, K, generator=g).to(dt).cuda()
        base, mag = a.double() @ b.double().T, a.double().abs() @ b.double().abs().T
        if k_major:
            a, b = a.t().contiguous(), b.t().contiguous()
        _CACHE[key] = dict(a=a, b=b, base=base, mag=mag, bias=torch.randn(N, generator=g).cuda(), res=torch.randn(M, N, generator=g).cuda(),
                           h=torch.tanh(torch.randn(M, N, generator=g)).to(dt).cuda())
    return _CACHE[key]


def _label(C, case, call, variant=None):
    """runs `call` once under a fresh KernelTimer and holds the one label it recorded to EXPECTED[case]"""
    timer = C.KernelTimer()
    C.TIMER = timer
    try:
        call()
    finally:
        C.TIMER = None
    torch.cuda.synchronize()
    got = list(timer.records)
    if got != [EXPECTED[case]] and variant is not None:
        print(f"{case}: enh_gemm_h16_variant_mode{variant} = {C.lib().enh_gemm_h16_variant_mode(*variant).decode()}, {C.device_cus()} CUs, budget {C.get_cu_budget()}")
    assert got == [EXPECTED[case]], (case, got, EXPECTED[case])


def test_no_kernel_before_the_first_call_of_a_thread(C):
    got = []
    t = threading.Thread(target=lambda: got.append(C.lib().enh_last_kernel()))
    t.start(); t.join()
    assert got == [b""]


@pytest.mark.parametrize("case,K", [("fwd_k72", 72), ("fwd_k128", 128)])
def test_small_forward(C, case, K):
    c = _operands(128, 128, K, F16)
    out = torch.empty(128, 128, dtype=F16, device="cuda")
    _label(C, case, lambda: C.gemm(c["a"], c["b"], 128, 128, K, out_bf16=out), (0, 0, 128, 128, K, 1))
    assert_elementwise(out, c["base"], elem_bound(c["base"], c["mag"], K, F16), case)


@pytest.mark.parametrize("case,K,override", [("h16_k192", 192, None), ("h16_k384", 384, None), ("static_scheduler", 384, "static")])
def test_plain_16bit_output(C, case, K, override):
    M = N = BIG
    c = _operands(M, N, K, F16)
    out = torch.empty(M, N, dtype=F16, device="cuda")
    try:
        if override == "static":
            assert C.lib().enh_gemm_set_scheduler(0) == 0
        _label(C, case, lambda: C.gemm(c["a"], c["b"], M, N, K, out_bf16=out), (0, 0, M, N, K, 1))
    finally:
        C.lib().enh_gemm_set_scheduler(1)
    assert_elementwise(out, c["base"], elem_bound(c["base"], c["mag"], K, F16), case, tile=(256, 256))


def test_one_workgroup_runs_the_static_schedule(C):
    M = N = 256; K = 384
    c = _operands(M, N, K, F16)
    out = torch.empty(M, N, dtype=F16, device="cuda")
    try:
        assert C.lib().enh_gemm_set_kernel(9) == 0
        _label(C, "one_workgroup", lambda: C.gemm(c["a"], c["b"], M, N, K, out_bf16=out), (0, 0, M, N, K, 1))
    finally:
        C.lib().enh_gemm_set_kernel(-1)
    assert_elementwise(out, c["base"], elem_bound(c["base"], c["mag"], K, F16), "one_workgroup", tile=(256, 256))


def test_bias_tanh(C):
    M = N = BIG; K = 384
    c = _operands(M, N, K, F16)
    out = torch.empty(M, N, dtype=F16, device="cuda")
    _label(C, "bias_tanh", lambda: C.gemm(c["a"], c["b"], M, N, K, bias=c["bias"], act=C.ACT_TANH, out_bf16=out), (0, 0, M, N, K, 2))
    ref = torch.tanh(c["base"] + c["bias"].double())
    assert_elementwise(out, ref, elem_bound(ref, (c["mag"] + c["bias"].double().abs()) * (1 - ref ** 2), K, F16, extra_abs=TANH_ABS), "bias_tanh", tile=(256, 256))


def test_f32_bias_residual(C):
    M = N = BIG; K = 384
    c = _operands(M, N, K, F16)
    out = c["res"].clone()          # in place on the residual stream
    _label(C, "f32_bias_res", lambda: C.gemm(c["a"], c["b"], M, N, K, bias=c["bias"], res=out, res_rows=M, out_f32=out), (0, 0, M, N, K, 4))
    ref = c["base"] + c["bias"].double() + c["res"].double()
    assert_elementwise(out, ref, elem_bound(ref, c["mag"] + c["bias"].double().abs() + c["res"].double().abs(), K), "f32_bias_res", tile=(256, 256))


def test_bf16_trans_b(C):
    M = N = BIG; K = 384
    c = _operands(M, N, K, BF16)
    bt = c["b"].t().contiguous()          # B stored [K][N]
    out = torch.empty(M, N, dtype=BF16, device="cuda")
    _label(C, "bf16_trans_b", lambda: C.gemm(c["a"], bt, M, N, K, trans_b=True, out_bf16=out), (0, 1, M, N, K, 1))
    assert_elementwise(out, c["base"], elem_bound(c["base"], c["mag"], K, BF16), "bf16_trans_b", tile=(256, 256))


def test_dtanh_colsum(C):
    M = N = BIG; K = 384
    c = _operands(M, N, K, F16)
    bt = c["b"].t().contiguous()
    out = torch.empty(M, N, dtype=F16, device="cuda")
    cs = torch.zeros(N, device="cuda")
    _label(C, "dtanh_colsum", lambda: C.gemm_dtanh_colsum(c["a"], bt, M, N, K, c["h"], out, cs, trans_b=True, accumulate_colsum=False), (0, 1, M, N, K, 3))
    d = 1 - c["h"].double() ** 2
    assert_elementwise(out, c["base"] * d, elem_bound(c["base"] * d, c["mag"] * d.abs(), K, F16), "dtanh_colsum", tile=(256, 256))
    stored = out.double()
    assert_elementwise(cs, stored.sum(0), elem_bound(stored.sum(0), stored.abs().sum(0), M), "dtanh_colsum column sums")


def test_weight_gradient_with_workspace(C):
    M = N = 512; K = 32768          # K = tokens
    c = _operands(M, N, K, F16, k_major=True)
    assert C.lib().enh_gemm_h16_workspace_bytes(1, 1, M, N, K) > 0          # the shape IS split, and gemm() brings the workspace
    old = c["res"].clone()
    _label(C, "wgrad_ws", lambda: C.gemm(c["a"], c["b"], M, N, K, trans_a=True, trans_b=True, accumulate=True, out_f32=old), (1, 1, M, N, K, 6))
    ref = c["base"] + c["res"].double()
    assert_elementwise(old, ref, elem_bound(ref, c["mag"] + c["res"].double().abs(), K), "wgrad_ws", tile=(256, 256))


@pytest.mark.parametrize("case,M,K,family", [("split2_k384", BIG, 384, -1), ("split2_k576", BIG, 576, -1), ("w256p_forced_split2", 2048, 384, 8)])
def test_split2(C, case, M, K, family):
    N = M
    c = _operands(M, N, K, BF16)
    hi, lo = torch.empty(M, N, dtype=BF16, device="cuda"), torch.empty(M, N, dtype=BF16, device="cuda")
    try:
        assert C.lib().enh_gemm_set_kernel(family) == 0
        if not C.gemm_split_fused(M, N, K):
            print(f"{case}: enh_gemm_h16_variant_mode = {C.lib().enh_gemm_h16_variant_mode(0, 0, M, N, K, 1).decode()}, {C.device_cus()} CUs, budget {C.get_cu_budget()}")
        assert C.gemm_split_fused(M, N, K)
        _label(C, case, lambda: C.gemm_split2(c["a"], c["b"], M, N, K, hi, lo))
    finally:
        C.lib().enh_gemm_set_kernel(-1)
    assert_elementwise(hi, c["base"], elem_bound(c["base"], c["mag"], K, BF16), case + " hi", tile=(256, 256))
    # lo = bf16(v - hi) of the f32 sum v (v - hi is exact in f32): |v - hi| <= 2^-8 |v|, rounded once more -> hi + lo is within 2^-16 |v| of v, and v
    # within the f32 bound b32 of the exact product (|v| <= |base| + b32)
    b32 = elem_bound(c["base"], c["mag"], K)
    assert_elementwise(hi.double() + lo.double(), c["base"], b32 + 2.0 ** -16 * (c["base"].abs().cpu() + b32), case + " hi + lo", tile=(256, 256))


def test_split3_tanh(C):
    M = N = BIG; K = 384
    c = _operands(M, N, K, BF16)
    y3 = torch.empty(M, 3 * N, dtype=BF16, device="cuda")
    _label(C, "split3_tanh", lambda: C.gemm_split3_tanh(c["a"], c["b"], M, N, K, c["bias"], y3))
    ref = torch.tanh(c["base"] + c["bias"].double())
    bound = elem_bound(ref, (c["mag"] + c["bias"].double().abs()) * (1 - ref ** 2), K, BF16, extra_abs=TANH_ABS)
    assert_elementwise(y3[:, :N], ref, bound, "split3_tanh hi", tile=(256, 256))
    assert bool((y3[:, 2 * N:] == y3[:, :N]).all()), "split3_tanh: the row is [hi | lo | hi]"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("pre", [True, False], ids=["pre", "plain"])
@pytest.mark.parametrize("N", [64, 48])
def test_attention_forward(C, N, pre, dt):
    B = H = 1
    scale = 0.125
    g = torch.Generator().manual_seed(N)
    qkv = h16r(torch.randn(B, N, 3 * 64, generator=g) * 1.5, dt)
    qdev, qref = qkv, qkv.double()
    if pre:       # the q third holds dt(q * scale * log2e); the reference is taken on the unscaled values those bits represent
        qdev = qkv.clone()
        qdev[..., :64] = h16r(qkv[..., :64] * (scale * LOG2E), dt)
        qref = qdev.double().clone()
        qref[..., :64] /= (scale * LOG2E)
    ref, _, pav, _ = attn_ref64(qref, torch.zeros(B, N, 64), B, N, H, scale)
    qd = qdev.to(dt).cuda()
    out = torch.full((B, N, 64), float("nan"), dtype=dt, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    case = f"attn_n{N}_{'pre' if pre else 'plain'}_{'fp16' if dt == F16 else 'bf16'}"
    _label(C, case, lambda: C.attention_forward(qd, B, N, H, scale, out, lse, q_prescaled=pre))
    assert_elementwise(out, ref, attn_out_bound(ref, pav, dt), case)
