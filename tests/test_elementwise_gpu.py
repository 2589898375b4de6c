"""Every element and every row of the hot kernels against fp64, not only the norm of the whole tensor.

util.rel (one relative Frobenius error per tensor) is the right metric for "the arithmetic is at the rounding floor" and blind to errors that are large but
local — a tile's last row or column, the last K stage, a split-K slab boundary, the last key tile of an attention row
(tests/test_local_error_metric_cpu.py injects such faults and prints what today's limits let through).  Here:

  * GEMM, LayerNorm: util.elem_bound per element — one rounding of the stored format plus the worst-case f32 summation bound, from the operands alone
    (no measured constant but the tanh term, see util.TANH_ABS).  The printed max(err / bound) of an honest kernel is at most 1.
  * attention forward: util.attn_out_bound per element; lse within 1e-4 absolute (the limit tests/test_x3_gpu.py uses for the same v_log_f32 / v_exp_f32
    arithmetic).
  * attention gradients: the worst 64-wide row (util.row_err, per head) of dq, dk, dv against the worst row of util.attn_model — fp64 with the kernels'
    roundings, started from the stored out / lse that the backward kernels are given; the kernel gets 2 x the model's worst row (the families differ
    from the model in the order of their f32 sums and in the running maximum the probabilities are rounded under).  A halved row lands at 20 x, a
    zeroed one at 30 x (tests/test_local_error_metric_cpu.py).

Measured on MI355X (largest values over all cases; the honest kernels' max(err / bound) is at most 1 everywhere):
  GEMM 16-bit output 0.942 bf16 / 0.748 fp16, bias + tanh 0.861 / 0.499, tanh' 0.945 / 0.755, f32 modes 0.003; forward split-K 0.597 (16-bit) / 0.0002 (f32);
  weight-gradient split-K 0.00001; tanh' + column sums 0.972 / column sums 0.0001; LayerNorm y16 0.996, dx16 0.946;
  attention forward 0.831 of the element bound, lse 3.2e-5 absolute (spiked rows; 1.5e-6 on random scores);
  attention gradients, worst row kernel / model: 1.00 in every family, convention, format and shape, the spiked rows included (limit 2).  That figure
  means one thing only: the worst row is dominated by the delta term, which kernel and model share once they start from the same out; an error of the
  kernels' own in a row is seen once it exceeds about twice that shared term (a halved or unwritten row is far beyond it).
  With the model's OWN forward in place of the stored out / lse the same ratios spread over 0.94 .. 2.08 (2.08: fp16, N = 1024, pre-scaled q, dq) although
  every element of out is within its bound: the worst gradient row is the row with the largest P K, it carries the 64 roundings of ITS out row through
  delta = rowsum(dO o out) coherently into every dS of the row, and kernel / model is then the ratio of two independent draws of that one sum.  Given
  the same out, model and kernels agree on the worst row to three digits.
"""
import os

import pytest
import torch

from util import TANH_ABS, assert_elementwise, assert_rows_within, attn_model, attn_out_bound, attn_ref64, elem_bound, h16r, rel, worst_rows

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _mm64(a, b):
    """fp64 product of two CPU tensors, taken by torch on the device (plain torch.matmul in fp64: not the code under test)"""
    return (a.double().cuda() @ b.double().cuda()).cpu()


# ---------------------------------------------------------------------------------------------
# GEMM: every family, layout, format and fused mode
# ---------------------------------------------------------------------------------------------
# the smallest shapes at which each code path still exists:
#   (1000, 200, 328) ragged against 128- and 256-row tiles, 8-column granularity, a partial 64-deep K stage: the register-staged kernel whatever is asked for
#   (1024, 768, 384) whole 256 x 256 tiles and 6 K stages: pipe2, w256, w256p, and w256r (which needs an even stage count >= 6)
#   (768, 512, 448)  7 stages: w256p only
GEMM_SHAPES = [(1000, 200, 328), (1024, 768, 384), (768, 512, 448)]
# (name, epi_mode as include/enh_hip.h enh_gemm_h16_variant_mode counts them; the position table and accumulate take the generic epilogue)
GEMM_MODES = [("h16", 1), ("f32", 5), ("bias_tanh", 2), ("dtanh", 3), ("bias_res", 4), ("bias_pos", 0), ("accumulate", 0)]
_GEMM_CACHE = {}


def _gemm_case(M, N, K, dt, seed=11):
    """operands (values representable in dt), the epilogues' inputs, and the fp64 product and magnitude — computed once per (shape, format)"""
    key = (M, N, K, dt, seed)
    if key not in _GEMM_CACHE:
        g = torch.Generator().manual_seed(seed + M + N + K)
        c = dict(A=h16r(torch.randn(M, K, generator=g) * 0.5, dt), B=h16r(torch.randn(N, K, generator=g) * 0.1, dt), bias=torch.randn(N, generator=g),
                 res=torch.randn(M, N, generator=g), pos=torch.randn(256, N, generator=g), h=h16r(torch.tanh(torch.randn(M, N, generator=g)), dt))
        c["base"] = _mm64(c["A"], c["B"].t())
        c["mag"] = _mm64(c["A"].abs(), c["B"].abs().t())
        c["dev"] = {}
        _GEMM_CACHE[key] = c
    return _GEMM_CACHE[key]


def _dev(c, name, dt=None, t=False):
    key = (name, dt, t)
    if key not in c["dev"]:
        x = c[name].t().contiguous() if t else c[name]
        c["dev"][key] = (x.to(dt) if dt is not None else x).cuda()
    return c["dev"][key]


def _expected_kernel(fam, ta, M, N, K, mode):
    """the kernel the planner of csrc/gemm.hip launches for a forced family (what this test INTENDS to reach with it).  This is a second statement of
    gemm_plan / gemm_persistent / gemm_regstaged: a change of the planner's rules has to be made here as well."""
    if K % 64:
        return "gemm_kernel"
    if fam in (0, 3):
        return "gemm_kernel" if fam == 0 else "gemm_pipe2_kernel"
    if M % 256 or N % 256:
        return "gemm_pipe2_kernel"
    nst = K // 64
    if fam == 7 or ta or nst < 3 or mode not in (1, 2, 3, 4, 5):
        return "gemm_w256_kernel"
    return "gemm_w256r_kernel" if fam == 9 and mode in (1, 2, 5) and nst % 2 == 0 and nst >= 6 else "gemm_w256p_kernel"


def _gemm_modes(C, c, M, N, K, dt, ta, tb, ld=None):
    """launch every fused mode; yields (name, output [M, N...], fp64 reference, element bound)"""
    a, b = _dev(c, "A", dt, ta), _dev(c, "B", dt, tb)
    bias, base, mag = _dev(c, "bias"), c["base"], c["mag"]
    kw = dict(trans_a=ta, trans_b=tb)
    W = N if ld is None else ld

    def buf(dtype, src=None):
        t = torch.full((M, W), 5.0, dtype=dtype, device="cuda")
        if src is not None:
            t[:, :N] = src.cuda()
        return t

    o = buf(dt); C.gemm(a, b, M, N, K, out_bf16=o, **kw)
    yield "h16", o, base, elem_bound(base, mag, K, dt)
    o = buf(torch.float32); C.gemm(a, b, M, N, K, out_f32=o, **kw)
    yield "f32", o, base, elem_bound(base, mag, K)
    ref = torch.tanh(base + c["bias"].double())
    o = buf(dt); C.gemm(a, b, M, N, K, bias=bias, act=C.ACT_TANH, out_bf16=o, **kw)
    yield "bias_tanh", o, ref, elem_bound(ref, (mag + c["bias"].double().abs()) * (1 - ref ** 2), K, dt, extra_abs=TANH_ABS)
    d = 1 - c["h"].double() ** 2
    o = buf(dt); C.gemm(a, b, M, N, K, act=C.ACT_DTANH, aux=buf(dt, c["h"]), out_bf16=o, **kw)
    yield "dtanh", o, base * d, elem_bound(base * d, mag * d.abs(), K, dt)
    ref = base + c["bias"].double() + c["res"].double()
    o = buf(torch.float32, c["res"]); C.gemm(a, b, M, N, K, bias=bias, res=o, res_rows=M, out_f32=o, **kw)          # in place on the residual stream
    yield "bias_res", o, ref, elem_bound(ref, mag + c["bias"].double().abs() + c["res"].double().abs(), K)
    pos = c["pos"].double()[torch.arange(M) % 256]
    ref = base + c["bias"].double() + pos
    o = buf(torch.float32); C.gemm(a, b, M, N, K, bias=bias, res=_dev(c, "pos"), res_rows=256, out_f32=o, **kw)
    yield "bias_pos", o, ref, elem_bound(ref, mag + c["bias"].double().abs() + pos.abs(), K)
    o = buf(torch.float32, c["res"]); C.gemm(a, b, M, N, K, accumulate=True, out_f32=o, **kw)
    yield "accumulate", o, base + c["res"].double(), elem_bound(base, mag + c["res"].double().abs(), K)


def _check_gemm(C, fam, dyn, M, N, K, dt, ta, tb):
    L = C.lib()
    c = _gemm_case(M, N, K, dt)
    worst = {}
    try:
        assert L.enh_gemm_set_kernel(fam) == 0 and L.enh_gemm_set_scheduler(dyn) == 0
        if not os.environ.get("ENH_GEMM_KERNEL"):
            for name, mode in GEMM_MODES:
                want = _expected_kernel(fam, ta, M, N, K, mode)
                assert L.enh_gemm_h16_variant_mode(int(ta), int(tb), M, N, K, mode).decode() == want, (name, want)
        modes = dict(GEMM_MODES)
        for name, out, ref, bound in _gemm_modes(C, c, M, N, K, dt, ta, tb):
            tile = (256, 256) if "w256" in _expected_kernel(fam, ta, M, N, K, modes[name]) else (128, 128)       # (for the failure message)
            worst[name] = assert_elementwise(out, ref, bound, f"family {fam} dyn {dyn} {M}x{N}x{K} ta={ta} tb={tb} {dt} {name}", tile=tile)
    finally:
        L.enh_gemm_set_kernel(-1)
        L.enh_gemm_set_scheduler(1)
    print(f"gemm family {fam} dyn {dyn} {M}x{N}x{K} ta={int(ta)} tb={int(tb)} {dt}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@DTS
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("fam", [0, 3, 7])
def test_gemm_every_element(C, fam, M, N, K, ta, tb, dt):
    """families 0 (register-staged), 3 (pipe2) and 7 (w256, one tile per workgroup) in all four operand layouts; a family that cannot serve a shape
    hands it to the one that does (1000 x 200 x 328: the register-staged kernel under every name, the per-shape choice included)"""
    _check_gemm(C, fam, 1, M, N, K, dt, ta, tb)


@DTS
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("M,N,K,dyn", [s + (1,) for s in GEMM_SHAPES] + [(1024, 768, 384, 0)])       # (12 tiles: the one shape with a tile queue per XCD to claim from)
@pytest.mark.parametrize("fam", [8, 9])
def test_persistent_gemm_every_element(C, fam, M, N, K, dyn, tb, dt):
    """the persistent kernels w256p / w256r against fp64 themselves (tests/test_ops_gpu.py holds them to w256 bit for bit — and w256 shares its K loop
    with them, so an error in the shared loop is identical in all three), under both tile schedules"""
    _check_gemm(C, fam, dyn, M, N, K, dt, False, tb)


def test_gemm_default_choice_every_element(C):
    """the per-shape choice (family -1) on the ragged shape, the one the forced families above hand over to"""
    for dt in (BF16, F16):
        _check_gemm_default(C, 1000, 200, 328, dt)


def _check_gemm_default(C, M, N, K, dt):
    c = _gemm_case(M, N, K, dt)
    assert C.lib().enh_gemm_set_kernel(-1) == 0
    for ta, tb in ((False, False), (False, True), (True, False), (True, True)):
        worst = {name: assert_elementwise(out, ref, bound, f"default {M}x{N}x{K} ta={ta} tb={tb} {dt} {name}", tile=(128, 128))
                 for name, out, ref, bound in _gemm_modes(C, c, M, N, K, dt, ta, tb)}
        print(f"gemm default {M}x{N}x{K} ta={int(ta)} tb={int(tb)} {dt}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("fam", [0, 3, 7, 8, 9])
def test_gemm_row_strides_every_element(C, fam):
    """ldc / ldaux / ldres wider than N (output, saved tanh output and residual stream living in wider buffers): the same bounds, and the columns
    beyond N untouched"""
    L = C.lib()
    M, N, K, LD = 1024, 768, 384, 1024
    c = _gemm_case(M, N, K, BF16)
    try:
        assert L.enh_gemm_set_kernel(fam) == 0
        for tb in (False, True):
            for name, out, ref, bound in _gemm_modes(C, c, M, N, K, BF16, False, tb, ld=LD):
                assert out.shape == (M, LD) and bool((out[:, N:] == 5.0).all()), f"family {fam} tb={tb} {name}: columns beyond N were written"
                assert_elementwise(out[:, :N], ref, bound, f"family {fam} tb={tb} ld={LD} {name}", tile=(256, 256) if fam >= 7 else (128, 128))
    finally:
        L.enh_gemm_set_kernel(-1)


@DTS
def test_forward_split_k_every_element(C, dt):
    """the forward kind of split-K (f32 slabs + the fixed-order second pass that carries bias / residual / position table / accumulate / the 16-bit pack):
    k = K whatever the slab boundaries"""
    M, N, K = 1024, 768, 2304
    assert C.lib().enh_gemm_h16_workspace_bytes(0, 1, M, N, K) > 0
    c = _gemm_case(M, N, K, dt)
    a, b, bias = _dev(c, "A", dt), _dev(c, "B", dt, True), _dev(c, "bias")
    base, mag, bb, rr = c["base"], c["mag"], c["bias"].double(), c["res"].double()
    pos = c["pos"].double().repeat(M // 256, 1)
    worst = {}

    def check(name, out, ref, bound):
        worst[name] = assert_elementwise(out, ref, bound, f"forward split-K {dt} {name}", tile=(128, 128))
    o = torch.empty(M, N, device="cuda"); C.gemm(a, b, M, N, K, trans_b=True, out_f32=o)
    check("f32", o, base, elem_bound(base, mag, K))
    x = c["res"].clone().cuda(); C.gemm(a, b, M, N, K, trans_b=True, bias=bias, res=x, res_rows=M, out_f32=x)
    check("bias_res", x, base + bb + rr, elem_bound(base, mag + bb.abs() + rr.abs(), K))
    o = torch.empty(M, N, device="cuda"); C.gemm(a, b, M, N, K, trans_b=True, bias=bias, res=_dev(c, "pos"), res_rows=256, out_f32=o)
    check("bias_pos", o, base + bb + pos, elem_bound(base, mag + bb.abs() + pos.abs(), K))
    acc = c["res"].clone().cuda(); C.gemm(a, b, M, N, K, trans_b=True, bias=bias, accumulate=True, out_f32=acc)
    check("bias_accumulate", acc, base + bb + rr, elem_bound(base, mag + bb.abs() + rr.abs(), K))
    o16 = torch.empty(M, N, dtype=dt, device="cuda"); C.gemm(a, b, M, N, K, trans_b=True, out_bf16=o16)
    check("h16", o16, base, elem_bound(base, mag, K, dt))
    print(f"forward split-K {M}x{N}x{K} {dt}: max err / bound " + " ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("tokens,n_out,k_in,form", [(8192, 256, 192, "atomic"), (8192, 256, 192, "two_pass"), (16384, 768, 768, "two_pass")])
def test_wgrad_split_k_every_element(C, tokens, n_out, k_in, form):
    """dW += dY^T X over many tokens, K split over the grid: f32 atomics in any order (no workspace given) and partial slabs with a fixed-order second pass —
    the f32 bound with k = tokens holds for either"""
    L = C.lib()
    g = torch.Generator().manual_seed(9)
    dY, X = h16r(torch.randn(tokens, n_out, generator=g) * 0.1, BF16), h16r(torch.randn(tokens, k_in, generator=g), BF16)
    old = torch.randn(n_out, k_in, generator=g)
    ref = _mm64(dY.t(), X) + old.double()
    bound = elem_bound(ref, _mm64(dY.abs().t(), X.abs()) + old.double().abs(), tokens)
    a, b, dW = dY.to(BF16).cuda(), X.to(BF16).cuda(), old.clone().cuda()
    assert L.enh_gemm_h16_workspace_bytes(1, 1, n_out, k_in, tokens) > 0          # the shape IS split
    if form == "two_pass":
        C.gemm(a, b, n_out, k_in, tokens, trans_a=True, trans_b=True, accumulate=True, out_f32=dW)
    else:
        C._check(L.enh_gemm_h16(C._p(a), n_out, 1, C._p(b), k_in, 1, n_out, k_in, tokens, None, C.ACT_NONE, None, 0, None, 0, 0, 1, C._p(dW), None, k_in,
                                C.DT_BF16, C._stream()), "enh_gemm_h16")
    w = assert_elementwise(dW, ref, bound, f"weight-gradient split-K {form} tokens={tokens} {n_out}x{k_in}", tile=(256, 256))
    print(f"weight-gradient split-K {form} tokens={tokens} {n_out}x{k_in}: max err / bound {w:.5f}")


@DTS
@pytest.mark.parametrize("M,N,K,fam", [(2048, 768, 192, -1), (2048, 768, 192, 9), (1000, 192, 256, -1)])
def test_dtanh_colsum_every_element(C, M, N, K, fam, dt):
    """enh_gemm_h16_dtanh_colsum in the two-call form (the per-shape choice at these sizes) and fused into the persistent kernel's epilogue (family 9):
    the output within the element bound, the column sums within the f32 bound (k = M) of the fp64 sum of the STORED values"""
    L = C.lib()
    c = _gemm_case(M, N, K, dt)
    a, b, h = _dev(c, "A", dt), _dev(c, "B", dt, True), _dev(c, "h", dt)
    old = _dev(c, "bias")
    d = 1 - c["h"].double() ** 2
    try:
        assert L.enh_gemm_set_kernel(fam) == 0
        if fam == 9 and not os.environ.get("ENH_GEMM_KERNEL"):
            assert L.enh_gemm_h16_variant_mode(0, 1, M, N, K, 3).decode() == "gemm_w256p_kernel"
            assert L.enh_gemm_h16_dtanh_colsum_workspace_bytes(1, M, N, K) == (M // 128) * N * 4        # the fused form's partial rows
        for accumulate in (False, True):
            out = torch.empty(M, N, dtype=dt, device="cuda")
            cs = old.clone()
            C.gemm_dtanh_colsum(a, b, M, N, K, h, out, cs, trans_b=True, accumulate_colsum=accumulate)
            w = assert_elementwise(out, c["base"] * d, elem_bound(c["base"] * d, c["mag"] * d.abs(), K, dt), f"dtanh_colsum family {fam} {dt} output", tile=(256, 256))
            stored = out.double().cpu()
            want = stored.sum(0) + (c["bias"].double() if accumulate else 0.0)
            ws = assert_elementwise(cs, want, elem_bound(want, stored.abs().sum(0) + (c["bias"].double().abs() if accumulate else 0.0), M), f"dtanh_colsum family {fam} {dt} column sums")
            print(f"dtanh_colsum {M}x{N}x{K} family {fam} {dt} accumulate={accumulate}: max err / bound output {w:.3f}, column sums {ws:.4f}")
    finally:
        L.enh_gemm_set_kernel(-1)


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
ATT_FAMILIES = [(0, 0, 0), (1, 1, 1), (1, 3, 2), (5, 1, 2), (5, 3, 1)]          # as tests/test_ops_gpu.py
ATT_SHAPES = [(2, 192, 2), (1, 320, 1), (1, 1024, 2)]                           # three, five and sixteen key tiles (odd counts for the two-slot prefetch)
ATT_MARGIN = 2.0
_ATT_CACHE = {}


def _spiked_qkv(g, B, N, H):
    """tests/test_ops_gpu.py _spiked_qkv: keys dominating a row — key 300 of head 0 aligned with query 5, a staircase for query 70 of head 1 (keys in tiles
    1, 2, 3 and the last tile, each beating everything before it): the rows that take the rescale branch"""
    qkv = torch.randn(B, N, 3 * H * 64, generator=g)
    qkv[0, 5, :64] *= 6.0
    qkv[0, 300, H * 64:H * 64 + 64] = qkv[0, 5, :64] * 1.5
    qv = qkv[0, 70, 64:128].clone()
    for key, gain in ((100, 2.0), (130, 4.0), (200, 7.0), (505, 11.0)):
        qkv[0, key, H * 64 + 64:H * 64 + 128] = qv * gain
    return qkv


def _att_case(B, N, H, pre, dt, spiked=False):
    """inputs and the fp64 reference — once per (shape, convention, format)"""
    key = (B, N, H, pre, dt, spiked)
    if key not in _ATT_CACHE:
        scale = 0.125
        g = torch.Generator().manual_seed(0 if spiked else B * 100 + N + H)
        qkv = h16r(_spiked_qkv(g, B, N, H) if spiked else torch.randn(B, N, 3 * H * 64, generator=g) * 1.5, dt)
        do = h16r(torch.randn(B, N, H * 64, generator=g), dt)
        qdev, qref = qkv, qkv.double()
        if pre:       # include/enh_hip.h q_prescaled: the q third holds dt(q * scale * log2e); the reference is taken on the UNSCALED values those bits represent
            qdev = qkv.clone()
            qdev[..., :H * 64] = h16r(qkv[..., :H * 64] * (scale * LOG2E), dt)
            qref = qdev.double().clone()
            qref[..., :H * 64] /= (scale * LOG2E)
        ref, lse_ref, pav, grads = attn_ref64(qref, do, B, N, H, scale)
        _ATT_CACHE[key] = dict(scale=scale, qref=qref, do64=do, qd=qdev.to(dt).cuda(), do=do.to(dt).cuda(), ref=ref, lse=lse_ref, bound=attn_out_bound(ref, pav, dt),
                               grads=grads, own_rows=[worst_rows(m, r_, H) for m, r_ in zip(attn_model(qref, do, B, N, H, scale, dt)[2:], grads)])
    return _ATT_CACHE[key]


def _check_attention(C, fam, B, N, H, pre, dt, spiked=False):
    c = _att_case(B, N, H, pre, dt, spiked)
    what = f"attention family {fam} {'spiked ' if spiked else ''}B={B} N={N} H={H} {'prescaled' if pre else 'plain'} {dt}"
    try:
        C.attention_set_kernel(*fam)
        out = torch.full((B, N, H * 64), float("nan"), dtype=dt, device="cuda")
        lse = torch.full((B, H, N), float("nan"), device="cuda")
        C.attention_forward(c["qd"], B, N, H, c["scale"], out, lse, q_prescaled=pre)
        dqkv = torch.full((B, N, 3 * H * 64), float("nan"), dtype=dt, device="cuda")
        delta = torch.empty(B, H, N, device="cuda")
        C.attention_backward(c["qd"], out, c["do"], lse, B, N, H, c["scale"], dqkv, delta, q_prescaled=pre)
        torch.cuda.synchronize()
    finally:
        C.attention_set_kernel(0, 0, 0)
    w = assert_elementwise(out, c["ref"], c["bound"], what + " out", tile=(64, 64))
    e_lse = (lse.double().cpu() - c["lse"]).abs().max().item()
    got = dqkv.float().cpu().view(B, N, 3, H * 64).unbind(2)
    # the model of the backward starts from what the backward kernels are given: the STORED out (delta = rowsum(dO o out)) and lse of this forward, both
    # held to fp64 above.  (With the model's own forward in their place the worst row — the row with the largest P K, the same one in every format — carries
    # another draw of the 64 roundings of its out row through delta, and kernel / model is the ratio of two such draws: printed below, not asserted.)
    model = attn_model(c["qref"], c["do64"], B, N, H, c["scale"], dt, out=out, lse=lse)
    model_rows = [worst_rows(m, r_, H) for m, r_ in zip(model[2:], c["grads"])]
    assert all(m == m and m > 0 for m in model_rows), (what, model_rows)
    # every row of every head finite (dqkv was filled with NaN: a row the kernels never wrote shows here) and within ATT_MARGIN x the model's worst row
    rows = [assert_rows_within(t, r_, H, ATT_MARGIN * m, f"{what} {n}") for n, t, r_, m in zip(("dq", "dk", "dv"), got, c["grads"], model_rows)]
    ratios = [k / m for k, m in zip(rows, model_rows)]
    own = [k / m for k, m in zip(rows, c["own_rows"])]
    print(f"{what}: out max err / bound {w:.3f}, lse max abs {e_lse:.1e}, worst gradient row kernel / model "
          + " ".join(f"{n} {k:.2e} / {m:.2e} = {r_:.2f}" for n, k, m, r_ in zip(("dq", "dk", "dv"), rows, model_rows, ratios))
          + " (against the model's own forward, not asserted: " + " ".join(f"{r_:.2f}" for r_ in own) + ")")
    assert rel(lse, c["lse"]) <= 1e-5 and e_lse <= 1e-4, (what, rel(lse, c["lse"]), e_lse)
    assert not any(not (r_ <= ATT_MARGIN) for r_ in ratios), (what, ratios)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", ATT_SHAPES)
@pytest.mark.parametrize("fam", ATT_FAMILIES, ids=lambda f: "fam%d%d%d" % f)
def test_attention_every_element_and_row(C, fam, B, N, H, pre):
    _check_attention(C, fam, B, N, H, pre, BF16)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("B,N,H", ATT_SHAPES)
def test_attention_every_element_and_row_fp16(C, B, N, H, pre):
    _check_attention(C, (0, 0, 0), B, N, H, pre, F16)


@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("fam", ATT_FAMILIES, ids=lambda f: "fam%d%d%d" % f)
def test_attention_spiked_scores_every_element_and_row(C, fam, pre):
    """the rows that take the rescale branch (a wrong rescale order is silent on bounded random data), element by element and row by row"""
    _check_attention(C, fam, 1, 512, 2, pre, BF16, spiked=True)


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("M,D", [(130, 1280), (33, 2048)])
def test_layernorm_every_element(C, M, D, dt):
    """y16 = one rounding of w x^ + b: u |y| + 8 * 2^-24 (|w| |x^| + |b|); dx16 against the fp64 autograd of the same inputs: u |ref| plus the f32 bound
    with k = D on the magnitudes of the terms of dx = rstd (w dy - mean(w dy) - x^ mean(w dy x^)) + dres"""
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    w = 1 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    dy = h16r(torch.randn(M, D, generator=g), dt)
    dres = torch.randn(M, D, generator=g)
    xt = x.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xt, (D,), w.double(), b.double(), 1e-5)
    y.backward(dy.double())
    y, dx_ref = y.detach(), xt.grad + dres.double()
    rstd64 = (x.double().var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    xhat = (x.double() - x.double().mean(1, keepdim=True)) * rstd64
    wdy = w.double() * dy.double()
    mag_dx = rstd64 * (wdy.abs() + wdy.abs().mean(1, keepdim=True) + xhat.abs() * (wdy * xhat).abs().mean(1, keepdim=True)) + dres.double().abs()
    xd = x.cuda()
    y16 = torch.empty(M, D, dtype=dt, device="cuda"); y32 = torch.empty(M, D, device="cuda")
    mean = torch.empty(M, device="cuda"); rstd = torch.empty(M, device="cuda")
    C.layernorm_forward(xd, w.cuda(), b.cuda(), 1e-5, y16, y32, mean, rstd)
    wy = assert_elementwise(y16, y, elem_bound(y, w.double().abs() * xhat.abs() + b.double().abs(), 0, dt), f"layernorm {M}x{D} {dt} y16")
    dx = torch.empty(M, D, device="cuda"); dx16 = torch.empty(M, D, dtype=dt, device="cuda")
    dw = torch.zeros(D, device="cuda"); db = torch.zeros(D, device="cuda"); dxs = torch.zeros(D, device="cuda")
    C.layernorm_backward(dy.to(dt).cuda(), xd, w.cuda(), mean, rstd, dres.cuda(), dx, dx16, dw, db, dxs)
    wx = assert_elementwise(dx16, dx_ref, elem_bound(dx_ref, mag_dx, D, dt), f"layernorm {M}x{D} {dt} dx16")
    print(f"layernorm {M}x{D} {dt}: max err / bound y16 {wy:.3f}, dx16 {wx:.3f}")
