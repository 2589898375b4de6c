"""The MXFP8 weight kernels (csrc/gpt_decode_w8.hip).  The quantizer is held to tests/mxfp8_util.py bit for bit; the product to an fp64 product of
x and the exactly dequantized weight, under tests/util.py's element bound.  That bound is worked out from the number formats and carries over from
the 16-bit product as it stands: a dequantized weight has 4 significant bits and x has 11 or 8, so every product is exact in f32 and what remains is
the f32 sum of K terms and the one rounding of the store.  Nothing here is a measured tolerance."""
import math

import pytest
import torch

from mxfp8_util import dequant, quant
from util import U16, assert_elementwise, elem_bound

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
E24 = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _e4m3(v: float) -> int:
    return int(torch.tensor(v).to(torch.float8_e4m3fn).view(torch.uint8).item())


# ---------------------------------------------------------------------------------------------
# quantizer
# ---------------------------------------------------------------------------------------------
def _crafted(N, K, seed):
    """randn / sqrt(K) with the edge-case blocks written over it, as many as the shape holds"""
    w = torch.randn(N, K, generator=_gen(seed)) / math.sqrt(K)
    blocks = w.view(-1, 32)
    rest = torch.randn(32, generator=_gen(seed + 1))
    edge = []
    edge.append(torch.zeros(32))                                                         # all zero: X = 0
    b = rest * 2.0 ** -22; b[5] = 3.0; edge.append(b)                                    # an outlier 2^20 times the rest: the rest flush to zero
    b = rest.clamp(-1, 1) * 0.1; b[7] = -0.5; edge.append(b)                             # amax exactly a power of two
    b = rest.clamp(-1, 1); b[0] = (1 - 2.0 ** -20) * 8.0; edge.append(b)                 # just under 512 of the scale: saturates to 448
    b = torch.zeros(32); b[0] = 256.0                                                    # X = 0: RNE ties in the normal range and at 2^-10
    b[1:9] = torch.tensor([17.0, 19.0, -21.0, 2.0 ** -10, 1.5 * 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 0.0703125 + 2.0 ** -8]); b[9] = -0.0
    edge.append(b)
    b = rest.abs() * 2.0 ** -140; b[3] = 2.0 ** -128; b[4] = -0.0; edge.append(b)        # f32 denormals: X clamps to -127
    b = rest.clamp(-1, 1) * 2.0 ** 120; b[2] = -1.9 * 2.0 ** 127; edge.append(b)         # amax near 2^127
    b = rest * 2.0 ** 100; edge.append(b)
    for i, e in enumerate(edge[:blocks.shape[0]]):
        blocks[(i * 7) % blocks.shape[0]] = e
    return w


@pytest.mark.parametrize("N, K", [(8, 32), (24, 160), (40, 1088), (512, 6144)])
def test_quantizer_equals_the_specification(N, K):
    from enhancing import _C
    w = _crafted(N, K, N + K)
    q_ref, s_ref = quant(w)
    codes = torch.full((N, K), 0xAA, dtype=torch.uint8, device="cuda")
    scales = torch.full((N, K // 32), 0xAA, dtype=torch.uint8, device="cuda")
    _C.quantize_mxfp8(w.cuda(), codes, scales)
    assert torch.equal(scales.cpu(), s_ref), f"{int((scales.cpu() != s_ref).sum())} scale bytes differ"
    bad = (codes.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} codes differ, the first at {bad[0].tolist()}: {codes[tuple(bad[0])].item():#x} for {q_ref[tuple(bad[0])].item():#x}"
    assert not bool(((codes & 0x7f) == 0x7f).any()), "a NaN code from finite input"


def test_quantizer_writes_one_row_block_of_a_fused_operand():
    from enhancing import _C
    N, K = 24, 160
    w = _crafted(N, K, 3)
    q_ref, s_ref = quant(w)
    codes = torch.full((3 * N, K), 0x5C, dtype=torch.uint8, device="cuda")
    scales = torch.full((3 * N, K // 32), 0x5C, dtype=torch.uint8, device="cuda")
    big = torch.zeros(N, K + 64)                 # the master as a view with a row stride of its own
    big[:, :K] = w
    _C.quantize_mxfp8(big.cuda()[:, :K], codes, scales, row0=N)
    assert torch.equal(codes[N:2 * N].cpu(), q_ref) and torch.equal(scales[N:2 * N].cpu(), s_ref)
    for lo, hi in ((0, N), (2 * N, 3 * N)):
        assert bool((codes[lo:hi] == 0x5C).all()) and bool((scales[lo:hi] == 0x5C).all()), "rows outside the block were written"


# ---------------------------------------------------------------------------------------------
# product
# ---------------------------------------------------------------------------------------------
_OPERANDS = {}


def _operand(K, N):
    """one weight per shape, quantized once on the CPU: (codes, scales) on the device, its exact dequantization in fp64, bias"""
    if (K, N) not in _OPERANDS:
        g = _gen(K + N)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        w.view(-1, 32)[::3] *= 2.0 ** -6                   # block scales that differ inside a row
        q, s = quant(w)
        _OPERANDS[(K, N)] = (q.cuda(), s.cuda(), dequant(q, s).double(), 0.5 * torch.randn(N, generator=g))
    return _OPERANDS[(K, N)]


def _check_product(x, q, s, wd, bias, res, what, combos):
    from enhancing import _C
    (M, K), N, dt = x.shape, q.shape[0], x.dtype
    xd = x.double().cpu()
    acc, mag = xd @ wd.t(), xd.abs() @ wd.abs().t()
    for use_b, use_r, relu, odt in combos:
        pre = acc + (bias.double() if use_b else 0.0)
        pmag = mag + (bias.double().abs() if use_b else 0.0)
        if relu:      # as tests/test_gpt_kernels_gpu.py: d(v^2) = (2 v + dv) dv
            b_pre = (2 * K + 8) * E24 * pmag
            ref, m2 = torch.relu(pre) ** 2, (2 * torch.relu(pre) + b_pre) * pmag
        else:
            ref, m2 = pre, pmag
        if use_r:
            ref, m2 = ref + res.double(), m2 + res.double().abs()
        out = torch.full((M, N), float("nan"), dtype=odt, device="cuda")
        kw = dict(bias=bias.cuda() if use_b else None, relu_sq=relu, res=res.cuda() if use_r else None)
        _C.skinny_gemm_w8(x, q, s, out, **kw)
        worst = assert_elementwise(out, ref, elem_bound(ref, m2, K, odt if odt in U16 else None), f"{what} bias={use_b} res={use_r} relu={relu} -> {odt}",
                                   tile=(16, 16))
        out2 = torch.full_like(out, float("nan"))
        _C.skinny_gemm_w8(x, q, s, out2, **kw)
        bits = torch.int16 if odt in U16 else torch.int32
        assert torch.equal(out.view(bits), out2.view(bits)), "bits differ between two calls"
        assert worst <= 1.0


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("K, N", [(32, 8), (128, 384), (160, 264), (768, 3072), (6144, 512)])
@pytest.mark.parametrize("M", [1, 3, 16, 17, 64])
def test_skinny_gemm_w8_against_fp64(M, K, N, fmt):
    dt = H16[fmt]
    q, s, wd, bias = _operand(K, N)
    g = _gen(1000 * M + K + N)
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    res = torch.randn(M, N, generator=g)
    #          bias   res    relu^2  output
    combos = [(False, False, False, torch.float32), (True, False, True, dt), (True, True, False, torch.float32), (False, True, True, torch.float32),
              (True, True, False, dt)]
    _check_product(x, q, s, wd, bias, res, f"skinny_gemm_w8 M={M} K={K} N={N} {fmt}", combos)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("K", [128, 768])
def test_block_scales_cost_no_accuracy(K, fmt):
    """operands built by hand from codes and scale bytes: rows whose every block has X = -28 (folded into an fp16 operand the weights underflow),
    rows with X = +10 (there they overflow), rows whose block exponents cycle through 0 .. 20; f32 output, the same element bound"""
    dt = H16[fmt]
    N, M = 48, 17
    g = _gen(K)
    vals = torch.randn(N, K, generator=g).clamp(-3, 3) * 100.0
    q = vals.to(torch.float8_e4m3fn).view(torch.uint8)
    X = torch.zeros(N, K // 32, dtype=torch.int64)
    X[:16] = -28
    X[16:32] = 10
    X[32:] = (torch.arange(K // 32)[None, :] * 5 + torch.arange(16)[:, None]) % 21
    s = (X + 127).to(torch.uint8)
    wd = dequant(q, s).double()
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    _check_product(x, q.cuda(), s.cuda(), wd, None, None, f"hand-built scales K={K} {fmt}", [(False, False, False, torch.float32)])


def test_refusals():
    from enhancing import _C
    K, N = 128, 16
    q = torch.zeros(N, K, dtype=torch.uint8, device="cuda")
    s = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
    x = lambda M, K=K, dt=torch.float16: torch.zeros(M, K, dtype=dt, device="cuda")
    out = lambda M: torch.empty(M, N, dtype=torch.float32, device="cuda")
    _C.skinny_gemm_w8(x(2), q, s, out(2))
    with pytest.raises(RuntimeError, match="M must be in"):
        _C.skinny_gemm_w8(x(65), q, s, out(65))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _C.skinny_gemm_w8(x(2, 40), torch.zeros(N, 40, dtype=torch.uint8, device="cuda"), torch.zeros(N, 1, dtype=torch.uint8, device="cuda"), out(2))
    with pytest.raises(RuntimeError, match="do not fit"):
        _C.skinny_gemm_w8(x(2), q, s[:, :3].contiguous(), out(2))
    with pytest.raises(RuntimeError, match="x must be"):
        _C.skinny_gemm_w8(x(2, dt=torch.float32), q, s, out(2))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _C.quantize_mxfp8(torch.zeros(8, 40, device="cuda"), torch.zeros(8, 40, dtype=torch.uint8, device="cuda"), torch.zeros(8, 1, dtype=torch.uint8, device="cuda"))
