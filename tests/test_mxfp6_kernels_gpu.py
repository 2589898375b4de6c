"""The MXFP6 weight kernels (csrc/gpt_decode_w6.hip).  The quantizer is held to tests/mxfp6_util.py bit for bit; the product to an fp64 product of
x and the exactly dequantized weight, under tests/util.py's element bound.  That bound is worked out from the number formats and carries over from
the 16-bit product as it stands: a dequantized weight has 4 significant bits and x has 11 or 8, so every product is exact in f32 and what remains is
the f32 sum of K terms and the one rounding of the store.  Nothing here is a measured tolerance."""
import math

import pytest
import torch

from mxfp6_util import dequant, pack, quant, row_bytes, unpack
from test_mxfp6_cpu import special_blocks
from util import U16, assert_elementwise, elem_bound

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
E24 = 2.0 ** -24
GUARD = 4096      # bytes of sentinel on either side of an output or of the workspace


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# quantizer
# ---------------------------------------------------------------------------------------------
def _crafted(N, K, seed):
    """randn / sqrt(K) with the hand-made blocks of tests/test_mxfp6_cpu.py written over it, as many as the shape holds, and blocks of wide
    exponents"""
    w = torch.randn(N, K, generator=_gen(seed)) / math.sqrt(K)
    blocks = w.view(-1, 32)
    rest = torch.randn(32, generator=_gen(seed + 1))
    edge = [b for b, _, _ in special_blocks().values()]
    edge.append(rest * 2.0 ** -22 + torch.nn.functional.one_hot(torch.tensor(5), 32) * 3.0)      # an outlier 2^20 times the rest: the rest flush to zero
    edge.append(rest.abs() * 2.0 ** -140)
    edge.append(rest * 2.0 ** 100)
    for i, e in enumerate(edge[:blocks.shape[0]]):
        blocks[(i * 7) % blocks.shape[0]] = e
    return w


@pytest.mark.parametrize("N, K", [(8, 32), (24, 160), (40, 1088), (512, 6144)])
def test_quantizer_equals_the_specification(N, K):
    from enhancing import _C
    w = _crafted(N, K, N + K)
    q_ref, s_ref = quant(w)
    codes = torch.full((N, row_bytes(K)), 0xAA, dtype=torch.uint8, device="cuda")
    scales = torch.full((N, K // 32), 0xAA, dtype=torch.uint8, device="cuda")
    _C.quantize_mxfp6(w.cuda(), codes, scales)
    assert torch.equal(scales.cpu(), s_ref), f"{int((scales.cpu() != s_ref).sum())} scale bytes differ"
    bad = (codes.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} code bytes differ, the first at {bad[0].tolist()}: {codes[tuple(bad[0])].item():#x} for {q_ref[tuple(bad[0])].item():#x}"
    assert not bool((scales == 0xFF).any()), "a NaN scale from finite input"


def test_quantizer_on_the_special_blocks_in_one_row():
    """every hand-made block of the CPU file side by side in one row, and the chosen non-finite behaviour: scale byte 0xff, all-zero codes"""
    from enhancing import _C
    S = special_blocks()
    row = torch.cat([b for b, _, _ in S.values()])
    w = torch.stack([row, row.flip(0).contiguous(), row.clone()])
    w[2, 40] = float("inf")
    w[2, 3 * 32 + 1] = float("nan")
    K = w.shape[1]
    q_ref, s_ref = quant(w)
    assert s_ref[0].tolist() == [sc for _, sc, _ in S.values()] and s_ref[2, 1].item() == 0xFF and s_ref[2, 3].item() == 0xFF
    codes = torch.full((3, row_bytes(K)), 0xAA, dtype=torch.uint8, device="cuda")
    scales = torch.full((3, K // 32), 0xAA, dtype=torch.uint8, device="cuda")
    _C.quantize_mxfp6(w.cuda(), codes, scales)
    assert torch.equal(scales.cpu(), s_ref) and torch.equal(codes.cpu(), q_ref)
    c = unpack(codes.cpu())
    assert bool((c[2, 32:64] == 0).all()) and bool((c[2, 96:128] == 0).all()) and bool((c[:, K:] == 0).all())      # K = 448: half a chunk of padding


def test_quantizer_writes_one_row_block_of_a_fused_operand():
    from enhancing import _C
    N, K = 24, 160
    w = _crafted(N, K, 3)
    q_ref, s_ref = quant(w)
    codes = torch.full((3 * N, row_bytes(K)), 0x5C, dtype=torch.uint8, device="cuda")
    scales = torch.full((3 * N, K // 32), 0x5C, dtype=torch.uint8, device="cuda")
    big = torch.zeros(N, K + 64)                 # the master as a view with a row stride of its own
    big[:, :K] = w
    _C.quantize_mxfp6(big.cuda()[:, :K], codes, scales, row0=N)
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


def _guarded(M, N, odt):
    """(the [M, N] view, the whole buffer): NaN inside, a sentinel in GUARD bytes on either side"""
    pad = GUARD // torch.empty((), dtype=odt).element_size()
    whole = torch.full((2 * pad + M * N,), 12345.0, dtype=odt, device="cuda")
    whole[pad:pad + M * N] = float("nan")
    return whole[pad:pad + M * N].view(M, N), whole, pad


def _guards_intact(whole, pad, what):
    assert bool((whole[:pad] == 12345.0).all()) and bool((whole[-pad:] == 12345.0).all()), f"{what}: written outside the output"


def _guarded_workspace(monkeypatch, M, N, K):
    """makes _C._workspace hand out the middle of a sentinel-filled buffer of exactly the size the product asks for; returns a check"""
    from enhancing import _C
    nb = int(_C.lib().enh_skinny_gemm_w6_workspace_bytes(M, N, K))
    if nb == 0:
        return lambda what: None
    whole = torch.full((2 * GUARD + nb,), 0x5C, dtype=torch.uint8, device="cuda")

    def workspace(nbytes, device):
        assert nbytes == nb
        return whole[GUARD:GUARD + nb]
    monkeypatch.setattr(_C, "_workspace", workspace)

    def check(what):
        assert bool((whole[:GUARD] == 0x5C).all()) and bool((whole[GUARD + nb:] == 0x5C).all()), f"{what}: written outside the workspace"
    return check


def _check_product(x, q, s, wd, bias, res, what, combos, monkeypatch):
    from enhancing import _C
    (M, K), N, dt = x.shape, q.shape[0], x.dtype
    ws_check = _guarded_workspace(monkeypatch, M, N, K)
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
        label = f"{what} bias={use_b} res={use_r} relu={relu} -> {odt}"
        out, whole, pad = _guarded(M, N, odt)
        kw = dict(bias=bias.cuda() if use_b else None, relu_sq=relu, res=res.cuda() if use_r else None)
        _C.skinny_gemm_w6(x, q, s, out, **kw)
        worst = assert_elementwise(out, ref, elem_bound(ref, m2, K, odt if odt in U16 else None), label, tile=(16, 16))
        _guards_intact(whole, pad, label)
        ws_check(label)
        out2 = torch.full((M, N), float("nan"), dtype=odt, device="cuda")
        _C.skinny_gemm_w6(x, q, s, out2, **kw)
        bits = torch.int16 if odt in U16 else torch.int32
        assert torch.equal(out.contiguous().view(bits), out2.view(bits)), "bits differ between two calls"
        assert worst <= 1.0


def _all_combos(dt):
    return [(b, r, a, o) for b in (False, True) for r in (False, True) for a in (False, True) for o in (torch.float32, dt)]


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("K, N", [(32, 8), (128, 384), (160, 264), (768, 3072), (6144, 512), (24576, 40)])
@pytest.mark.parametrize("M", [1, 3, 16, 17, 64])
def test_skinny_gemm_w6_against_fp64(M, K, N, fmt, monkeypatch):
    dt = H16[fmt]
    q, s, wd, bias = _operand(K, N)
    g = _gen(1000 * M + K + N)
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    res = torch.randn(M, N, generator=g)
    if (K, N) in ((160, 264), (6144, 512)):      # every bias / residual / relu^2 / output combination: one shape without slabs, one with
        combos = _all_combos(dt)
    else:
        #          bias   res    relu^2  output
        combos = [(False, False, False, torch.float32), (True, False, True, dt), (True, True, False, torch.float32), (False, True, True, torch.float32),
                  (True, True, False, dt)]
    _check_product(x, q, s, wd, bias, res, f"skinny_gemm_w6 M={M} K={K} N={N} {fmt}", combos, monkeypatch)


def test_the_shapes_cover_both_plans():
    from enhancing import _C
    ws = _C.lib().enh_skinny_gemm_w6_workspace_bytes
    assert ws(16, 264, 160) == 0 and ws(16, 8, 32) == 0 and ws(16, 512, 6144) > 0
    assert ws(64, 40, 24576) == 24 * 64 * 40 * 4      # 192 chunks, eight to a slab: the most slabs a shipped-size K gives


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("K", [128, 768])
def test_block_scales_cost_no_accuracy(K, fmt, monkeypatch):
    """operands built by hand from codes and scale bytes: rows whose every block has X = -28 (folded into an fp16 operand the weights underflow),
    rows with X = +10 (there they overflow), rows whose block exponents cycle through 0 .. 20; f32 output, the same element bound.  Every k holds
    a code of its own, so a product inside the bound also shows that the order of the codes inside a piece is the conversion's"""
    dt = H16[fmt]
    N, M = 48, 17
    g = _gen(K)
    q = pack(torch.randint(0, 64, (N, K), generator=g))      # all 64 codes, -0.0 among them
    X = torch.zeros(N, K // 32, dtype=torch.int64)
    X[:16] = -28
    X[16:32] = 10
    X[32:] = (torch.arange(K // 32)[None, :] * 5 + torch.arange(16)[:, None]) % 21
    s = (X + 127).to(torch.uint8)
    wd = dequant(q, s).double()
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    _check_product(x, q.cuda(), s.cuda(), wd, None, None, f"hand-built scales K={K} {fmt}", [(False, False, False, torch.float32)], monkeypatch)


def test_refusals():
    from enhancing import _C
    K, N = 128, 16
    q = torch.zeros(N, row_bytes(K), dtype=torch.uint8, device="cuda")
    s = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
    x = lambda M, K=K, dt=torch.float16: torch.zeros(M, K, dtype=dt, device="cuda")
    out = lambda M, N=N: torch.empty(M, N, dtype=torch.float32, device="cuda")
    _C.skinny_gemm_w6(x(2), q, s, out(2))
    with pytest.raises(RuntimeError, match="M must be in"):
        _C.skinny_gemm_w6(x(65), q, s, out(65))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _C.skinny_gemm_w6(x(2, 40), torch.zeros(N, 96, dtype=torch.uint8, device="cuda"), torch.zeros(N, 1, dtype=torch.uint8, device="cuda"), out(2))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _C.skinny_gemm_w6(x(2), q[:12], s[:12], out(2, 12))
    with pytest.raises(RuntimeError, match="do not fit"):
        _C.skinny_gemm_w6(x(2), q, s[:, :3].contiguous(), out(2))
    with pytest.raises(RuntimeError, match=r"codes \[N, 96 ceil\(K / 128\)\]"):      # the 4-bit operand's width is not this format's
        _C.skinny_gemm_w6(x(2), q[:, :K // 2].contiguous(), s, out(2))
    with pytest.raises(RuntimeError, match=r"codes \[rows, 96 ceil\(K / 128\)\]"):
        _C.quantize_mxfp6(torch.zeros(8, 160, device="cuda"), torch.zeros(8, 120, dtype=torch.uint8, device="cuda"), torch.zeros(8, 5, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="x must be"):
        _C.skinny_gemm_w6(x(2, dt=torch.float32), q, s, out(2))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        _C.quantize_mxfp6(torch.zeros(8, 40, device="cuda"), torch.zeros(8, 96, dtype=torch.uint8, device="cuda"), torch.zeros(8, 1, dtype=torch.uint8, device="cuda"))
    # the library's own argument checks, below the bindings
    L, p = _C.lib(), lambda t: t.data_ptr()
    o = out(2)
    x2 = x(2)
    args = lambda xx, M=2, N=N, K=K: (xx, p(q), p(s), M, N, K, None, 0, None, p(o), None, None, 0, _C._dt(x2), _C._stream())
    assert L.enh_skinny_gemm_w6(*args(None)) != 0 and b"null pointer" in L.enh_last_error()
    assert L.enh_skinny_gemm_w6(*args(p(x2), M=65)) != 0 and b"M must be in" in L.enh_last_error()
    assert L.enh_skinny_gemm_w6(*args(p(x2), K=48)) != 0 and b"multiple of 8 and K of 32" in L.enh_last_error()
    assert L.enh_skinny_gemm_w6(*args(p(x2), N=12)) != 0 and b"multiple of 8 and K of 32" in L.enh_last_error()
    assert L.enh_mxfp6_quantize(None, 8, 32, 32, p(q), 0, p(s), 0, _C._stream()) != 0 and b"null pointer" in L.enh_last_error()
