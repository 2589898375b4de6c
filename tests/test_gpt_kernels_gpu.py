"""The decode-shaped kernels of stage-2 sampling (csrc/gpt_decode.hip and the row kernels of csrc/gpt_rows.hip), each against an fp64 statement of what it computes, with bounds worked out
from the number formats (tests/util.py elem_bound and the reasoning written at each check); nothing here is a measured tolerance."""
import math

import numpy as np
import pytest
import torch

import gpt_cases as GC
from util import SUB16, U16, assert_elementwise, elem_bound

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
E24 = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------
# skinny GEMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("K, N", [(128, 384), (768, 3072), (6144, 512)])
@pytest.mark.parametrize("M", [1, 3, 16, 17, 64])
def test_skinny_gemm_against_fp64(M, K, N, fmt):
    from enhancing import _C
    dt = H16[fmt]
    g = _gen(1000 * M + K + N)
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dt).cuda()
    bias = (0.5 * torch.randn(N, generator=g)).cuda()
    res = torch.randn(M, N, generator=g).cuda()
    acc = x.double() @ w.double().t()                      # the truth: an fp64 product of the rounded operands
    mag = x.double().abs() @ w.double().abs().t()
    #        bias   res    relu^2  output
    for use_b, use_r, relu, odt in [(False, False, False, torch.float32), (True, False, True, dt), (True, True, False, torch.float32),
                                    (False, True, True, torch.float32), (True, True, False, dt)]:
        pre = acc + (bias.double() if use_b else 0.0)
        pmag = mag + (bias.double().abs() if use_b else 0.0)
        if relu:
            # d(v^2) = (2 v + dv) dv with |dv| <= the bound of the pre-activation: the magnitude carries the factor; 2 v^2 <= the new magnitude, so
            # elem_bound's "+ 8" also covers the rounding of the square itself
            b_pre = (2 * K + 8) * E24 * pmag
            ref, m2 = torch.relu(pre) ** 2, (2 * torch.relu(pre) + b_pre) * pmag
        else:
            ref, m2 = pre, pmag
        if use_r:
            ref, m2 = ref + res.double(), m2 + res.double().abs()
        out = torch.full((M, N), float("nan"), dtype=odt, device="cuda")
        kw = dict(bias=bias if use_b else None, relu_sq=relu, res=res if use_r else None)
        _C.skinny_gemm(x, w, out, **kw)
        worst = assert_elementwise(out, ref, elem_bound(ref, m2, K, odt if odt in U16 else None), f"skinny_gemm M={M} K={K} N={N} {fmt} {kw.keys()} -> {odt}",
                                   tile=(16, 16))
        out2 = torch.full_like(out, float("nan"))
        _C.skinny_gemm(x, w, out2, **kw)
        assert torch.equal(out.view(torch.int16 if odt in U16 else torch.int32), out2.view(torch.int16 if odt in U16 else torch.int32)), "bits differ between two calls"
        assert worst <= 1.0


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("M", [3, 17, 40])
def test_skinny_gemm_tails_against_fp64(M, fmt):
    """N % 16 == 8 (half a row tile) and K % 128 != 0, K % 32 != 0 (a partial chunk whose last MFMA step is half empty), with and without K slabs"""
    from enhancing import _C
    dt = H16[fmt]
    for K, N in [(200, 264), (8, 8), (1096, 40)]:
        g = _gen(M + K + N)
        x = torch.randn(M, K, generator=g).to(dt).cuda()
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dt).cuda()
        bias, res = (0.5 * torch.randn(N, generator=g)).cuda(), torch.randn(M, N, generator=g).cuda()
        ref = x.double() @ w.double().t() + bias.double() + res.double()
        mag = x.double().abs() @ w.double().abs().t() + bias.double().abs() + res.double().abs()
        for odt in (torch.float32, dt):
            out = torch.full((M, N), float("nan"), dtype=odt, device="cuda")
            _C.skinny_gemm(x, w, out, bias=bias, res=res)
            assert_elementwise(out, ref, elem_bound(ref, mag, K, odt if odt in U16 else None), f"skinny_gemm tails M={M} K={K} N={N} {fmt} -> {odt}", tile=(16, 16))


def test_skinny_gemm_refuses_more_than_64_rows_and_odd_widths():
    from enhancing import _C
    w = torch.zeros(64, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match=r"M must be in \[1, 64\]"):
        _C.skinny_gemm(torch.zeros(65, 64, dtype=torch.float16, device="cuda"), w, torch.empty(65, 64, device="cuda"))
    with pytest.raises(RuntimeError, match="multiples of 8"):
        _C.skinny_gemm(torch.zeros(2, 12, dtype=torch.float16, device="cuda"), torch.zeros(64, 12, dtype=torch.float16, device="cuda"), torch.empty(2, 64, device="cuda"))
    assert _C.lib().enh_skinny_gemm_workspace_bytes(16, 512, 6144) > 0 and _C.lib().enh_skinny_gemm_workspace_bytes(16, 24576, 6144) == 0


# ---------------------------------------------------------------------------------------------
# decode attention
# ---------------------------------------------------------------------------------------------
# The kernel cuts a cache of `len` slots into max(ceil(len / 256), min(ceil(len / 64), ceil(512 / (B H)))) pieces of equal length rounded up to 32
# (csrc/gpt_decode.hip gd_att_plan).  With B H <= 48 the second term rules: pieces of 64 slots (96 at B H = 48, len 1024), so these lengths sit on both
# sides of the 32-slot score pass and of the 64-slot minimum piece, and reach the merge with many short pieces.
LENS = [1, 2, 63, 64, 65, 257, 1024]
# With B H >= 512 one piece serves up to 256 slots in a single launch (all four waves of the max / sum reductions and every word of the score
# array in use); 255 | 256 | 257 is that boundary: 257 = two pieces of 160 + 97, 513 = three of 192 + 192 + 129.  B H = 256 at len 1024 = four full
# pieces of 256, the shape of the shipped model at batch 16.
LONG_PIECES = [(64, 8, 64, [128, 255, 256, 257, 513]), (16, 16, 64, [1024]), (32, 16, 128, [256, 257])]


@pytest.mark.parametrize("fmt", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("B, H", [(1, 1), (2, 3), (8, 6)])
@pytest.mark.parametrize("hs", [64, 128, 384])
def test_decode_attention_against_fp64(hs, B, H, fmt):
    _check_decode_attention(hs, B, H, fmt, LENS)


@pytest.mark.parametrize("fmt", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("B, H, hs, lens", LONG_PIECES)
def test_decode_attention_full_pieces_against_fp64(B, H, hs, lens, fmt):
    _check_decode_attention(hs, B, H, fmt, lens)


def _check_decode_attention(hs, B, H, fmt, lens):
    from enhancing import _C
    dt = H16.get(fmt, torch.float32)
    C = H * hs
    g = _gen(hs + 7 * B)
    for n in lens:
        t, Tmax = n - 1, n + 3
        qkv = torch.randn(B, 3 * C, generator=g).to(dt).cuda()
        kc = torch.randn(B, H, Tmax, hs, generator=g).to(dt).cuda()
        vc = torch.randn(B, H, Tmax, hs, generator=g).to(dt).cuda()
        kc[:, :, t:], vc[:, :, t:] = float("nan"), float("nan")      # slot t is written, slots > t must never be read
        k0, v0 = kc.clone(), vc.clone()
        out = torch.full((B, C), float("nan"), dtype=dt, device="cuda")
        _C.decode_attention(qkv, kc, vc, t, out)
        q, k, v = (z.view(B, H, hs) for z in qkv.split(C, dim=1))
        assert torch.equal(kc[:, :, t], k) and torch.equal(vc[:, :, t], v), f"slot {t} does not hold the step's k / v"
        assert torch.equal(kc[:, :, :t], k0[:, :, :t]) and torch.equal(vc[:, :, :t], v0[:, :, :t]), "older slots changed"
        assert bool(torch.isnan(kc[:, :, t + 1:]).all()) and bool(torch.isnan(vc[:, :, t + 1:]).all()), "slots > t were written"
        assert bool(torch.isfinite(out.float()).all()), f"len {n}: the output is not finite: a slot > t was read"
        # the truth: fp64 on the cache contents as stored
        K64, V64, q64 = kc[:, :, :n].double(), vc[:, :, :n].double(), q.double()
        scale = 1.0 / math.sqrt(hs)
        s = torch.einsum("bhd,bhtd->bht", q64, K64) * scale
        p = torch.softmax(s, dim=-1)
        ref = torch.einsum("bht,bhtd->bhd", p, V64).reshape(B, C)
        pav = torch.einsum("bht,bhtd->bhd", p, V64.abs()).reshape(B, C)
        # scores: an f32 fma chain of hs exact products: |ds| <= (2 hs + 8) 2^-24 max_j sum_d |q_d k_jd| scale (elem_bound's sum model).  A probability is
        # a ratio of exponentials of scores: relative error <= 2 ds, plus expf and the f32 sums of n terms in any order ((2 n + 8) 2^-24 of P |V|).
        ds = (2 * hs + 8) * E24 * torch.einsum("bhd,bhtd->bht", q64.abs(), K64.abs()).amax(-1) * scale        # [B, H]
        bound = (2 * ds.unsqueeze(-1) + (2 * n + 8) * E24 + 8 * E24).expand(B, H, hs).reshape(B, C) * pav
        if dt in U16:
            bound = bound + U16[dt] * ref.abs() + SUB16.get(dt, 0.0)
        assert_elementwise(out, ref, bound, f"decode_attention hs={hs} B={B} H={H} len={n} {fmt}")
        kc2, vc2, out2 = k0.clone(), v0.clone(), torch.full_like(out, float("nan"))
        _C.decode_attention(qkv, kc2, vc2, t, out2)
        bits = torch.int16 if dt in U16 else torch.int32
        assert torch.equal(out.view(bits), out2.view(bits)), f"len {n}: bits differ between two calls"


def test_decode_attention_refuses_other_head_sizes():
    from enhancing import _C
    for hs in (32, 96, 448):
        qkv = torch.zeros(1, 3 * hs, dtype=torch.float16, device="cuda")
        c = torch.zeros(1, 1, 4, hs, dtype=torch.float16, device="cuda")
        with pytest.raises(RuntimeError, match="multiple of 64 up to 384"):
            _C.decode_attention(qkv, c, c.clone(), 0, torch.empty(1, hs, dtype=torch.float16, device="cuda"))


# ---------------------------------------------------------------------------------------------
# row LayerNorm, embedding
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 64])
@pytest.mark.parametrize("D", [8, 128, 2056, 6144, 8192])
def test_row_ln_scale_against_fp64(D, M):
    from enhancing import _C
    g = _gen(D + M)
    x = (0.5 + 2.0 * torch.randn(M, D, generator=g)).cuda()
    w = (1.0 + 0.1 * torch.randn(D, generator=g)).cuda()
    b = (0.1 * torch.randn(D, generator=g)).cuda()
    sc = torch.rand(D, generator=g).cuda()
    x64 = x.double()
    mean, var = x64.mean(-1, keepdim=True), x64.var(-1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (x64 - mean) * rstd
    # f32 statistics: a thread adds <= 32 values, then a 10-level tree: sums carry <= 42 x 2^-24 of the mean |x| (the mean) or of the variance (rstd:
    # half of that, relative); x - mean, the three products and the sum add a few roundings each.  64 x 2^-24 covers each group.
    a = x64.abs().mean(-1, keepdim=True) * rstd
    for scale in (None, sc):
        s64 = torch.ones(D, dtype=torch.float64, device="cuda") if scale is None else scale.double()
        ref = (xhat * w.double() + b.double()) * s64
        base = 64 * E24 * ((xhat.abs() + a) * (w.double() * s64).abs()) + 8 * E24 * (b.double() * s64).abs()
        for odt in (torch.float32, torch.float16, torch.bfloat16):
            out = torch.full((M, D), float("nan"), dtype=odt, device="cuda")
            _C.row_ln_scale(x, w, b, out, colscale=scale)
            bound = base + (U16[odt] * ref.abs() + SUB16.get(odt, 0.0) if odt in U16 else 0.0)
            assert_elementwise(out, ref, bound, f"row_ln_scale D={D} M={M} scale={scale is not None} -> {odt}")
    for bad in (4, 12, 8200):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            _C.row_ln_scale(torch.zeros(1, bad, device="cuda"), torch.zeros(bad, device="cuda"), torch.zeros(bad, device="cuda"), torch.empty(1, bad, device="cuda"))


def test_gpt_embed_reads_ids_from_device_memory_and_exact_product():
    from enhancing import _C
    g = _gen(5)
    table, pos = torch.randn(50, 136, generator=g).cuda(), torch.randn(9, 136, generator=g).cuda()
    codes = torch.randint(0, 50, (7, 9), generator=g).cuda()
    out = torch.empty(7, 136, device="cuda")
    _C.gpt_embed(table, codes[:, 4], pos[3], out)
    assert torch.equal(out, table[codes[:, 4]] + pos[3])
    # the exact mode's product: a lane adds K / 64 products, then a 6-level tree: k = K / 64 + 6 terms in elem_bound's sum model
    for M, K, N in [(3, 768, 264), (17, 3072, 40)]:
        x, w = torch.randn(M, K, generator=g).cuda(), (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda()
        bias, res = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
        out = torch.full((M, N), float("nan"), device="cuda")
        _C.skinny_gemm_f32(x, w, out, bias=bias, res=res)
        ref = x.double() @ w.double().t() + bias.double() + res.double()
        mag = x.double().abs() @ w.double().abs().t() + bias.double().abs() + res.double().abs()
        assert_elementwise(out, ref, elem_bound(ref, mag, K // 64 + 6), f"skinny_gemm_f32 {M}x{N}x{K}")
        out2 = torch.full((M, N), float("nan"), device="cuda")
        _C.skinny_gemm_f32(x, w, out2, bias=bias, relu_sq=True)
        pre, pmag = x.double() @ w.double().t() + bias.double(), x.double().abs() @ w.double().abs().t() + bias.double().abs()
        b_pre = (2 * (K // 64 + 6) + 8) * E24 * pmag            # the square: as in test_skinny_gemm_against_fp64
        assert_elementwise(out2, torch.relu(pre) ** 2, elem_bound(pre, (2 * torch.relu(pre) + b_pre) * pmag, K // 64 + 6), f"skinny_gemm_f32 relu^2 {M}x{N}x{K}")


# ---------------------------------------------------------------------------------------------
# every decode entry point names the kernel it launched (enh_last_kernel), at its smallest legal shape
# ---------------------------------------------------------------------------------------------
def _last():
    from enhancing import _C
    return _C.lib().enh_last_kernel().decode()


def _stale():
    """a call with another label in front of the checked one, so that a label left over from an earlier call cannot pass"""
    from enhancing import _C
    _C.mean_f32(torch.ones(8, device="cuda"), torch.empty(1, device="cuda"))
    assert _last() == "gpt_prefill_mean_kernel"


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("M, N, K, mt", [(1, 8, 8, 1), (17, 8, 8, 2), (33, 8, 8, 4), (3, 16, 6144, 1)])
def test_skinny_gemm_names_its_kernel(M, N, K, mt, fmt):
    """the three row-tile forms in both operand types; (3, 16, 6144) runs K slabs, and the label is still the product kernel's"""
    from enhancing import _C
    dt = H16[fmt]
    g = _gen(M + N + K)
    x = torch.randn(M, K, generator=g).to(dt).cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dt).cuda()
    assert (_C.lib().enh_skinny_gemm_workspace_bytes(M, N, K) > 0) == (K == 6144)
    out = torch.full((M, N), float("nan"), device="cuda")
    _stale()
    _C.skinny_gemm(x, w, out)
    assert _last() == f"gpt_skinny_gemm_kernel<{'F16' if fmt == 'fp16' else 'BF16'}, {mt}>"
    ref, mag = x.double() @ w.double().t(), x.double().abs() @ w.double().abs().t()
    assert_elementwise(out, ref, elem_bound(ref, mag, K), f"skinny_gemm M={M} N={N} K={K} {fmt}")


@pytest.mark.parametrize("fmt, label", [("fp16", "gpt_decode_attn_kernel<F16, false>"), ("bf16", "gpt_decode_attn_kernel<BF16, false>"),
                                        ("f32", "gpt_decode_attn_kernel<BF16, true>")])
def test_decode_attention_names_its_kernel(fmt, label):
    from enhancing import _C
    dt = H16.get(fmt, torch.float32)
    g = _gen(3)
    qkv = torch.randn(1, 192, generator=g).to(dt).cuda()
    kc, vc = (torch.full((1, 1, 4, 64), float("nan"), dtype=dt, device="cuda") for _ in range(2))
    out = torch.full((1, 64), float("nan"), dtype=dt, device="cuda")
    _stale()
    _C.decode_attention(qkv, kc, vc, 0, out)
    assert _last() == label
    # one key: its probability is exactly 1 and the output is v itself
    assert torch.equal(out.double(), qkv[:, 128:].double()) and torch.equal(kc[0, 0, 0], qkv[0, 64:128]) and torch.equal(vc[0, 0, 0], qkv[0, 128:])


def test_row_kernels_sampler_and_exact_product_name_their_kernels():
    from enhancing import _C
    g = _gen(9)
    x, w, b = (0.5 + 2.0 * torch.randn(1, 8, generator=g)).cuda(), (1.0 + 0.1 * torch.randn(8, generator=g)).cuda(), (0.1 * torch.randn(8, generator=g)).cuda()
    for odt, label in ((torch.float16, "gpt_row_ln_kernel<F16>"), (torch.bfloat16, "gpt_row_ln_kernel<BF16>")):
        out = torch.full((1, 8), float("nan"), dtype=odt, device="cuda")
        _stale()
        _C.row_ln_scale(x, w, b, out)
        assert _last() == label
        # the bound of test_row_ln_scale_against_fp64
        x64 = x.double()
        rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + 1e-5)
        xhat = (x64 - x64.mean(-1, keepdim=True)) * rstd
        ref = xhat * w.double() + b.double()
        bound = 64 * E24 * (xhat.abs() + x64.abs().mean(-1, keepdim=True) * rstd) * w.double().abs() + 8 * E24 * b.double().abs()
        assert_elementwise(out, ref, bound + U16[odt] * ref.abs() + SUB16.get(odt, 0.0), f"row_ln_scale -> {odt}")
    g = _gen(4)
    table, pos, ids = torch.randn(5, 4, generator=g).cuda(), torch.randn(4, generator=g).cuda(), torch.tensor([3]).cuda()
    out = torch.full((1, 4), float("nan"), device="cuda")
    _stale()
    _C.gpt_embed(table, ids, pos, out)
    assert _last() == "gpt_embed_kernel" and torch.equal(out, table[ids] + pos)
    logits = torch.tensor([[0.5, -1.0, 2.0, 0.0, 1.5, -0.5, 1.0, -2.0]]).cuda()
    code = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    _stale()
    _C.sample_logits(logits, code, top_k=1, uniforms=torch.tensor([0.5]).cuda())      # top_k = 1 keeps the largest logit alone
    assert _last() == "gpt_sample_kernel" and code.item() == 2
    xs, ws = torch.randn(1, 8, generator=g).cuda(), torch.randn(1, 8, generator=g).cuda()
    out = torch.full((1, 1), float("nan"), device="cuda")
    _stale()
    _C.skinny_gemm_f32(xs, ws, out)
    assert _last() == "gpt_skinny_gemm_f32_kernel"
    ref, mag = xs.double() @ ws.double().t(), xs.double().abs() @ ws.double().abs().t()
    assert_elementwise(out, ref, elem_bound(ref, mag, 8 // 64 + 6), "skinny_gemm_f32 1x1x8")


# ---------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------
def _unambiguous(x64, keep, probs, u, top_k, top_p):
    """the fp64 restatement must not sit on a decision boundary: no tie at the top-k or top-p cut, the mass in front of the entries at the top-p cut
    at least 1e-5 from top_p, every u at least 1e-4 of the kept mass from a cumulative boundary"""
    srt = torch.sort(x64, dim=-1, descending=True).values
    if top_k is not None and top_k < x64.shape[1]:
        if bool(((srt[:, top_k - 1] - srt[:, top_k]).abs() <= 1e-5 * srt[:, top_k - 1].abs().clamp_min(1.0)).any()):
            return False
    if top_p is not None:
        p0 = torch.softmax(torch.where(torch.isfinite(x64), x64, torch.full_like(x64, -float("inf"))), -1)
        sp = torch.sort(p0, dim=-1, descending=True).values
        front = torch.cumsum(sp, -1) - sp
        nk = keep.sum(-1)                                   # kept entries: the nk largest
        for r in range(x64.shape[0]):
            n = int(nk[r])
            if n < x64.shape[1]:
                if abs(front[r, n].item() - top_p) < 1e-5 or abs(front[r, n - 1].item() - top_p) < 1e-5:
                    return False
                if sp[r, n - 1] - sp[r, n] <= 1e-6 * sp[r, n - 1]:
                    return False
    c = torch.cumsum(probs, -1)
    tgt = (u.double() * c[:, -1]).unsqueeze(-1)
    live = probs > 0
    return not bool((((c - tgt).abs() < 1e-4 * c[:, -1:]) & live).any())


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("top_p", [None, 0.9])
@pytest.mark.parametrize("top_k", [None, 1, 50])
@pytest.mark.parametrize("V", [512, 1000, 8192])
def test_sampler_equals_the_fp64_restatement(V, top_k, top_p, temperature):
    from enhancing import _C
    B = 4
    for seed in range(100):      # inputs are CHOSEN so that the fp64 restatement is unambiguous; the conditions are asserted below
        g = _gen(seed + V)
        logits = 2.0 * torch.randn(B, V, generator=g)
        u = torch.rand(B, generator=g).clamp(1e-3, 1 - 1e-3)
        x32 = logits / temperature                              # the kernel's f32 division
        x64, keep, probs = GC.host_filter(x32.double(), top_k, top_p, 1.0)
        if _unambiguous(x64, keep, probs, u, top_k, top_p):
            break
    assert _unambiguous(x64, keep, probs, u, top_k, top_p), "no unambiguous input found"
    want = GC.inverse_cdf(probs, u.double())
    codes = torch.full((B, 3), -1, dtype=torch.int64, device="cuda")
    lo = torch.full((B, 2 * V), float("nan"), device="cuda")
    mask = torch.full((B, V), 7, dtype=torch.uint8, device="cuda")
    pr = torch.full((B, V), float("nan"), device="cuda")
    _C.sample_logits(logits.cuda(), codes[:, 1], temperature=temperature, top_k=top_k, top_p=top_p, uniforms=u.cuda(), logits_out=lo[:, V:], mask_out=mask,
                     probs_out=pr)
    assert torch.equal(mask.cpu().bool(), keep), "kept mask differs from the fp64 restatement"
    # probabilities to f32 rounding: exp of an f32 argument of size <= 32 (relative 2^-24 |x - max| + expf's own ulp) and f32 sums in tree order
    err = (pr.cpu().double() - probs).abs()
    assert bool((err <= 128 * E24 * probs + 1e-37).all()), (err / probs.clamp_min(1e-300)).max().item()
    assert torch.equal(codes[:, 1].cpu(), want), (codes[:, 1].cpu(), want)
    assert bool((codes[:, 0] == -1).all()) and bool((codes[:, 2] == -1).all()) and bool(torch.isnan(lo[:, :V]).all())
    got = lo[:, V:].cpu()
    fin = torch.isfinite(x64)
    assert torch.equal(torch.isfinite(got), fin) and bool((got[~fin] == -float("inf")).all())
    assert torch.equal(got[fin], x32[fin]), "the stored logits row is logits / temperature with -inf below the k-th largest"


def test_sampler_top_k_keeps_ties():
    from enhancing import _C
    logits = torch.tensor([[0.0, 3.0, 1.0, 3.0, 2.0, 2.0, -1.0, 2.0]]).cuda()
    codes = torch.empty(1, 1, dtype=torch.int64, device="cuda")
    mask = torch.empty(1, 8, dtype=torch.uint8, device="cuda")
    _C.sample_logits(logits, codes[:, 0], top_k=3, uniforms=torch.tensor([0.5]).cuda(), mask_out=mask)
    assert mask.cpu().tolist() == [[0, 1, 0, 1, 1, 1, 0, 1]]


def _chi2(counts, probs):
    n = counts.sum()
    return float((((counts - n * probs) ** 2) / (n * probs)).sum())


def test_sampler_device_generator_statistics_and_streams():
    """V = 8, 20 000 draws from the device generator against the exact probabilities: chi-square with 7 degrees of freedom at the 1e-4 level (29.88)"""
    from enhancing import _C
    n, crit = 20000, 29.878
    logits = torch.tensor([0.3, -1.2, 2.0, 0.0, 1.1, -0.4, 0.9, -2.5])
    probs = torch.softmax(logits.double(), 0).numpy()
    ref_draw = np.random.default_rng(12345).choice(8, size=n, p=probs)
    assert _chi2(np.bincount(ref_draw, minlength=8), probs) < crit      # the statistic itself, on numpy's generator
    rows = logits.repeat(n, 1).contiguous().cuda()

    def draw(seed, step=3):
        codes = torch.empty(n, dtype=torch.int64, device="cuda")
        _C.sample_logits(rows, codes, seed=seed, call=1, step=step)
        return codes.cpu()
    a, a2, b, c = draw(2024), draw(2024), draw(2025), draw(2024, step=4)
    assert _chi2(np.bincount(a.numpy(), minlength=8), probs) < crit
    assert torch.equal(a, a2), "one seed must give one stream"
    assert (a != b).float().mean().item() > 0.5 and (a != c).float().mean().item() > 0.5, "another seed or step must give another stream"
