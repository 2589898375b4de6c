"""The kernels of csrc/rq_decode.hip on their own: enh_rq_embed_step against the same f32 sums in torch (bit for bit) and against
enh_rq_embed_seq's rows, and enh_short_decode_attention against fp64 and against enh_decode_attention on the same inputs, under the bound of
tests/test_gpt_kernels_gpu.py's decode-attention test."""
import math

import pytest
import torch

from util import SUB16, U16, assert_elementwise

pytestmark = pytest.mark.gpu

H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
E24 = 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _last():
    from enhancing import _C
    return _C.lib().enh_last_kernel().decode()


# ---------------------------------------------------------------------------------------------
# the step's embedding
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("C", [4, 132, 4100])      # 4100: past the 1024 float4 columns of one pass
def test_rq_embed_step_is_the_f32_sum_in_depth_order_and_rq_embed_seq_s_row(C, B):
    from enhancing import _C
    V, Vc, T, D = 37, 3, 3, 8
    g = _gen(C + B)
    table, tok_cond = torch.randn(V, C, generator=g).cuda(), torch.randn(Vc, C, generator=g).cuda()
    pos_code, pos_depth, pos_cond = torch.randn(T, C, generator=g).cuda(), torch.randn(D - 1, C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
    codes = torch.randint(0, V, (B, T, D), generator=g).cuda()
    conds = torch.randint(0, Vc, (B,), generator=g).cuda()
    spatial = torch.full((B, T, C), float("nan"), device="cuda")
    depth = torch.full((B * T, D, C), float("nan"), device="cuda")
    _C.rq_embed_seq(conds, codes, tok_cond, pos_cond, table, pos_code, pos_depth, spatial, depth)
    depth = depth.view(B, T, D, C)
    t = 1
    for n in (1, 3, 8):
        ids = codes[:, t, :n]      # a strided view of the [B, T, D] codes: row stride T D
        assert ids.stride(0) == T * D or B == 1
        pos = pos_code[t] if n == D else pos_depth[n - 1]
        out = torch.full((B, C), float("nan"), device="cuda")
        _C.rq_embed_step(table, ids, pos, out)
        assert _last() == "rq_embed_step_kernel"
        want = table[ids[:, 0]]
        for j in range(1, n):
            want = want + table[ids[:, j]]
        want = want + pos
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), f"n={n}: not the bits of the f32 sums in ascending depth"
        seq_row = spatial[:, t + 1] if n == D else depth[:, t, n]
        assert torch.equal(out.view(torch.int32), seq_row.view(torch.int32)), f"n={n}: not the bits of rq_embed_seq's row"


def test_rq_embed_step_refuses_bad_arguments_and_never_follows_a_bad_id():
    """a bad n or C is an error code; an id outside the table cannot be seen from the host without reading it back, so the kernel clamps it to the
    table's rows, as enh_gpt_embed does: never a fault, never another row's memory"""
    from enhancing import _C
    g = _gen(1)
    table, pos = torch.randn(6, 8, generator=g).cuda(), torch.randn(8, generator=g).cuda()
    out = torch.full((2, 8), float("nan"), device="cuda")
    for n in (0, 9):
        with pytest.raises(RuntimeError, match=r"must be in \[1, 8\]"):
            _C.rq_embed_step(table, torch.zeros(2, n, dtype=torch.int64, device="cuda"), pos, out)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        _C.rq_embed_step(torch.zeros(6, 6, device="cuda"), torch.zeros(2, 1, dtype=torch.int64, device="cuda"), torch.zeros(6, device="cuda"),
                         torch.empty(2, 6, device="cuda"))
    with pytest.raises(RuntimeError, match="int64"):
        _C.rq_embed_step(table, torch.zeros(2, 2, dtype=torch.int32, device="cuda"), pos, out)
    with pytest.raises(RuntimeError, match="contiguous"):
        _C.rq_embed_step(table, torch.zeros(2, 4, dtype=torch.int64, device="cuda")[:, ::2], pos, out)
    ids = torch.tensor([[-5, 2], [3, 6 + 7]], device="cuda")
    _C.rq_embed_step(table, ids, pos, out)
    want = table[ids.clamp(0, 5)[:, 0]] + table[ids.clamp(0, 5)[:, 1]] + pos
    assert torch.equal(out, want)


# ---------------------------------------------------------------------------------------------
# the decode attention over a short cache
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["fp16", "bf16", "f32"])
@pytest.mark.parametrize("B, H", [(1, 1), (11, 3)])      # 33 pairs: a second, partial workgroup
@pytest.mark.parametrize("hs", [64, 192, 384])
def test_short_decode_attention_against_fp64_and_decode_attention(hs, B, H, fmt):
    from enhancing import _C
    dt = H16.get(fmt, torch.float32)
    C = H * hs
    g = _gen(hs + 7 * B)
    label = {"fp16": "rq_short_decode_attn_kernel<F16, false>", "bf16": "rq_short_decode_attn_kernel<BF16, false>",
             "f32": "rq_short_decode_attn_kernel<BF16, true>"}[fmt]
    for Tmax in (2, 3, 8):
        for t in range(Tmax):
            n = t + 1
            qkv = torch.randn(B, 3 * C, generator=g).to(dt).cuda()
            kc = torch.randn(B, H, Tmax, hs, generator=g).to(dt).cuda()
            vc = torch.randn(B, H, Tmax, hs, generator=g).to(dt).cuda()
            kc[:, :, t:], vc[:, :, t:] = float("nan"), float("nan")      # slot t is written, slots > t must never be read
            k0, v0 = kc.clone(), vc.clone()
            out = torch.full((B, C), float("nan"), dtype=dt, device="cuda")
            _C.short_decode_attention(qkv, kc, vc, t, out)
            assert _last() == label
            q, k, v = (z.view(B, H, hs) for z in qkv.split(C, dim=1))
            what = f"short_decode_attention hs={hs} B={B} H={H} Tmax={Tmax} t={t} {fmt}"
            assert torch.equal(kc[:, :, t], k) and torch.equal(vc[:, :, t], v), f"{what}: slot t does not hold the step's k / v"
            assert torch.equal(kc[:, :, :t], k0[:, :, :t]) and torch.equal(vc[:, :, :t], v0[:, :, :t]), f"{what}: older slots changed"
            assert bool(torch.isnan(kc[:, :, t + 1:]).all()) and bool(torch.isnan(vc[:, :, t + 1:]).all()), f"{what}: slots > t were written"
            assert bool(torch.isfinite(out.float()).all()), f"{what}: the output is not finite: a slot > t was read"
            # the truth and the bound of test_gpt_kernels_gpu.py _check_decode_attention: fp64 on the cache contents as stored
            K64, V64, q64 = kc[:, :, :n].double(), vc[:, :, :n].double(), q.double()
            scale = 1.0 / math.sqrt(hs)
            s = torch.einsum("bhd,bhtd->bht", q64, K64) * scale
            p = torch.softmax(s, dim=-1)
            ref = torch.einsum("bht,bhtd->bhd", p, V64).reshape(B, C)
            pav = torch.einsum("bht,bhtd->bhd", p, V64.abs()).reshape(B, C)
            ds = (2 * hs + 8) * E24 * torch.einsum("bhd,bhtd->bht", q64.abs(), K64.abs()).amax(-1) * scale        # [B, H]
            bound = (2 * ds.unsqueeze(-1) + (2 * n + 8) * E24 + 8 * E24).expand(B, H, hs).reshape(B, C) * pav
            if dt in U16:
                bound = bound + U16[dt] * ref.abs() + SUB16.get(dt, 0.0)
            assert_elementwise(out, ref, bound, what)
            # the general kernel on the same inputs: the same cache afterwards, outputs within the two kernels' bounds of each other
            kc2, vc2, out2 = k0.clone(), v0.clone(), torch.full_like(out, float("nan"))
            _C.decode_attention(qkv, kc2, vc2, t, out2)
            bits = torch.int16 if dt in U16 else torch.int32
            assert torch.equal(kc2[:, :, :n].view(bits), kc[:, :, :n].view(bits)) and torch.equal(vc2[:, :, :n].view(bits), vc[:, :, :n].view(bits))
            assert_elementwise(out, out2.double(), 2 * bound, what + " vs decode_attention")
            kc3, vc3, out3 = k0.clone(), v0.clone(), torch.full_like(out, float("nan"))
            _C.short_decode_attention(qkv, kc3, vc3, t, out3)
            assert torch.equal(out.view(bits), out3.view(bits)), f"{what}: bits differ between two calls"


def test_short_decode_attention_refuses_other_shapes():
    from enhancing import _C
    f16 = dict(dtype=torch.float16, device="cuda")
    for hs in (32, 96, 448):
        c = torch.zeros(1, 1, 4, hs, **f16)
        with pytest.raises(RuntimeError, match="multiple of 64 up to 384"):
            _C.short_decode_attention(torch.zeros(1, 3 * hs, **f16), c, c.clone(), 0, torch.empty(1, hs, **f16))
    c = torch.zeros(1, 1, 9, 64, **f16)
    with pytest.raises(RuntimeError, match=r"cache length must be in \[1, 8\]"):
        _C.short_decode_attention(torch.zeros(1, 192, **f16), c, c.clone(), 0, torch.empty(1, 64, **f16))
    c = torch.zeros(1, 1, 4, 64, **f16)
    with pytest.raises(RuntimeError, match="outside the cache"):
        _C.short_decode_attention(torch.zeros(1, 192, **f16), c, c.clone(), 4, torch.empty(1, 64, **f16))
