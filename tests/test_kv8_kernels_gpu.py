"""enh_decode_attention_kv8 and its cursor form (csrc/gpt_decode_kv8.hip): the decode attention over an MXFP8 k / v cache.  Caches are made on the
CPU with tests/mxfp8_util.quant from randn; the truth is fp64 attention over the DEQUANTIZED cache as stored after the call, slot t included, held
to the element bound of tests/test_gpt_kernels_gpu.py::_check_decode_attention unchanged: a 16-bit q times a dequantized code is exact in f32, so
that bound's "f32 chain of hs exact products" model still holds.  The append is held byte for byte to the torch quantizer.  Every slot > t is
pre-filled with the e4m3fn NaN code 0x7f, so reading one poisons the output.  Nothing here is a measured tolerance."""
import math

import pytest
import torch

from mxfp8_util import BLOCK, dequant, quant
from util import SUB16, U16, assert_elementwise

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
E24 = 2.0 ** -24
GUARD, SENT8, NAN8 = 256, 0xA5, 0x7F
LENS = [1, 2, 63, 64, 65, 257, 1024]
# B H >= 512: one piece serves up to 256 slots; 255 | 256 | 257 is that boundary, 513 = three pieces; B H = 256 at len 1024 = four full pieces
LONG_PIECES = [(64, 8, 64, [255, 256, 257, 513]), (16, 16, 64, [1024])]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _guarded_u8(content):
    """(whole allocation, the view of content's shape in its middle): sentinel bytes around a copy of `content` (a CPU uint8 tensor)"""
    n = content.numel()
    whole = torch.full((n + 2 * GUARD,), SENT8, dtype=torch.uint8, device="cuda")
    view = whole[GUARD:GUARD + n].view(content.shape)
    view.copy_(content)
    return whole, view


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENT8).all()) and bool((whole[-GUARD:] == SENT8).all())


def _cache(B, H, Tmax, hs, t, g):
    """(codes [B, H, Tmax, hs], scales [B, H, Tmax, hs / 32]) on the CPU: slots < t quantized from randn, slots >= t NaN codes under a scale of 1"""
    q, s = quant(torch.randn(B * H * Tmax, hs, generator=g))
    q, s = q.view(B, H, Tmax, hs).clone(), s.view(B, H, Tmax, hs // BLOCK).clone()
    q[:, :, t:], s[:, :, t:] = NAN8, 127
    return q, s


def _row_quant(z):
    """[B, C] 16-bit rows of the step -> (codes [B, H.., hs] flattened as [B, C], scales [B, C / 32]) of every head row; blocks never straddle heads"""
    q, s = quant(z.float().cpu().contiguous().view(-1, BLOCK))
    return q.view(z.shape), s.view(z.shape[0], -1)


def _call(qkv, caches, t, out, cursor=None, t_offset=0):
    from enhancing import _C
    if cursor is None:
        _C.decode_attention_kv8(qkv, *caches, t, out)
    else:
        _C.decode_attention_kv8_at(qkv, *caches, torch.tensor([cursor], dtype=torch.int32, device="cuda"), out, t_offset=t_offset)


def _check_append(qkv, before, after, wholes, B, H, hs, t, what):
    """slot t holds the quantized k / v rows byte for byte, slots < t are unchanged, slots > t still hold their NaN codes, the guards are intact"""
    C = H * hs
    k, v = qkv[:, C:2 * C], qkv[:, 2 * C:]
    for (codes0, scales0), (codes, scales), row, name in zip((before[:2], before[2:]), (after[:2], after[2:]), (k, v), ("k", "v")):
        wq, ws = _row_quant(row)
        assert torch.equal(codes[:, :, t].cpu().reshape(B, C), wq), f"{what}: slot {t} of {name}_codes is not quant(the step's {name} row)"
        assert torch.equal(scales[:, :, t].cpu().reshape(B, C // BLOCK), ws), f"{what}: slot {t} of {name}_scales is not quant(the step's {name} row)"
        assert torch.equal(codes[:, :, :t].cpu(), codes0[:, :, :t]) and torch.equal(scales[:, :, :t].cpu(), scales0[:, :, :t]), f"{what}: older {name} slots changed"
        assert torch.equal(codes[:, :, t + 1:].cpu(), codes0[:, :, t + 1:]) and torch.equal(scales[:, :, t + 1:].cpu(), scales0[:, :, t + 1:]), \
            f"{what}: {name} slots > t were written"
    assert all(_guards_intact(w) for w in wholes), f"{what}: a write outside a cache tensor"


def _check(hs, B, H, fmt, lens):
    dt = H16[fmt]
    C = H * hs
    g = _gen(hs + 7 * B)
    for n in lens:
        t, Tmax = n - 1, n + 3
        qkv = torch.randn(B, 3 * C, generator=g).to(dt).cuda()
        kq, ks = _cache(B, H, Tmax, hs, t, g)
        vq, vs = _cache(B, H, Tmax, hs, t, g)
        before = (kq, ks, vq, vs)
        wholes, caches = zip(*[_guarded_u8(z) for z in before])
        out = torch.full((B, C), float("nan"), dtype=dt, device="cuda")
        _call(qkv, caches, t, out)
        what = f"decode_attention_kv8 hs={hs} B={B} H={H} len={n} {fmt}"
        _check_append(qkv, before, caches, wholes, B, H, hs, t, what)
        assert bool(torch.isfinite(out.float()).all()), f"{what}: the output is not finite: a slot > t was read"
        # the truth: fp64 on the dequantized cache contents as stored, slot t included
        deq = lambda q, s: dequant(q[:, :, :n].cpu().reshape(-1, hs), s[:, :, :n].cpu().reshape(-1, hs // BLOCK)).view(B, H, n, hs).double()
        K64, V64 = deq(caches[0], caches[1]), deq(caches[2], caches[3])
        q64 = qkv[:, :C].cpu().view(B, H, hs).double()
        scale = 1.0 / math.sqrt(hs)
        s = torch.einsum("bhd,bhtd->bht", q64, K64) * scale
        p = torch.softmax(s, dim=-1)
        ref = torch.einsum("bht,bhtd->bhd", p, V64).reshape(B, C)
        pav = torch.einsum("bht,bhtd->bhd", p, V64.abs()).reshape(B, C)
        # test_gpt_kernels_gpu.py::_check_decode_attention's bound: scores are an f32 fma chain of hs exact products, a probability is a ratio of
        # exponentials of scores, the f32 sums of n terms run in some fixed order
        ds = (2 * hs + 8) * E24 * torch.einsum("bhd,bhtd->bht", q64.abs(), K64.abs()).amax(-1) * scale        # [B, H]
        bound = (2 * ds.unsqueeze(-1) + (2 * n + 8) * E24 + 8 * E24).expand(B, H, hs).reshape(B, C) * pav
        bound = bound + U16[dt] * ref.abs() + SUB16.get(dt, 0.0)
        assert_elementwise(out, ref, bound, what)
        # a second call from the same start gives the same bits, in the output and in the caches
        wholes2, caches2 = zip(*[_guarded_u8(z) for z in before])
        out2 = torch.full_like(out, float("nan"))
        _call(qkv, caches2, t, out2)
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)), f"{what}: bits differ between two calls"
        assert all(torch.equal(a, b) for a, b in zip(wholes, wholes2)), f"{what}: cache bytes differ between two calls"


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("hs, B, H", [(64, 1, 1), (128, 2, 3), (384, 8, 6)])
def test_decode_attention_kv8_against_fp64(hs, B, H, fmt):
    _check(hs, B, H, fmt, LENS)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("B, H, hs, lens", LONG_PIECES)
def test_decode_attention_kv8_full_pieces_against_fp64(B, H, hs, lens, fmt):
    _check(hs, B, H, fmt, lens)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("B, H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("hs", [64, 128, 384])
def test_append_is_the_torch_quantizer_byte_for_byte(hs, B, H, fmt):
    """random rows, and rows that hold an all-zero block, fp16's largest finite value, an fp16 subnormal and a bf16 value near 1e-38 (an f32
    denormal: the block exponent's clamp); no inf / NaN inputs.  At t = 0 and at the end of a cache of two pieces."""
    dt = H16[fmt]
    C = H * hs
    g = _gen(hs + B + H)
    for t, Tmax in ((0, 1), (70, 140)):
        qkv = torch.randn(B, 3 * C, generator=g)
        tiny = torch.tensor([-3 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -20, -2.0 ** -15] if dt == torch.float16 else [1e-38, -2e-38, 3e-38, 1.2e-38]).repeat(8)
        k, v = (qkv[:, part * C:(part + 1) * C].view(B, H, hs) for part in (1, 2))
        k[:, :, :32] = 0.0                                         # an all-zero block
        k[:, :, 40] = 65504.0                                      # fp16's largest finite value (bf16 rounds it to 65536) among O(1) values
        k[:, :, 41] = tiny[0]                                      # ... and a value the block's scale flushes to zero
        v[:, :, :32] = tiny                                        # a block of fp16 subnormals / of bf16 values near 1e-38 (f32 denormals: the exponent clamp)
        v[:, :, 63] = -65504.0
        qkv = qkv.to(dt).cuda()
        assert bool(torch.isfinite(qkv.float()).all())
        before = _cache(B, H, Tmax, hs, t, g) + _cache(B, H, Tmax, hs, t, g)
        wholes, caches = zip(*[_guarded_u8(z) for z in before])
        out = torch.full((B, C), float("nan"), dtype=dt, device="cuda")
        _call(qkv, caches, t, out)
        _check_append(qkv, before, caches, wholes, B, H, hs, t, f"append hs={hs} B={B} H={H} t={t} {fmt}")
        assert bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_cursor_form_equals_the_by_value_form(fmt):
    """at t in {0, 1, 64, Tmax - 1}, reached through the cursor alone and through t_offset: the same bits in the output and in all four cache
    tensors, guards included"""
    dt = H16[fmt]
    B, H, hs, Tmax = 2, 3, 128, 130
    C = H * hs
    g = _gen(11)
    for t in (0, 1, 64, Tmax - 1):
        qkv = torch.randn(B, 3 * C, generator=g).to(dt).cuda()
        before = _cache(B, H, Tmax, hs, t, g) + _cache(B, H, Tmax, hs, t, g)
        res = []
        for cursor, off in ((None, 0), (t, 0), (t - 5, 5), (t + 3, -3)):
            wholes, caches = zip(*[_guarded_u8(z) for z in before])
            out = torch.full((B * C + 2 * GUARD,), 777.0, dtype=dt, device="cuda")
            _call(qkv, caches, t, out[GUARD:GUARD + B * C].view(B, C), cursor=cursor, t_offset=off)
            res.append((out, wholes))
        for (o, ws), how in zip(res[1:], ("cursor", "t_offset 5", "t_offset -3")):
            assert torch.equal(o.view(torch.int16), res[0][0].view(torch.int16)), (how, t, "out")
            assert all(torch.equal(a, b) for a, b in zip(ws, res[0][1])), (how, t, "cache bytes")
        assert bool(torch.isfinite(res[0][0].float()).all()) and not bool((res[0][0][GUARD:GUARD + B * C] == 777.0).any())


def test_a_cursor_outside_the_cache_writes_nothing():
    from enhancing import _C
    B, H, hs, Tmax = 2, 2, 64, 200
    C = H * hs
    g = _gen(12)
    qkv = torch.randn(B, 3 * C, generator=g).half().cuda()
    ws = _C._workspace(_C.lib().enh_decode_attention_workspace_bytes(B, H, hs, Tmax), qkv.device)
    for cursor, off in ((-1, 0), (Tmax, 0), (Tmax - 1, 1), (0, -1), (2 ** 31 - 1, 5)):
        before = _cache(B, H, Tmax, hs, 0, g) + _cache(B, H, Tmax, hs, 0, g)
        wholes, caches = zip(*[_guarded_u8(z) for z in before])
        keep = [w.clone() for w in wholes]
        out = torch.full((B, C), 777.0, dtype=torch.float16, device="cuda")
        ws.fill_(SENT8)
        _call(qkv, caches, None, out, cursor=cursor, t_offset=off)
        assert bool((out == 777.0).all()) and all(torch.equal(a, b) for a, b in zip(wholes, keep)) and bool((ws == SENT8).all()), (cursor, off)


def test_every_launch_names_its_kernel():
    from enhancing import _C
    last = lambda: _C.lib().enh_last_kernel().decode()
    g = _gen(13)
    for fmt, tag in (("fp16", "F16"), ("bf16", "BF16")):
        qkv = torch.randn(1, 3 * 64, generator=g).to(H16[fmt]).cuda()
        caches = [z.cuda() for z in _cache(1, 1, 4, 64, 0, g) + _cache(1, 1, 4, 64, 0, g)]
        out = torch.empty(1, 64, dtype=H16[fmt], device="cuda")
        _call(qkv, caches, 0, out)
        assert last() == f"gpt_decode_attn_kv8_kernel<{tag}>"
        _call(qkv, caches, None, out, cursor=1)
        assert last() == f"gpt_decode_attn_kv8_at_kernel<{tag}>"


def test_refusals():
    from enhancing import _C
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int32, device="cuda")

    def both(qkv, kc, ks, vc, vs, out, match):
        with pytest.raises(RuntimeError, match=match):
            _C.decode_attention_kv8(qkv, kc, ks, vc, vs, 0, out)
        with pytest.raises(RuntimeError, match=match):
            _C.decode_attention_kv8_at(qkv, kc, ks, vc, vs, cur, out)

    h = lambda *shape: torch.zeros(*shape, dtype=torch.float16, device="cuda")
    both(h(1, 3 * 96), u8(1, 1, 4, 96), u8(1, 1, 4, 3), u8(1, 1, 4, 96), u8(1, 1, 4, 3), h(1, 96), "multiple of 64 up to 384")       # hs = 96
    both(torch.zeros(1, 3 * 64, device="cuda"), u8(1, 1, 4, 64), u8(1, 1, 4, 2), u8(1, 1, 4, 64), u8(1, 1, 4, 2), torch.zeros(1, 64, device="cuda"),
         "bf16 or fp16")                                                                                                           # an f32 qkv
    both(h(1, 3 * 64), u8(1, 1, 4, 64), u8(1, 1, 4, 64), u8(1, 1, 4, 64), u8(1, 1, 4, 2), h(1, 64), "do not fit")                     # k_scales per element
    both(h(1, 3 * 64), u8(1, 1, 4, 64), u8(1, 1, 4, 2), u8(1, 1, 4, 64), u8(1, 1, 3, 2), h(1, 64), "do not fit")                      # v_scales one slot short
    with pytest.raises(RuntimeError, match="outside the cache"):
        _C.decode_attention_kv8(h(1, 3 * 64), u8(1, 1, 4, 64), u8(1, 1, 4, 2), u8(1, 1, 4, 64), u8(1, 1, 4, 2), 4, h(1, 64))
