"""enh_kv_cache_fill and enh_kv_cache_fill_kv8 (csrc/gpt_prefill_cache.hip): the k / v rows of whole sequences put into the caches of the decode
attention in one launch.  Everything here is an equality of bits or bytes: against the torch gather of the k / v columns, against the caches
that S successive decode-attention calls leave, against tests/mxfp8_util.py (the specification of the quantizer) and its exact dequantization.
Caches and their surroundings are pre-filled with sentinels, so a write outside the slots [slot0, slot0 + S) shows.  Nothing is a measured
tolerance."""
import ctypes

import pytest
import torch

from mxfp8_util import BLOCK, dequant, quant

pytestmark = pytest.mark.gpu
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
SENT = {torch.int16: 0x3C5A, torch.int32: 0x3F8A5A5A}      # finite in every format (about 1.1): a decode attention may read it
GUARD, SENT8 = 256, 0xA5
#         B  H  hs   S   Tmax slot0
SHAPES = [(1, 1, 64, 1, 1, 0), (2, 3, 64, 5, 9, 0), (3, 2, 384, 130, 131, 1), (2, 1, 128, 7, 16, 9)]


def _rows(B, S, C, dt, seed):
    """qkv [B S, 3C] in dt: Gaussian rows at three magnitudes (so the block exponents differ), with one all-zero block of 32 in a k column"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * S, 3 * C, generator=g) * torch.tensor([1.0, 8.0, 0.25])[torch.arange(B * S) % 3].unsqueeze(1)
    x[0, C:C + BLOCK] = 0.0
    return x.to(dt).cuda()


def _guarded(shape, dtype, fill):
    """(whole allocation, the view of `shape` in its middle), every element the sentinel `fill`"""
    n = 1
    for d in shape:
        n *= d
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n].view(shape)


def _gather(qkv, B, S, H, hs):
    """(k, v) [B, H, S, hs]: the k and v columns of the packed rows, as the caches hold them"""
    C = H * hs
    return tuple(qkv[:, j * C:(j + 1) * C].reshape(B, S, H, hs).permute(0, 2, 1, 3).contiguous() for j in (1, 2))


@pytest.mark.parametrize("fmt", list(DTYPES))
@pytest.mark.parametrize("B, H, hs, S, Tmax, slot0", SHAPES)
def test_fill_is_the_gather_bit_for_bit_and_touches_nothing_else(B, H, hs, S, Tmax, slot0, fmt):
    from enhancing import _C
    dt, C = DTYPES[fmt], H * hs
    bits = BITS[dt]
    qkv = _rows(B, S, C, dt, 11 + hs + S)
    keep = qkv.clone()
    (wk, kc), (wv, vc) = (_guarded((B, H, Tmax, hs), bits, SENT[bits]) for _ in range(2))
    _C.kv_cache_fill(qkv, S, kc.view(dt), vc.view(dt), slot0=slot0)
    assert torch.equal(qkv.view(bits), keep.view(bits)), "qkv was written"
    for cache, whole, want, name in zip((kc, vc), (wk, wv), _gather(qkv, B, S, H, hs), "kv"):
        assert torch.equal(cache[:, :, slot0:slot0 + S], want.view(bits)), f"{name}: slots [{slot0}, {slot0 + S}) are not the {name} columns"
        other = torch.cat([cache[:, :, :slot0], cache[:, :, slot0 + S:]], 2)
        assert bool((other == SENT[bits]).all()), f"{name}: a slot outside [{slot0}, {slot0 + S}) was written"
        assert bool((whole[:GUARD] == SENT[bits]).all()) and bool((whole[-GUARD:] == SENT[bits]).all()), f"{name}: a write outside the cache"
    if dt == torch.float32:
        return
    # what S successive decode attentions append, one row per batch element and call
    (_, k2), (_, v2) = (_guarded((B, H, Tmax, hs), bits, SENT[bits]) for _ in range(2))
    out = torch.empty(B, C, dtype=dt, device="cuda")
    for s in range(S):
        _C.decode_attention(qkv.view(B, S, 3 * C)[:, s].contiguous(), k2.view(dt), v2.view(dt), slot0 + s, out)
    assert torch.equal(kc, k2) and torch.equal(vc, v2), "one fill and S successive decode_attention calls leave different caches"


def _kv8_caches(B, H, Tmax, hs):
    wholes, views = zip(*[_guarded((B, H, Tmax, n), torch.uint8, SENT8) for n in (hs, hs // BLOCK, hs, hs // BLOCK)])
    return wholes, views


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
@pytest.mark.parametrize("hs", [64, 128, 384])
@pytest.mark.parametrize("B, H, S, Tmax, slot0", [(b, h, s, t, s0) for b, h, _, s, t, s0 in SHAPES])
def test_kv8_fill_is_the_quantizer_the_append_and_the_exact_write_back(B, H, S, Tmax, slot0, hs, fmt):
    from enhancing import _C
    dt, C = DTYPES[fmt], H * hs
    qkv = _rows(B, S, C, dt, 5 + hs + S)
    keep = qkv.clone()
    if dt == torch.float16:      # the write-back's exactness holds from a block amax of 2^-7 on (or for a block of zeros)
        amax = keep[:, C:].float().view(-1, BLOCK).abs().amax(-1)
        assert bool(((amax >= 2.0 ** -7) | (amax == 0)).all())
    wholes, caches = _kv8_caches(B, H, Tmax, hs)
    _C.kv_cache_fill_kv8(qkv, S, *caches, slot0=slot0)
    what = f"kv_cache_fill_kv8 B={B} H={H} hs={hs} S={S} Tmax={Tmax} slot0={slot0} {fmt}"
    assert torch.equal(qkv[:, :C].view(torch.int16), keep[:, :C].view(torch.int16)), f"{what}: the q columns changed"
    for j, (rows, name) in enumerate(zip(_gather(keep, B, S, H, hs), "kv")):
        codes, scales = caches[2 * j], caches[2 * j + 1]
        wq, ws = quant(rows.float().cpu().reshape(-1, hs))
        wq, ws = wq.view(B, H, S, hs), ws.view(B, H, S, hs // BLOCK)
        assert torch.equal(codes[:, :, slot0:slot0 + S].cpu(), wq), f"{what}: {name} codes are not quant(the rows)"
        assert torch.equal(scales[:, :, slot0:slot0 + S].cpu(), ws), f"{what}: {name} scales are not quant(the rows)"
        for z in (codes, scales):
            other = torch.cat([z[:, :, :slot0], z[:, :, slot0 + S:]], 2)
            assert bool((other == SENT8).all()), f"{what}: a {name} slot outside [{slot0}, {slot0 + S}) was written"
        # the k / v columns now hold what the slots hold: the exact dequantization, which the format holds without another rounding
        deq = dequant(wq.view(-1, hs), ws.view(-1, hs // BLOCK)).view(B, H, S, hs).permute(0, 2, 1, 3).reshape(B * S, C)
        back = qkv[:, (1 + j) * C:(2 + j) * C].cpu()
        assert torch.equal(back.float(), deq), f"{what}: the {name} columns of qkv are not dequant(the slot)"
        assert torch.equal(back.view(torch.int16), deq.to(dt).view(torch.int16))
    for w in wholes:
        assert bool((w[:GUARD] == SENT8).all()) and bool((w[-GUARD:] == SENT8).all()), f"{what}: a write outside a cache tensor"
    # what S successive appends of the decode attention leave (slots < slot0 hold sentinel codes and scales there too: finite garbage it may read)
    _, caches2 = _kv8_caches(B, H, Tmax, hs)
    out = torch.empty(B, C, dtype=dt, device="cuda")
    for s in range(S):
        _C.decode_attention_kv8(keep.view(B, S, 3 * C)[:, s].contiguous(), *caches2, slot0 + s, out)
    assert all(torch.equal(a, b) for a, b in zip(caches, caches2)), f"{what}: one fill and S successive decode_attention_kv8 calls leave different caches"
    # the same bytes on a second run from the same start
    _, caches3 = _kv8_caches(B, H, Tmax, hs)
    again = keep.clone()
    _C.kv_cache_fill_kv8(again, S, *caches3, slot0=slot0)
    assert all(torch.equal(a, b) for a, b in zip(caches, caches3)) and torch.equal(again.view(torch.int16), qkv.view(torch.int16))


@pytest.mark.parametrize("fmt", ["bf16", "fp16"])
def test_a_block_with_a_nan_gets_the_nan_scale(fmt):
    from enhancing import _C
    dt, (B, H, hs, S, Tmax) = DTYPES[fmt], (2, 2, 128, 3, 4)
    C = H * hs
    qkv = _rows(B, S, C, dt, 23)
    qkv[4, C + hs + 40] = float("nan")      # row (b, s) = (1, 1), k, head 1, block 1
    keep = qkv.clone()
    _, caches = _kv8_caches(B, H, Tmax, hs)
    _C.kv_cache_fill_kv8(qkv, S, *caches, slot0=0)
    ks = caches[1].cpu()
    assert int(ks[1, 1, 1, 1]) == 0xFF
    wq, ws = quant(_gather(keep, B, S, H, hs)[0].float().cpu().reshape(-1, hs))
    ws = ws.view(B, H, S, hs // BLOCK).clone()
    got = ks[:, :, :S].clone()
    ws[1, 1, 1, 1] = got[1, 1, 1, 1] = 0
    assert torch.equal(got, ws), "another block's scale changed"
    back = qkv[4, C + hs + 32:C + hs + 64].float()
    assert not bool(torch.isfinite(back).any()), "the block's write-back must not be finite"
    assert bool(torch.isfinite(qkv[4, C + hs + 64:].float()).all()) and bool(torch.isfinite(qkv[4, :C + hs + 32].float()).all())


def test_bad_arguments_return_an_error_not_a_launch():
    from enhancing import _C
    L = _C.lib()
    dt, (B, H, hs, S, Tmax) = torch.bfloat16, (2, 2, 64, 3, 4)
    C = H * hs
    qkv = _rows(B, S, C, dt, 3)
    (wk, kc), (wv, vc) = (_guarded((B, H, Tmax, hs), torch.int16, SENT[torch.int16]) for _ in range(2))
    wholes, caches = _kv8_caches(B, H, Tmax, hs)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fill(B=B, S=S, H=H, hs=hs, Tmax=Tmax, slot0=0, q=p(qkv), k=p(kc)):
        return L.enh_kv_cache_fill(q, B, S, H, hs, Tmax, slot0, k, p(vc), 0, stream)

    def fill8(B=B, S=S, H=H, hs=hs, Tmax=Tmax, slot0=0, q=p(qkv), ks=p(caches[1])):
        return L.enh_kv_cache_fill_kv8(q, B, S, H, hs, Tmax, slot0, p(caches[0]), ks, p(caches[2]), p(caches[3]), 0, stream)

    for f in (fill, fill8):
        assert f(slot0=2) == -2 and "outside the cache" in L.enh_last_error().decode()      # slot0 + S > Tmax
        assert f(slot0=-1) == -2
        assert f(hs=96) == -2 and "multiple of 64" in L.enh_last_error().decode()
        assert f(hs=448) == -2
        assert f(q=None) == -1 and "null pointer" in L.enh_last_error().decode()
    assert fill(k=None) == -1 and fill8(ks=None) == -1
    assert L.enh_kv_cache_fill(p(qkv), B, S, H, hs, Tmax, 0, p(kc), p(vc), 3, stream) == -1          # no such dtype
    assert L.enh_kv_cache_fill_kv8(p(qkv), B, S, H, hs, Tmax, 0, *(p(c) for c in caches), 2, stream) == -1      # the exact mode has no MXFP8 cache
    with pytest.raises(RuntimeError, match="outside the cache"):
        _C.kv_cache_fill(qkv, S, kc.view(dt), vc.view(dt), slot0=Tmax - S + 1)
    with pytest.raises(RuntimeError, match="do not fit"):
        _C.kv_cache_fill(qkv, S + 1, kc.view(dt), vc.view(dt))
    torch.cuda.synchronize()
    assert bool((wk == SENT[torch.int16]).all()) and bool((wv == SENT[torch.int16]).all()) and all(bool((w == SENT8).all()) for w in wholes)
    assert fill() == 0 and fill8() == 0
