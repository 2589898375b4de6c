"""What the stage-2 priors of layers.py (GPT, RQTransformer) and their optimizer (engine/optim.py GPTAdam) share, each stated once: the limits of
the kernels, the launches of one Block over whole sequences forward (`_block_rows`) and backward (`_block_rows_backward`) with the products between
them (`_row_linear`, `_grad_linears`), the launches of one Block in a cached sampling step (`_block_step`) and the product they run (`_step_linear`), the operand copies of a stack of Blocks (`_layer_operands`, `qkv_bias`; MXFP8, MXFP6 and MXFP4: `_layer_operands_mx`), the k / v caches of a sampling chunk and the attention over them (`_kv_caches`, `_step_attention`), the prefill of given codes into those caches (`_prefill_stack` with its
products `_prefill_linear` and buffers `_prefill_buffers`; `Prior._check_prefix`, `_place_prefix`), the flat
parameter layout
(`flat_layout`), a layer's slice of the optimizer's operand arena (`ARENA_LAYER`), and `Prior`, the base class: init, input checks, the
version-keyed operand cache, the one-chunk-at-a-time buffer cache and the two teacher-forced drivers (forward: chunks, cross-entropy rows, mean; forward_backward: chunks under the
saved-activation cap, the loss scale, gradients set in the first chunk and added to in the later ones)."""
import os
from typing import NamedTuple

import torch
import torch.nn as nn

MAX_BATCH = 64          # rows of one decode step (enh_skinny_gemm_h16); larger batches run in chunks
MAX_EMBED = 8192        # enh_row_ln_scale
MAX_VOCAB = 16384       # enh_sample_logits
MAX_HEAD = 384          # enh_decode_attention
MAX_TOKENS = 8192       # enh_decode_attention: slots of the k / v cache
FORWARD_HIDDEN_CAP = 2 << 30   # bytes of forward()'s [chunk T, 4C] hidden activation (f32 + operand copy): shipped size, 6 sequences per chunk
OPERAND_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
SAMPLE_WEIGHTS = ("h16", "fp8", "fp6", "fp4")      # sample(weights=): the Block weights of a decode step as 16-bit operands, or as MXFP8 / MXFP6 / MXFP4 codes and scales
QUANT_WEIGHTS = {"fp8": "MXFP8", "fp6": "MXFP6", "fp4": "MXFP4"}
SAMPLE_CACHES = ("h16", "fp8")       # sample(cache=): the k / v caches of the long decode attention as 16-bit tensors, or as MXFP8 codes and scales

# one layer's slice of GPTAdam's 16-bit operand arena: (operand, the Linear masters that are its row blocks, offset / C^2, rows / C, cols / C)
ARENA_LAYER = (("wqkv", ("attn.query", "attn.key", "attn.value"), 0, 3, 1), ("wproj", ("attn.proj",), 3, 1, 1), ("w0", ("mlp.p0",), 4, 4, 1),
               ("w1", ("mlp.p1",), 8, 1, 4))
ARENA_LAYER_SIZE = sum(r * c for *_, r, c in ARENA_LAYER)      # 12, in units of C^2


def check_limits(who: str, embed_dim: int, heads: dict, cond_num_tokens: int, vocab_img_size: int, img_num_tokens: int) -> None:
    """the shapes the kernels take, as ValueErrors of class `who`; heads: constructor argument -> head count"""
    if cond_num_tokens != 1:
        raise ValueError(f"{who}: cond_num_tokens must be 1 (class conditioning: every sampling step is one token), got {cond_num_tokens}")
    for arg, n in heads.items():
        if embed_dim % n:
            raise ValueError(f"{who}: embed_dim {embed_dim} is not a multiple of {arg} {n}")
        if (embed_dim // n) % 64 or embed_dim // n > MAX_HEAD:
            raise ValueError(f"{who}: the head size embed_dim / {arg} must be a multiple of 64 up to {MAX_HEAD}, got {embed_dim // n}")
    if vocab_img_size > MAX_VOCAB:
        raise ValueError(f"{who}: vocab_img_size must be at most {MAX_VOCAB}, got {vocab_img_size}")
    if embed_dim > MAX_EMBED:
        raise ValueError(f"{who}: embed_dim must be at most {MAX_EMBED}, got {embed_dim}")
    if vocab_img_size % 8:
        raise ValueError(f"{who}: vocab_img_size must be a multiple of 8 (the head's GEMM), got {vocab_img_size}")
    if img_num_tokens > MAX_TOKENS:
        raise ValueError(f"{who}: img_num_tokens must be at most {MAX_TOKENS} (the cache of the decode attention), got {img_num_tokens}")


def flat_layout(module: nn.Module):
    """([(offset, numel) per parameter], total): the flat f32 buffers of gradients, masters and moments (engine/stage1.py ParamStore's layout:
    registration order, every parameter padded to 64 elements)"""
    table, total = [], 0
    for _, p in module.named_parameters():
        table.append((total, p.numel()))
        total += (p.numel() + 63) // 64 * 64
    return table, total


def qkv_bias(attn, out=None):
    """the q | k | v bias concatenation, one f32 vector beside the fused [3C, C] weight (None without biases); out= rewrites an earlier one"""
    if attn.query.bias is None:
        return None
    return torch.cat([lin.bias.detach() for lin in (attn.query, attn.key, attn.value)], out=out).float().contiguous()


def _layer_operands(blocks, cast) -> list:
    """per Block: the fused q|k|v weight and bias, proj, p0 and p1 through `cast`, and time_mix as a flat f32 vector"""
    layers = []
    for blk in blocks:
        a, m = blk.attn, blk.mlp
        layers.append(dict(wqkv=cast(torch.cat([a.query.weight, a.key.weight, a.value.weight], 0)), bqkv=qkv_bias(a), wproj=cast(a.proj.weight),
                           w0=cast(m.p0.weight), w1=cast(m.p1.weight), time_mix=a.time_mix.detach().reshape(-1).contiguous()))
    return layers


def _mxfp8_operand(masters) -> tuple:
    """(codes [N, K] uint8, scales [N, K / 32] uint8): the MXFP8 operand (include/enh_hip.h) whose row blocks are the f32 `masters`, quantized on
    the device straight from them: one rounding, and no 16-bit copy is ever made"""
    from ... import _C
    K = masters[0].shape[1]
    N = sum(m.shape[0] for m in masters)
    codes = torch.empty(N, K, dtype=torch.uint8, device=masters[0].device)
    scales = torch.empty(N, K // _C.MX_BLOCK, dtype=torch.uint8, device=masters[0].device)
    row0 = 0
    for m in masters:
        _C.quantize_mxfp8(m.detach(), codes, scales, row0=row0)
        row0 += m.shape[0]
    return codes, scales


class MXFP4(NamedTuple):
    """the MXFP4 operand of a weight [N, K] (include/enh_hip.h): codes [N, K / 2] uint8, two e2m1 codes per byte, and scales [N, K / 32] uint8"""
    codes: torch.Tensor
    scales: torch.Tensor


def _mxfp4_operand(masters) -> MXFP4:
    """`_mxfp8_operand` in the 4-bit format: quantized on the device straight from the f32 `masters`, no 16-bit or 8-bit copy is ever made"""
    from ... import _C
    K = masters[0].shape[1]
    N = sum(m.shape[0] for m in masters)
    codes = torch.empty(N, K // 2, dtype=torch.uint8, device=masters[0].device)
    scales = torch.empty(N, K // _C.MX_BLOCK, dtype=torch.uint8, device=masters[0].device)
    row0 = 0
    for m in masters:
        _C.quantize_mxfp4(m.detach(), codes, scales, row0=row0)
        row0 += m.shape[0]
    return MXFP4(codes, scales)


class MXFP6(NamedTuple):
    """the MXFP6 operand of a weight [N, K] (include/enh_hip.h): codes [N, 96 ceil(K / 128)] uint8, e2m3 codes in 128-k chunks of 96 bytes in the
    product's order, and scales [N, K / 32] uint8"""
    codes: torch.Tensor
    scales: torch.Tensor


def _mxfp6_operand(masters) -> MXFP6:
    """`_mxfp4_operand` in the 6-bit format: quantized on the device straight from the f32 `masters`, no copy in another format is ever made"""
    from ... import _C
    K = masters[0].shape[1]
    N = sum(m.shape[0] for m in masters)
    codes = torch.empty(N, _C.mxfp6_row_bytes(K), dtype=torch.uint8, device=masters[0].device)
    scales = torch.empty(N, K // _C.MX_BLOCK, dtype=torch.uint8, device=masters[0].device)
    row0 = 0
    for m in masters:
        _C.quantize_mxfp6(m.detach(), codes, scales, row0=row0)
        row0 += m.shape[0]
    return MXFP6(codes, scales)


MX_OPERAND = {"fp8": _mxfp8_operand, "fp6": _mxfp6_operand, "fp4": _mxfp4_operand}


def _layer_operands_mx(blocks, operand) -> list:
    """`_layer_operands` with every Linear weight through `operand` (`_mxfp8_operand`: a (codes, scales) pair, `_mxfp6_operand`: an MXFP6,
    `_mxfp4_operand`: an MXFP4); biases and time_mix stay f32"""
    layers = []
    for blk in blocks:
        a, m = blk.attn, blk.mlp
        layers.append(dict(wqkv=operand([a.query.weight, a.key.weight, a.value.weight]), bqkv=qkv_bias(a), wproj=operand([a.proj.weight]),
                           w0=operand([m.p0.weight]), w1=operand([m.p1.weight]), time_mix=a.time_mix.detach().reshape(-1).contiguous()))
    return layers


# ---- the products --------------------------------------------------------------------------------------------------------------------------
def _step_linear(dt: torch.dtype):
    """linear(inp, w, out, bias, relu_sq, res), the product of a cached sampling step (M <= 64 rows), chosen by the operand it is given: the exact
    mode's f32 form, enh_skinny_gemm_h16 for a 16-bit weight, enh_skinny_gemm_w8 for an MXFP8 (codes, scales) pair, enh_skinny_gemm_w6 for an MXFP6,
    enh_skinny_gemm_w4 for an MXFP4"""
    from ... import _C
    if dt == torch.float32:
        return _C.skinny_gemm_f32

    def linear(inp, w, out, bias=None, relu_sq=False, res=None):
        if isinstance(w, MXFP4):
            _C.skinny_gemm_w4(inp, w.codes, w.scales, out, bias=bias, relu_sq=relu_sq, res=res)
        elif isinstance(w, MXFP6):
            _C.skinny_gemm_w6(inp, w.codes, w.scales, out, bias=bias, relu_sq=relu_sq, res=res)
        elif isinstance(w, tuple):
            _C.skinny_gemm_w8(inp, w[0], w[1], out, bias=bias, relu_sq=relu_sq, res=res)
        else:
            _C.skinny_gemm(inp, w, out, bias=bias, relu_sq=relu_sq, res=res)
    return linear


def _row_linear(M: int, dt: torch.dtype):
    """linear(inp, w, out, bias, res, relu_sq) over the leading M rows: out = inp w^T (+ bias) (+ res) in the operand format `dt`"""
    from ... import _C
    if dt == torch.float32:
        def linear(inp, w, out, bias=None, res=None, relu_sq=False):      # tree-ordered sums: enh_gemm_f32 adds K terms in ascending order
            for m0 in range(0, M, MAX_BATCH):
                m1 = min(m0 + MAX_BATCH, M)
                _C.skinny_gemm_f32(inp[m0:m1], w, out[m0:m1], bias=bias, relu_sq=relu_sq, res=None if res is None else res[m0:m1])
    else:
        def linear(inp, w, out, bias=None, res=None, relu_sq=False):
            N, K = w.shape
            if out.dtype == torch.float32:
                _C.gemm(inp, w, M, N, K, bias=bias, res=res, res_rows=M if res is not None else 0, out_f32=out)
            else:
                _C.gemm(inp, w, M, N, K, bias=bias, out_bf16=out)
    return linear


def _grad_linears(M: int, Mp: int, accumulate: bool):
    """(wgrad, dgrad), the two products of a linear layer's backward over a chunk of M rows in buffers of Mp = M rounded up to 8 (the contraction
    length of a weight-gradient product; the tail rows of its operands are zero)"""
    from ... import _C

    def wgrad(dy, inp, grad, n_out: int, k_in: int, lda=None):      # grad [n_out, k_in] (+)= dy^T inp over the chunk's Mp rows
        _C.gemm(dy, inp, n_out, k_in, Mp, trans_a=True, trans_b=True, accumulate=accumulate, out_f32=grad, lda=lda, ldb=k_in)

    def dgrad(dy, w, out):      # out [M, K] = dy [M, N] w [N, K]
        N, K = w.shape
        if out.dtype == torch.float32:
            _C.gemm(dy, w, M, K, N, trans_b=True, out_f32=out)
        else:
            _C.gemm(dy, w, M, K, N, trans_b=True, out_bf16=out)
    return wgrad, dgrad


# ---- one Block over whole sequences --------------------------------------------------------------------------------------------------------
def _block_rows(blk, W, linear, dt, S: int, attention, x, x_out, a, a2, qkv, att, x2, hid32, hid) -> None:
    """the launches of one Block over whole sequences of S rows: x -> x_out (both f32).  attention(qkv, att) is the block's causal attention."""
    from ... import _C
    _C.ln_timeshift(x, blk.ln1.weight, blk.ln1.bias, a, S, colscale=W["time_mix"], eps=blk.ln1.eps)
    linear(a, W["wqkv"], qkv, bias=W["bqkv"])
    attention(qkv, att)
    linear(att, W["wproj"], x2, bias=blk.attn.proj.bias, res=x)
    _C.ln_timeshift(x2, blk.ln2.weight, blk.ln2.bias, a2, S, eps=blk.ln2.eps)
    if dt == torch.float32:
        linear(a2, W["w0"], hid32, bias=blk.mlp.p0.bias, relu_sq=True)
        linear(hid32, W["w1"], x_out, bias=blk.mlp.p1.bias, res=x2)
    else:
        # relu^2 on the f32 product, one rounding to the operand format (in place on a 16-bit product it would be two)
        linear(a2, W["w0"], hid32, bias=blk.mlp.p0.bias)
        _C.relu_sq(hid, hid32)
        linear(hid, W["w1"], x_out, bias=blk.mlp.p1.bias, res=x2)


def _kv_caches(n_layers: int, b: int, H: int, T: int, hs: int, dt: torch.dtype, dev, cache: str) -> list:
    """per layer the k / v cache of enh_decode_attention: under "h16" the pair (k, v) [b, H, T, hs] in the operand format, under "fp8" the MXFP8
    form (k_codes, k_scales, v_codes, v_scales), codes [b, H, T, hs] and scales [b, H, T, hs / 32] uint8 (include/enh_hip.h): no 16-bit tensor"""
    if cache != "fp8":
        return [(torch.empty(b, H, T, hs, dtype=dt, device=dev), torch.empty(b, H, T, hs, dtype=dt, device=dev)) for _ in range(n_layers)]
    from ... import _C
    u8 = lambda n: torch.empty(b, H, T, n, dtype=torch.uint8, device=dev)
    return [(u8(hs), u8(hs // _C.MX_BLOCK), u8(hs), u8(hs // _C.MX_BLOCK)) for _ in range(n_layers)]


def _step_attention(t, cursor=None):
    """attend(qkv, kv, out), the attention of a cached sampling step over the long cache `kv` of one layer (`_kv_caches`), at step t or, in the
    cursor form, at the step the device int32 `cursor` holds: enh_decode_attention for a 16-bit (k, v) pair, enh_decode_attention_kv8 for the four
    tensors of an MXFP8 cache"""
    from ... import _C
    if cursor is not None:
        return lambda q, kv, o: (_C.decode_attention_kv8_at if len(kv) == 4 else _C.decode_attention_at)(q, *kv, cursor, o)
    return lambda q, kv, o: (_C.decode_attention_kv8 if len(kv) == 4 else _C.decode_attention)(q, *kv, t, o)


def _block_step(blk, W, linear, attention, x, x2, a, qkv, att, hid) -> None:
    """the launches of one Block in a cached sampling step, one row per batch element: x -> x (f32, in place).  The Block sees T == 1, so
    time_shift is all zeros and the mix is ln1(x) * time_mix.  linear is enh_skinny_gemm_h16 or, in the exact mode, its f32 form;
    attention(qkv, att) appends the step's k / v to the layer's cache and attends over it."""
    from ... import _C
    _C.row_ln_scale(x, blk.ln1.weight, blk.ln1.bias, a, colscale=W["time_mix"], eps=blk.ln1.eps)
    linear(a, W["wqkv"], qkv, bias=W["bqkv"])
    attention(qkv, att)
    linear(att, W["wproj"], x2, bias=blk.attn.proj.bias, res=x)
    _C.row_ln_scale(x2, blk.ln2.weight, blk.ln2.bias, a, eps=blk.ln2.eps)
    linear(a, W["w0"], hid, bias=blk.mlp.p0.bias, relu_sq=True)
    linear(hid, W["w1"], x, bias=blk.mlp.p1.bias, res=x2)


# ---- the prefill of a sampling chunk: given codes put into the caches ------------------------------------------------------------------
def _prefill_linear(M: int, dt: torch.dtype):
    """linear(inp, w, out, bias, res, relu_sq) over the M rows of a prefill: `_row_linear` for a 16-bit or (exact mode) f32 weight; for an MXFP8 /
    MXFP6 / MXFP4 operand the step's own product (`_step_linear`) in pieces of at most MAX_BATCH rows, which re-reads the codes once per piece and
    builds no 16-bit copy of the weight"""
    rows = _row_linear(M, dt)
    if dt == torch.float32:
        return rows
    step = _step_linear(dt)

    def linear(inp, w, out, bias=None, res=None, relu_sq=False):
        if not isinstance(w, tuple):      # (MXFP6 and MXFP4 are NamedTuples, MXFP8 a plain pair)
            return rows(inp, w, out, bias=bias, res=res, relu_sq=relu_sq)
        for m0 in range(0, M, MAX_BATCH):
            m1 = min(m0 + MAX_BATCH, M)
            step(inp[m0:m1], w, out[m0:m1], bias=bias, relu_sq=relu_sq, res=None if res is None else res[m0:m1])
    return linear


def _prefill_buffers(b: int, P: int, C: int, dt: torch.dtype, dev, hidden_cap: int) -> dict:
    """the buffers of a prefill of b sequences of P rows, apart from the b-row buffers of the steps: g, the whole sequences of one group, sized so
    that the [g P, 4C] hidden activation (f32 and its operand copy) stays under `hidden_cap` bytes, and `_block_rows`' buffers at g P rows"""
    f32 = torch.float32
    g = max(1, min(b, int(hidden_cap) // (P * 4 * C * (4 + (2 if dt != f32 else 0)))))
    M = g * P
    e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
    return dict(g=g, x=e(M, C, dtype=f32), x2=e(M, C, dtype=f32), a=e(M, C), qkv=e(M, 3 * C), att=e(M, C), hid32=e(M, 4 * C, dtype=f32),
                hid=e(M, 4 * C) if dt != f32 else None)


def _prefill_stack(blocks, layers, caches, b0: int, n: int, P: int, H: int, dt: torch.dtype, pf: dict) -> None:
    """rows s = 0 .. P - 1 of n sequences, built in pf["x"] [n P, C], through a stack of Blocks under the SAMPLER's model: under
    the cache time_shift is zero in every Block, so every row is ln1(x) * time_mix with no previous-row term, which is enh_ln_timeshift at S = 1
    over all rows.  Per layer `_block_rows`' launches at S = 1 with the fill of slots 0 .. P - 1 of caches[layer][b0 : b0 + n] (`_kv_caches`:
    enh_kv_cache_fill, or for an MXFP8 cache enh_kv_cache_fill_kv8, which also leaves in qkv what the slots now hold) in front of the causal
    attention over N = P.  The last layer stops behind its fill: nothing of it is needed any more."""
    from ... import _C
    M = n * P
    x, x2, a, qkv, att, hid32, hid = (None if pf[k] is None else pf[k][:M] for k in ("x", "x2", "a", "qkv", "att", "hid32", "hid"))
    hs = x.shape[1] // H
    linear = _prefill_linear(M, dt)

    def fill(kv):
        (_C.kv_cache_fill_kv8 if len(kv) == 4 else _C.kv_cache_fill)(qkv, P, *(c[b0:b0 + n] for c in kv))

    for i, (blk, W, kv) in enumerate(zip(blocks, layers, caches)):
        if i == len(blocks) - 1:
            _C.ln_timeshift(x, blk.ln1.weight, blk.ln1.bias, a, 1, colscale=W["time_mix"], eps=blk.ln1.eps)
            linear(a, W["wqkv"], qkv, bias=W["bqkv"])
            fill(kv)
            return

        def attention(q, o, kv=kv):
            fill(kv)
            _C.causal_attention(q, n, P, H, hs, o)

        _block_rows(blk, W, linear, dt, 1, attention, x, x, a, a, qkv, att, x2, hid32, hid)


def _block_rows_backward(blk, W, wgrad, dgrad, accumulate: bool, S: int, attention_backward, sv, st, g, g2, d32, g16, dh16, dqkv, datt, hid32) -> None:
    """the backward of _block_rows, setting (accumulate=False) or adding to the Block's parameter gradients.  sv: what the forward
    kept of the layer (x, a, qkv, att, lse, x2, a2, hid); st: the chunk's gradient buffers at their full Mp rows, which the weight-gradient
    products contract over; g .. hid32: their leading M rows.  In: g, the f32 gradient of the Block's output, and g16, its operand copy; out: the
    same two for the Block's input.  attention_backward(sv, datt, dqkv) is the backward of the block's causal attention."""
    from ... import _C
    at, ml = blk.attn, blk.mlp
    M, C = g.shape
    # p1, relu^2, p0
    wgrad(st["g16"], sv["hid"], ml.p1.weight.grad, C, 4 * C)
    if ml.p1.bias is not None:
        _C.colsum(g16, M, C, ml.p1.bias.grad, accumulate)
    dgrad(g16, W["w1"], hid32)
    _C.relu_sq_backward(hid32, sv["hid"][:M], dh16)
    wgrad(st["dh16"], sv["a2"], ml.p0.weight.grad, 4 * C, C)
    if ml.p0.bias is not None:
        _C.colsum(dh16, M, 4 * C, ml.p0.bias.grad, accumulate)
    dgrad(dh16, W["w0"], d32)
    _C.ln_timeshift_backward(d32, sv["x2"][:M], blk.ln2.weight, S, g2, blk.ln2.weight.grad, blk.ln2.bias.grad, dres=g, dx16=g16, eps=blk.ln2.eps,
                             accumulate=accumulate)
    # proj, attention, q | k | v
    wgrad(st["g16"], sv["att"], at.proj.weight.grad, C, C)
    if at.proj.bias is not None:
        _C.colsum(g16, M, C, at.proj.bias.grad, accumulate)
    dgrad(g16, W["wproj"], datt)
    attention_backward(sv, datt, dqkv)
    flat = st["dqkv"].view(-1)      # the gradient of the fused [3C, C] operand, split back: column block j of dqkv is lin's output gradient
    for j, lin in enumerate((at.query, at.key, at.value)):
        wgrad(flat[j * C:], sv["a"], lin.weight.grad, C, C, lda=3 * C)
    if at.query.bias is not None:
        _C.colsum(dqkv, M, 3 * C, st["dbqkv"], False)
        for j, lin in enumerate((at.query, at.key, at.value)):
            if accumulate:
                lin.bias.grad.add_(st["dbqkv"][j * C:(j + 1) * C])
            else:
                lin.bias.grad.copy_(st["dbqkv"][j * C:(j + 1) * C])
    dgrad(dqkv, W["wqkv"], d32)
    _C.ln_timeshift_backward(d32, sv["x"][:M], blk.ln1.weight, S, g, blk.ln1.weight.grad, blk.ln1.bias.grad, b=blk.ln1.bias, colscale=W["time_mix"],
                             dcolscale=at.time_mix.grad.view(-1), dres=g2, dx16=g16, eps=blk.ln1.eps, accumulate=accumulate)


class Prior(nn.Module):
    """the chassis under GPT and RQTransformer.  A subclass registers its parameters (the registration order is the flat layout), names its
    stacks of Blocks in STACKS (operand key -> attribute) and gives `_forward_buffers` and `_forward_rows`."""
    STACKS = {}

    def __init__(self, vocab_cond_size: int, vocab_img_size: int, embed_dim: int, cond_num_tokens: int, img_num_tokens: int, **heads) -> None:
        super().__init__()
        check_limits(type(self).__name__, embed_dim, heads, cond_num_tokens, vocab_img_size, img_num_tokens)
        self.img_num_tokens = img_num_tokens
        self.vocab_cond_size = vocab_cond_size
        self.vocab_img_size = vocab_img_size
        self.embed_dim = embed_dim
        self._operands = {}       # operand format -> (versions of the masters, operand copies)
        self._fwd_states = {}     # (chunk, dtype, device) -> the buffers of forward()
        self.forward_hidden_cap = FORWARD_HIDDEN_CAP
        self._arena = None        # set by engine/optim.py GPTAdam: dict(dt, ptrs, ops, versions, refresh) — the operand arena its step kernel keeps current
        self._grad_key = None     # the parameters whose .grad are views into flat_grad
        self.flat_grad = None
        self._sample_stream = None    # sample(graph=True): the side stream its chunks are captured and replayed on
        self._sample_keep = None      # ... and what the last call's graphs point at (_sample_graphed)

    def _init_weights(self, module: nn.Module) -> None:
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if isinstance(module, nn.Linear) and module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    def _block_stacks(self) -> dict:
        """operand key -> (attribute name, the nn.Sequential of Blocks)"""
        return {key: (attr, getattr(self, attr)) for key, attr in self.STACKS.items()}

    # ---- what the entries begin with --------------------------------------------------------------
    def _on_device_conds(self, conds: torch.Tensor, B: int, who: str) -> torch.Tensor:
        """moves a module whose parameters are elsewhere to the device of `conds`; returns the [B] int64 column of the one condition token per row"""
        if self.head.weight.device != conds.device:
            self.to(conds.device)
        conds = conds.reshape(B, -1)
        if conds.shape[1] != 1:
            raise ValueError(f"{who}: one condition token per row (cond_num_tokens == 1), got {conds.shape[1]}")
        return conds[:, 0].to(torch.int64).contiguous()

    @staticmethod
    def _operand_dtype(use_fp16: bool, who: str) -> torch.dtype:
        """use_fp16 -> the 16-bit operand format of ENH_PRECISION (default fp16), else f32: the exact mode"""
        if not use_fp16:
            return torch.float32
        prec = os.environ.get("ENH_PRECISION", "fp16")
        if prec not in OPERAND_DTYPE:
            raise ValueError(f"{who}(use_fp16=True): ENH_PRECISION must be 'fp16' or 'bf16' for the 16-bit mode, got {prec!r}")
        return OPERAND_DTYPE[prec]

    def _check_inputs(self, codes, conds, who: str, why: str = "there is no CPU path"):
        """what the teacher-forced entries accept: device tensors, returned as (codes [B, T] int64, or [B, T, D] where the class has a depth_num_tokens,
        conds [B] int64), ranges checked"""
        if not (torch.is_tensor(codes) and torch.is_tensor(conds) and codes.is_cuda and conds.is_cuda):
            raise NotImplementedError(f"{who} runs on a ROCm device only: codes and conds must be device tensors ({why})")
        B, T, V, D = codes.shape[0], self.img_num_tokens, self.vocab_img_size, getattr(self, "depth_num_tokens", None)
        if D is not None:
            if codes.shape[-1] != D or codes.numel() != B * T * D:
                raise ValueError(f"{who}: codes must be [B, img_num_tokens = {T}, depth_num_tokens = {D}], got {tuple(codes.shape)}")
            codes = codes.reshape(B, T, D).to(torch.int64).contiguous()
        else:
            codes = codes.reshape(B, -1).to(torch.int64).contiguous()
            if codes.shape[1] != T:
                raise ValueError(f"{who}: codes must hold img_num_tokens = {T} codes per row, got {codes.shape[1]}")
        conds = self._on_device_conds(conds, B, who)
        if int(codes.min()) < 0 or int(codes.max()) >= V:
            raise ValueError(f"{who}: codes outside [0, {V})")
        if int(conds.min()) < 0 or int(conds.max()) >= self.vocab_cond_size:
            raise ValueError(f"{who}: conds outside [0, {self.vocab_cond_size})")
        return codes, conds

    def _check_prefix(self, prefix, B: int, who: str):
        """sample(prefix_codes=): anything with B rows that reshapes to [B, P] (or [B, P, D] where the class has a depth_num_tokens, its last axis D)
        with 0 <= P < img_num_tokens and ids in [0, V), returned as int64 where it lives (None for P == 0: the call is then the one without a prefix);
        a ValueError otherwise.  Nothing here looks at the device unless the prefix is there: the range check reads the ids where they are."""
        if prefix is None:
            return None
        T, V, D = self.img_num_tokens, self.vocab_img_size, getattr(self, "depth_num_tokens", None)
        prefix = torch.as_tensor(prefix)
        shape = "[B, P, depth_num_tokens = %d]" % D if D is not None else "[B, P]"
        if prefix.dim() < 1 or prefix.shape[0] != B or prefix.is_complex():
            raise ValueError(f"{who}: prefix_codes must be {shape} with one row per row of conds (B = {B}), got {tuple(prefix.shape)}")
        if D is not None and (prefix.dim() < 2 or prefix.shape[-1] != D):
            raise ValueError(f"{who}: prefix_codes must be {shape} (every given position holds all its codes), got {tuple(prefix.shape)}")
        P = prefix.numel() // max(B * (D or 1), 1)
        if P >= T:
            raise ValueError(f"{who}: prefix_codes gives {P} of the img_num_tokens = {T} positions: at least one must be left to draw (0 <= P < {T})")
        if P == 0:
            return None
        prefix = prefix.reshape((B, P) if D is None else (B, P, D)).to(torch.int64)
        if int(prefix.min()) < 0 or int(prefix.max()) >= V:
            raise ValueError(f"{who}: prefix_codes outside [0, {V})")
        return prefix

    def _place_prefix(self, prefix, forced, codes, logits, who: str):
        """the prefix on the device of `codes`, checked once against forced_codes (whose first P positions must be the prefix: a ValueError), written
        into codes[:, :P]; the logits of the given positions, which are not computed, are set to NaN"""
        prefix = prefix.to(codes.device).contiguous()
        P = prefix.shape[1]
        if forced is not None and not torch.equal(forced[:, :P], prefix):
            raise ValueError(f"{who}: forced_codes and prefix_codes disagree in the first {P} positions")
        codes[:, :P] = prefix
        if logits is not None:
            logits.view(codes.shape[0], self.img_num_tokens, -1)[:, :P] = float("nan")
        return prefix

    # ---- caches -----------------------------------------------------------------------------------
    def _chunk_state(self, cache: str, build, b: int, dt: torch.dtype, dev) -> dict:
        """build(b, dt, dev), the buffers of a chunk of b batch items, kept in the dict attribute `cache` from call to call; a shorter last chunk
        uses their leading rows.  One chunk size at a time: the buffers of a shipped-size chunk are gigabytes"""
        key = (b, dt, str(dev))
        if key not in getattr(self, cache):
            setattr(self, cache, {key: build(b, dt, dev)})
        return getattr(self, cache)[key]

    def _operand_copies(self, dt: torch.dtype):
        """the GEMM weights in the operand format `dt` (torch.float32: the exact mode's packed f32 q|k|v): per stack of STACKS its
        `_layer_operands`, and the head.  Built once from the fp32 masters and rebuilt when a master was replaced or written in place
        (load_state_dict): the masters' version counters are the key.  Under a GPTAdam (`_arena`) the 16-bit operands are views into the
        optimizer's arena, which its step kernel rewrites with the masters: nothing is rebuilt, and a module whose parameters were moved or
        replaced since, or whose operand format changed, is refused."""
        ar, who = self._arena, type(self).__name__
        if ar is not None and dt != torch.float32:
            if dt != ar["dt"]:
                raise RuntimeError(f"{who}: the optimizer's operand arena holds {ar['dt']} but the engine's operand format (ENH_PRECISION) is now {dt}: "
                                   "build a new GPTAdam (configure_optimizers) under the format you train in")
            if tuple(p.data_ptr() for p in self.parameters()) != ar["ptrs"]:
                raise RuntimeError(f"{who}: the parameters were moved or replaced after GPTAdam was built (.to(), .half(), assigning .data): the "
                                   "optimizer's flat buffers and operand arena no longer belong to them; build a new GPTAdam (configure_optimizers)")
            if tuple(p._version for p in self.parameters()) != ar["versions"]:      # torch wrote a master in place (load_state_dict): recast the arena
                ar["refresh"]()
            return ar["ops"]
        masters = [p for _, p in sorted(self.named_parameters())]
        key = tuple((p.data_ptr(), p._version) for p in masters)
        hit = self._operands.get(dt)
        if hit is not None and hit[0] == key:
            return hit[1]
        cast = (lambda w: w.detach().to(dt).contiguous())
        ops = {k: _layer_operands(stack, cast) for k, (_, stack) in self._block_stacks().items()}
        ops["head"] = cast(self.head.weight)
        self._operands[dt] = (key, ops)
        return ops

    @staticmethod
    def _sample_weights(weights, use_fp16: bool, who: str) -> str:
        """sample(weights=): None reads ENH_SAMPLE_WEIGHTS (default "h16"); "fp8", "fp6" and "fp4" need the 16-bit mode (their activations are 16-bit operands)"""
        if weights is None:
            weights = os.environ.get("ENH_SAMPLE_WEIGHTS", "h16")
        if weights not in SAMPLE_WEIGHTS:
            raise ValueError(f"{who}: weights (or ENH_SAMPLE_WEIGHTS) must be one of {SAMPLE_WEIGHTS}, got {weights!r}")
        if weights in QUANT_WEIGHTS and not use_fp16:
            raise ValueError(f"{who}: weights=\"{weights}\" streams {QUANT_WEIGHTS[weights]} weights against 16-bit activations; the exact mode (use_fp16=False) has no such form")
        return weights

    @staticmethod
    def _sample_cache(cache, use_fp16: bool, who: str) -> str:
        """sample(cache=): None reads ENH_SAMPLE_CACHE (default "h16"); "fp8" needs the 16-bit mode (q and the step's k / v rows are 16-bit)"""
        if cache is None:
            cache = os.environ.get("ENH_SAMPLE_CACHE", "h16")
        if cache not in SAMPLE_CACHES:
            raise ValueError(f"{who}: cache (or ENH_SAMPLE_CACHE) must be one of {SAMPLE_CACHES}, got {cache!r}")
        if cache == "fp8" and not use_fp16:
            raise ValueError(f"{who}: cache=\"fp8\" quantizes 16-bit k / v rows into an MXFP8 cache; the exact mode (use_fp16=False) has no such form")
        return cache

    def _sample_operands(self, dt: torch.dtype, weights: str):
        """the operands of sample(): `_operand_copies(dt)`, or under weights == "fp8" / "fp6" / "fp4" the MXFP8 / MXFP6 / MXFP4 form, where every Linear of
        every Block is a (codes, scales) pair / an MXFP6 / an MXFP4 and only the head is a 16-bit copy.  Built once on the device from the f32 masters and keyed on
        their data pointers and version counters like the 16-bit copies; building it builds no copy of a Block weight in another format.  Under a
        GPTAdam, whose step kernel writes the masters behind those counters, the optimizer's step drops every entry of `_operands`, so the next
        call rebuilds."""
        if weights not in QUANT_WEIGHTS:
            return self._operand_copies(dt)
        operand = MX_OPERAND[weights]
        masters = [p for _, p in sorted(self.named_parameters())]
        key = tuple((p.data_ptr(), p._version) for p in masters)
        hit = self._operands.get((weights, dt))
        if hit is not None and hit[0] == key:
            return hit[1]
        self._operands.pop((weights, dt), None)      # release the stale copies before their replacements are allocated
        ops = {k: _layer_operands_mx(stack, operand) for k, (_, stack) in self._block_stacks().items()}
        ops["head"] = self.head.weight.detach().to(dt).contiguous()
        self._operands[(weights, dt)] = (key, ops)
        return ops

    def _flat_grads(self, dev) -> torch.Tensor:
        """one flat f32 buffer that every parameter's .grad is a view into (`flat_layout`), allocated on first use and kept while the parameters
        stay where they are"""
        params = list(self.named_parameters())
        key = (str(dev),) + tuple(p.data_ptr() for _, p in params)
        if self._grad_key != key or any(p.grad is None for _, p in params):
            table, total = flat_layout(self)
            self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
            for (_, p), (o, n) in zip(params, table):
                p.grad = self.flat_grad[o:o + n].view(p.shape)
            self._grad_key = key
        return self.flat_grad

    # ---- sampling: one captured position, replayed ------------------------------------------------------
    @staticmethod
    def _use_graph(graph) -> bool:
        """sample(graph=): None reads ENH_GRAPHS == "1" (the stage-1 engine's switch), anything else is the caller's choice.  While per-kernel
        timing is on (_C.TIMER) the answer is False: a replay runs no host code to time (as engine/stage1.py forward_backward_graphed)."""
        from ... import _C
        use = os.environ.get("ENH_GRAPHS", "0") == "1" if graph is None else bool(graph)
        return use and _C.TIMER is None

    def _sample_graphed(self, B: int, dev, make_state, run_chunk) -> None:
        """sample(graph=True): the chunks of <= MAX_BATCH rows, each as position 0 and one captured position.  run_chunk(st, s, e, positions) runs
        rows s .. e - 1 in the buffers st = make_state(e - s) by calling positions(T, first, later, start = 0): first() runs eagerly (it embeds the
        condition, or under prefix_codes prefills `start` positions and runs position `start`, and it warms the launches and their workspaces), the
        cursor (device int32) is set to start + 1, later(cursor), the launches of one position in
        their cursor forms, is captured once with enh_cursor_advance behind it, and the graph is replayed T - start - 1 times.  Everything runs on one
        side stream, so the graph is a chain; the current stream waits for it at the end.  Nothing is kept from call to call but what a replay
        that may still be running points at: the graphs, their cursors, the chunk buffers and the workspaces of the launches (`_sample_keep`),
        until the next call replaces them."""
        from ... import _C
        cur = torch.cuda.current_stream(dev)
        side = self._sample_stream
        if side is None or side.device != dev:
            side = self._sample_stream = torch.cuda.Stream(dev)
        keep, states = [], {}

        def positions(T, first, later, start: int = 0):
            first()
            if T == start + 1:
                return
            cursor = torch.full((1,), start + 1, dtype=torch.int32, device=dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                later(cursor)
                _C.cursor_advance(cursor)
            for _ in range(T - start - 1):
                g.replay()
            keep.append((g, cursor))

        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for s in range(0, B, MAX_BATCH):
                e = min(s + MAX_BATCH, B)
                if e - s not in states:       # chunks of one size share their buffers: the stream orders them
                    states[e - s] = make_state(e - s)
                run_chunk(states[e - s], s, e, positions)
        cur.wait_stream(side)
        self._sample_keep = (keep, states, list(_C._WS.values()), list(_C._GEMM_WS.values()))

    # ---- the teacher-forced driver ------------------------------------------------------------------
    def _teacher_forced(self, who: str, codes, conds, use_fp16: bool, return_loss: bool, why: str):
        """forward() of both priors: logits (f32) and, with return_loss=True, (logits, nll, mean); nll has the shape of the codes with their
        leading axes folded ([B, T], or [B T, D]), logits one more axis of V.  Batches run in chunks of whole batch items sized so that the MLP's
        hidden activation ([rows, 4C], f32 and its operand copy) stays under `forward_hidden_cap` bytes;
        `_forward_rows(st, codes, conds, logits [b, rows per item, V], dt)` runs a chunk in the buffers of `_forward_buffers`."""
        codes, conds = self._check_inputs(codes, conds, who, why)
        from ... import _C
        dev, B, V = codes.device, codes.shape[0], self.vocab_img_size
        dt = self._operand_dtype(use_fp16, who)
        rows = codes[0].numel()       # of the hidden activation, per batch item
        chunk = max(1, min(B, int(self.forward_hidden_cap) // (rows * 4 * self.embed_dim * (4 + (2 if use_fp16 else 0)))))
        shape = codes.view(-1, codes.shape[-1]).shape
        logits = torch.empty(*shape, V, dtype=torch.float32, device=dev)
        nll = torch.empty(*shape, dtype=torch.float32, device=dev) if return_loss else None
        st = self._chunk_state("_fwd_states", self._forward_buffers, chunk, dt, dev)
        for s in range(0, B, chunk):
            e = min(s + chunk, B)
            lg = logits.view(B, rows, V)[s:e]
            self._forward_rows(st, codes[s:e], conds[s:e], lg, dt)
            if return_loss:
                _C.cross_entropy_rows(lg.view(-1, V), codes[s:e].reshape(-1), nll.view(B, rows)[s:e].view(-1))
        if not return_loss:
            return logits
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        _C.mean_f32(nll.view(-1), mean)
        return logits, nll, mean[0]

    def _teacher_forced_backward(self, who: str, codes, conds, use_fp16: bool, loss_scale, accumulate: bool, item_bytes: int) -> torch.Tensor:
        """forward_backward() of both priors: the unscaled mean cross-entropy over every code, with loss_scale x its gradient left in every
        parameter's .grad (views into `flat_grad`).  Batches run in chunks of whole batch items sized so that the activations saved for the
        backward (`item_bytes` per item) stay under `backward_saved_cap` bytes;
        `_backward_rows(st, codes, conds, nll, dt, gscale, accumulate, gscale_dev)` runs a chunk in the buffers of `_backward_buffers`, setting
        the gradients in the first chunk (unless accumulate) and adding to them in the later ones."""
        if not use_fp16:
            raise NotImplementedError(f"{who}(use_fp16=False): the exact-f32 backward is not built; use the 16-bit operand format")
        codes, conds = self._check_inputs(codes, conds, who)
        from ... import _C
        dev, B = codes.device, codes.shape[0]
        dt = self._operand_dtype(True, who)
        rows = codes[0].numel()       # codes per batch item
        chunk = max(1, min(B, int(self.backward_saved_cap) // item_bytes))
        self._flat_grads(dev)
        st = self._chunk_state("_bwd_states", self._backward_buffers, chunk, dt, dev)
        nll = torch.empty(B, rows, dtype=torch.float32, device=dev)
        scale_dev = None
        if torch.is_tensor(loss_scale):
            if not (loss_scale.is_cuda and loss_scale.dtype == torch.float32 and loss_scale.numel() == 1):
                raise ValueError(f"{who}: a tensor loss_scale must be a device f32 tensor of one element")
            scale_dev, loss_scale = loss_scale.view(1), 1.0
        gscale = float(loss_scale) / float(B * rows)
        for s in range(0, B, chunk):
            e = min(s + chunk, B)
            self._backward_rows(st, codes[s:e], conds[s:e], nll[s:e], dt, gscale, accumulate=accumulate or s > 0, gscale_dev=scale_dev)
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        _C.mean_f32(nll.view(-1), mean)
        return mean[0]
