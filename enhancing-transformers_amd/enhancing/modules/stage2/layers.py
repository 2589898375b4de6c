"""Stage-2 GPT prior (reference enhancing/modules/stage2/layers.py:23-303): sampling, the teacher-forced forward, and the loss with its gradients;
the optimizer step over them is engine/optim.py GPTAdam.

The modules below are parameter containers with the reference's names, shapes and init, so its checkpoints and yaml load.  `GPT.sample` is the
reference's cached sampling loop restated per step on the device (csrc/gpt_decode.hip, gpt_rows.hip).  With cond_num_tokens == 1 every step is one token per
batch row; under the cache the block sees T == 1, where `time_shift(x)` is all zeros and the mix `x * time_mix + time_shift(x) * (1 - time_mix)`
is `ln1(x) * time_mix`.  That is what `GPT.sample` computes, and it is NOT what the teacher-forced `GPT.forward` computes (there the shifted
term is the previous token's ln1 row): two contracts, two goldens (tests/golden/gpt_<case>.npz, gpt_fwd_<case>.npz).

Per step and layer: ln1 * time_mix -> fused q|k|v (one [3C, C] weight) -> attention against the cache, appending k / v -> proj + residual ->
ln2 -> p0 with relu^2 -> p1 + residual; then the final LayerNorm, the head and the sampler.  Nothing in the loop reads a device value on
the host: the drawn codes stay in device memory and the next step's embedding kernel reads them there.

`GPT.forward` runs the whole sequence at once (csrc/gpt_rows.hip and gpt_prefill.hip between enh_gemm_h16 products): embedding of [B, S, C] in one launch, per layer
ln1 + time shift -> q|k|v -> causal flash attention -> proj + residual -> ln2 -> p0 -> relu^2 -> p1 + residual, the final LayerNorm and the head;
optionally the per-position cross-entropy and its mean on the device.  Inference only: no autograd graph.

`GPT.forward_backward` is that forward with its activations kept per layer, followed by a hand-written backward on the device: the
loss gradient fused with the cross-entropy, every product an enh_gemm_h16 call (weight gradients accumulated in f32 into one flat gradient buffer
that every `p.grad` is a view into), the f32 gradient of the residual stream carried through the LayerNorm / time-shift, relu^2 and embedding
backward kernels of csrc/gpt_rows.hip and the causal flash-attention backward of csrc/gpt_attn_bwd.hip.  16-bit operand formats only.

`GPTAdam` (engine/optim.py) re-homes the parameters into one flat f32 buffer with `flat_grad`'s layout and owns a 16-bit operand arena that its step
kernel (csrc/gpt_adam.hip) rewrites together with the masters; `_operand_copies` then returns views into that arena (`_arena`), so forward, sample and
forward_backward see stepped weights without a rebuild.

`RQTransformer` (reference layers.py:306-547) is the prior over a residual quantizer's [B, T, D] codes: `RQTransformer.forward` is the teacher-forced
forward and the validation loss.  Its spatial transformer is `GPT.forward`'s per-layer launch sequence (`_block_rows`, shared); the
embedding stage, ln_spatial written into slot 0 of the depth sequences and the depth transformer's attention over B T sequences of D <= 8 slots are
csrc/rq_prefill.hip.  The reference's forward sums the code embeddings along the CHANNELS (`codes.cumsum(-1)`) where its sampler sums along DEPTH:
keyword `code_sum` chooses, "depth" by default (see the class docstring).

Left out: RQTransformer's sampling, backward and optimizer step, an exact-f32 backward, more than one condition token, HIP-graph capture, relu^2 /
LayerNorm fused into GEMM epilogues."""
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn

MAX_BATCH = 64          # rows of one decode step (enh_skinny_gemm_h16); larger batches run in chunks
MAX_EMBED = 8192        # enh_row_ln_scale
MAX_VOCAB = 16384       # enh_sample_logits
MAX_HEAD = 384          # enh_decode_attention
MAX_TOKENS = 8192       # enh_decode_attention: slots of the k / v cache
FORWARD_HIDDEN_CAP = 2 << 30   # bytes of forward()'s [chunk T, 4C] hidden activation (f32 + operand copy): shipped size, 6 sequences per chunk
BACKWARD_SAVED_CAP = 16 << 30  # bytes of forward_backward()'s saved activations: shipped size 24 x 172,096 B per token, 4 sequences of 1024 per chunk
OPERAND_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}


class MultiHeadSelfAttention(nn.Module):
    def __init__(self, ctx_len: int, cond_len: int, embed_dim: int, n_heads: int, attn_bias: bool, use_mask: bool = True):
        super().__init__()
        assert embed_dim % n_heads == 0
        self.key = nn.Linear(embed_dim, embed_dim, bias=attn_bias)
        self.query = nn.Linear(embed_dim, embed_dim, bias=attn_bias)
        self.value = nn.Linear(embed_dim, embed_dim, bias=attn_bias)
        self.proj = nn.Linear(embed_dim, embed_dim, attn_bias)
        self.n_heads = n_heads
        self.ctx_len = ctx_len
        # (the reference's `mask` buffer is non-persistent: no state-dict entry; sampling one token per step needs no mask)
        self.time_mix = nn.Parameter((torch.arange(embed_dim, dtype=torch.float32) / (embed_dim - 1)).view(1, 1, embed_dim))


class FFN(nn.Module):
    def __init__(self, embed_dim: int, mlp_bias: bool):
        super().__init__()
        self.p0 = nn.Linear(embed_dim, 4 * embed_dim, bias=mlp_bias)
        self.p1 = nn.Linear(4 * embed_dim, embed_dim, bias=mlp_bias)


class Block(nn.Module):
    def __init__(self, ctx_len: int, cond_len: int, embed_dim: int, n_heads: int, mlp_bias: bool, attn_bias: bool):
        super().__init__()
        self.ln1 = nn.LayerNorm(embed_dim)
        self.ln2 = nn.LayerNorm(embed_dim)
        self.attn = MultiHeadSelfAttention(ctx_len=ctx_len, cond_len=cond_len, embed_dim=embed_dim, n_heads=n_heads, attn_bias=attn_bias)
        self.mlp = FFN(embed_dim=embed_dim, mlp_bias=mlp_bias)


# ---- what the teacher-forced forwards of GPT and RQTransformer share: the products, one block's launches, the operand copies ----------------
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


def _layer_operands(blocks, cast) -> list:
    """per Block: the fused q|k|v weight and bias, proj, p0 and p1 through `cast`, and time_mix as a flat f32 vector"""
    layers = []
    for blk in blocks:
        a, m = blk.attn, blk.mlp
        bias = None
        if a.query.bias is not None:
            bias = torch.cat([a.query.bias, a.key.bias, a.value.bias]).detach().float().contiguous()
        layers.append(dict(wqkv=cast(torch.cat([a.query.weight, a.key.weight, a.value.weight], 0)), bqkv=bias, wproj=cast(a.proj.weight),
                           w0=cast(m.p0.weight), w1=cast(m.p1.weight), time_mix=a.time_mix.detach().reshape(-1).contiguous()))
    return layers


class GPT(nn.Module):
    def __init__(self, vocab_cond_size: int, vocab_img_size: int, embed_dim: int, cond_num_tokens: int, img_num_tokens: int, n_heads: int,
                 n_layers: int, mlp_bias: bool = True, attn_bias: bool = True) -> None:
        super().__init__()
        if cond_num_tokens != 1:
            raise ValueError(f"GPT: cond_num_tokens must be 1 (class conditioning: every sampling step is one token), got {cond_num_tokens}")
        if embed_dim % n_heads:
            raise ValueError(f"GPT: embed_dim {embed_dim} is not a multiple of n_heads {n_heads}")
        hs = embed_dim // n_heads
        if hs % 64 or hs > MAX_HEAD:
            raise ValueError(f"GPT: the head size embed_dim / n_heads must be a multiple of 64 up to {MAX_HEAD}, got {hs}")
        if vocab_img_size > MAX_VOCAB:
            raise ValueError(f"GPT: vocab_img_size must be at most {MAX_VOCAB}, got {vocab_img_size}")
        if embed_dim > MAX_EMBED:
            raise ValueError(f"GPT: embed_dim must be at most {MAX_EMBED}, got {embed_dim}")
        if vocab_img_size % 8:
            raise ValueError(f"GPT: vocab_img_size must be a multiple of 8 (the head's GEMM), got {vocab_img_size}")
        if img_num_tokens > MAX_TOKENS:
            raise ValueError(f"GPT: img_num_tokens must be at most {MAX_TOKENS} (the cache of the decode attention), got {img_num_tokens}")
        self.img_num_tokens = img_num_tokens
        self.vocab_cond_size = vocab_cond_size
        self.vocab_img_size = vocab_img_size
        self.embed_dim = embed_dim
        self.n_heads = n_heads
        self.tok_emb_cond = nn.Embedding(vocab_cond_size, embed_dim)
        self.pos_emb_cond = nn.Parameter(torch.zeros(1, cond_num_tokens, embed_dim))
        self.tok_emb_code = nn.Embedding(vocab_img_size, embed_dim)
        self.pos_emb_code = nn.Parameter(torch.zeros(1, img_num_tokens, embed_dim))
        self.blocks = nn.Sequential(*[Block(ctx_len=cond_num_tokens + img_num_tokens, cond_len=cond_num_tokens, embed_dim=embed_dim,
                                            n_heads=n_heads, mlp_bias=mlp_bias, attn_bias=attn_bias) for _ in range(n_layers)])
        self.layer_norm = nn.LayerNorm(embed_dim)
        self.head = nn.Linear(embed_dim, vocab_img_size, bias=False)
        self.apply(self._init_weights)
        self._operands = {}       # operand format -> (versions of the masters, per-layer operand copies)
        self._fwd_states = {}     # (chunk, dtype, device) -> the buffers of forward()
        self.forward_hidden_cap = FORWARD_HIDDEN_CAP
        self.backward_saved_cap = BACKWARD_SAVED_CAP      # bytes of forward_backward()'s saved activations of all layers in one chunk
        self._bwd_states = {}     # (chunk, dtype, device) -> the buffers of forward_backward()
        self._grad_key = None     # the parameters whose .grad are views into flat_grad
        self.flat_grad = None
        self._arena = None        # set by engine/optim.py GPTAdam: dict(dt, ptrs, ops, versions, refresh) — the operand arena its step kernel keeps current

    def _init_weights(self, module: nn.Module) -> None:
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if isinstance(module, nn.Linear) and module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    # ---- what forward() and sample() both begin with ----------------------------------------------
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

    # ---- teacher-forced forward -------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, codes: torch.Tensor, conds: torch.Tensor, *, use_fp16: bool = True, return_loss: bool = False):
        """reference layers.py:193-211: logits [B, T, V] (f32) of every code given the condition and the codes before it; with return_loss=True
        (logits, nll [B, T], mean): the per-position cross-entropy against `codes` and its mean (the reference's val/total_loss), both on the device.

        Inference only: the call runs under torch.no_grad and the result carries no autograd graph (stage-2 training is not built).
        S = T rows are built, the condition and the first T - 1 codes: the causal mask keeps the last code's row from every logit that is kept.
        use_fp16=True runs the 16-bit operand format of ENH_PRECISION (default fp16) through enh_gemm_h16 and the MFMA causal attention; biases,
        residuals and LayerNorms stay on the f32 residual stream.  False is the exact mode: f32 operands, tree-ordered sums (enh_skinny_gemm_f32
        in 64-row pieces), the f32 attention instrument.  Device tensors only.  Batches run in chunks of whole sequences sized so that the hidden
        activation of the MLP ([chunk T, 4C], f32 and its operand copy) stays under `forward_hidden_cap` bytes.
        Side effect, as in sample(): a module whose parameters are not on the device of `codes` is moved there."""
        if not (torch.is_tensor(codes) and torch.is_tensor(conds) and codes.is_cuda and conds.is_cuda):
            raise NotImplementedError("GPT.forward runs on a ROCm device only: codes and conds must be device tensors (there is no CPU path for the "
                                      "teacher-forced forward; note that the cached sample() does not compute the same logits: time_shift)")
        from ... import _C
        dev = codes.device
        B, T, V = codes.shape[0], self.img_num_tokens, self.vocab_img_size
        codes, conds = self._check_inputs(codes, conds, "GPT.forward")
        dt = self._operand_dtype(use_fp16, "GPT.forward")
        chunk = max(1, min(B, int(self.forward_hidden_cap) // (T * 4 * self.embed_dim * (4 + (2 if use_fp16 else 0)))))
        logits = torch.empty(B, T, V, dtype=torch.float32, device=dev)
        nll = torch.empty(B, T, dtype=torch.float32, device=dev) if return_loss else None
        st = self._forward_state(chunk, dt, dev)
        for s in range(0, B, chunk):
            e = min(s + chunk, B)
            self._forward_rows(st, codes[s:e], conds[s:e], logits[s:e], dt)
            if return_loss:
                _C.cross_entropy_rows(logits[s:e].view(-1, V), codes[s:e].reshape(-1), nll[s:e].view(-1))
        if not return_loss:
            return logits
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        _C.mean_f32(nll.view(-1), mean)
        return logits, nll, mean[0]

    # ---- teacher-forced loss and its gradients -----------------------------------------------------
    def _check_inputs(self, codes, conds, who: str):
        """what forward() and forward_backward() accept: (codes [B, T] int64, conds [B] int64) on the device, ranges checked"""
        B, T, V = codes.shape[0], self.img_num_tokens, self.vocab_img_size
        codes = codes.reshape(B, -1).to(torch.int64).contiguous()
        if codes.shape[1] != T:
            raise ValueError(f"{who}: codes must hold img_num_tokens = {T} codes per row, got {codes.shape[1]}")
        conds = self._on_device_conds(conds, B, who)
        if int(codes.min()) < 0 or int(codes.max()) >= V:
            raise ValueError(f"{who}: codes outside [0, {V})")
        if int(conds.min()) < 0 or int(conds.max()) >= self.vocab_cond_size:
            raise ValueError(f"{who}: conds outside [0, {self.vocab_cond_size})")
        return codes, conds

    def saved_bytes_per_token(self) -> int:
        """bytes forward_backward keeps per token row for ALL layers: per layer the f32 inputs of ln1 and ln2 (4C + 4C), the
        16-bit operands a, qkv, att, a2 and hid (2C + 6C + 2C + 2C + 8C) and the attention's lse (4 H)"""
        return len(self.blocks) * (28 * self.embed_dim + 4 * self.n_heads)

    def _flat_grads(self, dev) -> torch.Tensor:
        """one flat f32 buffer that every parameter's .grad is a view into (engine/stage1.py ParamStore's layout: registration order, every
        parameter padded to 64 elements), allocated on first use and kept while the parameters stay where they are"""
        params = list(self.named_parameters())
        key = (str(dev),) + tuple(p.data_ptr() for _, p in params)
        if self._grad_key != key or any(p.grad is None for _, p in params):
            total, offs = 0, []
            for _, p in params:
                offs.append(total)
                total += (p.numel() + 63) // 64 * 64
            self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
            for (_, p), o in zip(params, offs):
                p.grad = self.flat_grad[o:o + p.numel()].view(p.shape)
            self._grad_key = key
        return self.flat_grad

    def _backward_state(self, b: int, dt: torch.dtype, dev) -> dict:
        """the buffers of a chunk of b sequences: row counts rounded up to 8 (the contraction length of a weight-gradient product), everything
        zero at first so that the tail rows of an operand are finite; the tail rows of the gradient operands are zeroed again for a shorter chunk"""
        key = (b, dt, str(dev))
        st = self._bwd_states.get(key)
        if st is None:
            f32, C, H, V, T = torch.float32, self.embed_dim, self.n_heads, self.vocab_img_size, self.img_num_tokens
            Mp = (b * T + 7) // 8 * 8
            z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype, device=dev)
            saved = [dict(x=z(Mp, C, dtype=f32), a=z(Mp, C), qkv=z(Mp, 3 * C), att=z(Mp, C), lse=z(b * H * T, dtype=f32), x2=z(Mp, C, dtype=f32),
                          a2=z(Mp, C), hid=z(Mp, 4 * C)) for _ in self.blocks]
            st = dict(saved=saved, x=z(Mp, C, dtype=f32), a=z(Mp, C), hid32=z(Mp, 4 * C, dtype=f32), logits=z(Mp, V, dtype=f32), dlogits=z(Mp, V),
                      g=z(Mp, C, dtype=f32), g2=z(Mp, C, dtype=f32), d32=z(Mp, C, dtype=f32), g16=z(Mp, C), dh16=z(Mp, 4 * C), dqkv=z(Mp, 3 * C),
                      datt=z(Mp, C), dbqkv=z(3 * C, dtype=f32))
            self._bwd_states = {key: st}      # one chunk size at a time, as _forward_state
        return st

    @torch.no_grad()
    def forward_backward(self, codes: torch.Tensor, conds: torch.Tensor, *, use_fp16: bool = True, loss_scale=1.0, accumulate: bool = False) -> torch.Tensor:
        """the teacher-forced loss and its gradients in one call: returns the unscaled mean cross-entropy over all B T positions (0-dim f32 on the
        device: what forward(..., return_loss=True)[2] returns, and with the same chunking the same bits) and leaves in `p.grad` of EVERY
        parameter loss_scale x the gradient of that mean (f32, views into the flat buffer `flat_grad`: what GradScaler.scale(loss).backward()
        leaves).  loss_scale is a float or a device f32 [1] tensor (a loss scale that lives on the device: engine/optim.py GPTAdam; the cross-entropy
        backward reads it there, no host round trip).  The call SETS the gradients, or with accumulate=True ADDS to them (accumulate_grad_batches);
        rows of the token tables whose id does not occur are exactly zero when set.

        use_fp16=True runs the 16-bit operand format of ENH_PRECISION: every product is an enh_gemm_h16 call (weight gradients accumulate in f32),
        the residual stream's gradient stays f32, the kernels between the products are csrc/gpt_rows.hip's and csrc/gpt_attn_bwd.hip's.  The
        exact-f32 backward is not built: use_fp16=False raises.  Device tensors only.  Batches run in chunks of whole sequences sized so that the
        activations saved for the backward stay under `backward_saved_cap` bytes (saved_bytes_per_token() per token row); weight gradients
        accumulate across the chunks in a fixed order, so two runs give the same bits.  Any B T works: a chunk's row buffers are rounded up to 8 rows
        and the tail rows of every gradient operand are zero.  The optimizer step and the overflow check are GPTAdam.step()."""
        if not use_fp16:
            raise NotImplementedError("GPT.forward_backward(use_fp16=False): the exact-f32 backward is not built; use the 16-bit operand format")
        if not (torch.is_tensor(codes) and torch.is_tensor(conds) and codes.is_cuda and conds.is_cuda):
            raise NotImplementedError("GPT.forward_backward runs on a ROCm device only: codes and conds must be device tensors (there is no CPU path)")
        from ... import _C
        dev = codes.device
        B, T, V = codes.shape[0], self.img_num_tokens, self.vocab_img_size
        codes, conds = self._check_inputs(codes, conds, "GPT.forward_backward")
        dt = self._operand_dtype(True, "GPT.forward_backward")
        chunk = max(1, min(B, int(self.backward_saved_cap) // (T * self.saved_bytes_per_token())))
        self._flat_grads(dev)
        st = self._backward_state(chunk, dt, dev)
        nll = torch.empty(B, T, dtype=torch.float32, device=dev)
        scale_dev = None
        if torch.is_tensor(loss_scale):
            if not (loss_scale.is_cuda and loss_scale.dtype == torch.float32 and loss_scale.numel() == 1):
                raise ValueError("GPT.forward_backward: a tensor loss_scale must be a device f32 tensor of one element")
            scale_dev, loss_scale = loss_scale.view(1), 1.0
        gscale = float(loss_scale) / float(B * T)
        for s in range(0, B, chunk):
            e = min(s + chunk, B)
            self._backward_rows(st, codes[s:e], conds[s:e], nll[s:e], dt, gscale, accumulate=accumulate or s > 0, gscale_dev=scale_dev)
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        _C.mean_f32(nll.view(-1), mean)
        return mean[0]

    def _backward_rows(self, st, codes, conds, nll, dt, gscale: float, accumulate: bool, gscale_dev=None) -> None:
        """one chunk: the saving forward, then the backward of DESIGN.md §3.7, setting (accumulate=False) or adding to every parameter's gradient"""
        from ... import _C
        b, T, C, H, V = codes.shape[0], self.img_num_tokens, self.embed_dim, self.n_heads, self.vocab_img_size
        M, hs = b * T, C // H
        Mp = (M + 7) // 8 * 8
        ops = self._operand_copies(dt)
        saved = st["saved"]
        logits, dlogits, g, g2, d32, g16, dh16, dqkv, datt, hid32 = (st[k][:M] for k in ("logits", "dlogits", "g", "g2", "d32", "g16", "dh16", "dqkv",
                                                                                         "datt", "hid32"))
        if Mp > M:      # rows M .. Mp - 1 of the gradient operands may hold a longer chunk's rows
            for k in ("dlogits", "g16", "dh16", "dqkv"):
                st[k][M:Mp].zero_()
        self._forward_rows(st, codes, conds, logits.view(b, T, V), dt, saved=saved)

        def wgrad(dy, inp, grad, n_out: int, k_in: int, lda=None):      # grad [n_out, k_in] (+)= dy^T inp over the chunk's Mp rows
            _C.gemm(dy, inp, n_out, k_in, Mp, trans_a=True, trans_b=True, accumulate=accumulate, out_f32=grad, lda=lda, ldb=k_in)

        def dgrad(dy, w, out):      # out [M, K] = dy [M, N] w [N, K]
            N, K = w.shape
            if out.dtype == torch.float32:
                _C.gemm(dy, w, M, K, N, trans_b=True, out_f32=out)
            else:
                _C.gemm(dy, w, M, K, N, trans_b=True, out_bf16=out)

        if gscale_dev is None:
            _C.cross_entropy_backward(logits, codes.reshape(-1), nll.view(-1), dlogits, gscale)
        else:
            _C.cross_entropy_backward(logits, codes.reshape(-1), nll.view(-1), dlogits, gscale, gscale_dev=gscale_dev)
        wgrad(st["dlogits"], st["a"], self.head.weight.grad, V, C)
        dgrad(dlogits, ops["head"], d32)
        ln = self.layer_norm
        _C.ln_timeshift_backward(d32, st["x"][:M], ln.weight, T, g, ln.weight.grad, ln.bias.grad, dx16=g16, eps=ln.eps, accumulate=accumulate)
        for i in range(len(self.blocks) - 1, -1, -1):
            blk, W, sv = self.blocks[i], ops["layers"][i], saved[i]
            at, ml = blk.attn, blk.mlp
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
            _C.ln_timeshift_backward(d32, sv["x2"][:M], blk.ln2.weight, T, g2, blk.ln2.weight.grad, blk.ln2.bias.grad, dres=g, dx16=g16, eps=blk.ln2.eps,
                                     accumulate=accumulate)
            # proj, attention, q | k | v
            wgrad(st["g16"], sv["att"], at.proj.weight.grad, C, C)
            if at.proj.bias is not None:
                _C.colsum(g16, M, C, at.proj.bias.grad, accumulate)
            dgrad(g16, W["wproj"], datt)
            _C.causal_attention_backward(sv["qkv"][:M], sv["att"][:M], datt, sv["lse"][:b * H * T], b, T, H, hs, dqkv)
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
            _C.ln_timeshift_backward(d32, sv["x"][:M], blk.ln1.weight, T, g, blk.ln1.weight.grad, blk.ln1.bias.grad, b=blk.ln1.bias, colscale=W["time_mix"],
                                     dcolscale=at.time_mix.grad.view(-1), dres=g2, dx16=g16, eps=blk.ln1.eps, accumulate=accumulate)
        _C.gpt_embed_seq_backward(g.view(b, T, C), conds, codes, self.tok_emb_cond.weight.grad, self.pos_emb_cond.grad.view(-1), self.tok_emb_code.weight.grad,
                                  self.pos_emb_code.grad.view(-1, C), accumulate)

    def _forward_state(self, b: int, dt: torch.dtype, dev) -> dict:
        """the buffers of a chunk of b sequences, kept per (b, dtype) from call to call; a shorter last chunk uses their leading rows"""
        key = (b, dt, str(dev))
        st = self._fwd_states.get(key)
        if st is None:
            f32, C, M = torch.float32, self.embed_dim, b * self.img_num_tokens
            e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
            st = dict(x=e(M, C, dtype=f32), x2=e(M, C, dtype=f32), a=e(M, C), qkv=e(M, 3 * C), att=e(M, C), hid32=e(M, 4 * C, dtype=f32),
                      hid=e(M, 4 * C) if dt != f32 else None)
            self._fwd_states = {key: st}      # one chunk size at a time: the buffers of a shipped-size chunk are gigabytes
        return st

    def _forward_rows(self, st, codes, conds, logits, dt, saved=None) -> None:
        """one chunk of b whole sequences in the leading b T rows of the buffers `st`: logits [b, T, V] f32.  saved (forward_backward): one dict of
        buffers per layer; the layer's input x, a (ln1), qkv, att, lse, x2, a2 (ln2) and hid then stay there instead of in the shared buffers of
        `st`, and the last layer's output goes to st["x"].  The launches and their arguments are the same: so are the bits."""
        from ... import _C
        b, T, C, H, V = codes.shape[0], self.img_num_tokens, self.embed_dim, self.n_heads, self.vocab_img_size
        M, hs = b * T, C // H
        ops = self._operand_copies(dt)
        x, x2, a, qkv, att, hid32, hid = (None if st.get(k) is None else st[k][:M] for k in ("x", "x2", "a", "qkv", "att", "hid32", "hid"))
        linear = _row_linear(M, dt)
        x_out, a2, lse = x, a, None
        if saved is not None:
            x = saved[0]["x"][:M]
        _C.gpt_embed_seq(conds, codes, self.tok_emb_cond.weight.detach(), self.pos_emb_cond.detach()[0, 0], self.tok_emb_code.weight.detach(),
                         self.pos_emb_code.detach()[0], x.view(b, T, C))
        for i, (blk, W) in enumerate(zip(self.blocks, ops["layers"])):
            if saved is not None:
                a, qkv, att, x2, a2, hid = (saved[i][k][:M] for k in ("a", "qkv", "att", "x2", "a2", "hid"))
                lse = saved[i]["lse"][:b * H * T]
                x_out = saved[i + 1]["x"][:M] if i + 1 < len(saved) else st["x"][:M]
            _block_rows(blk, W, linear, dt, T, lambda qkv_, att_, lse_=lse: _C.causal_attention(qkv_, b, T, H, hs, att_, lse=lse_),
                        x, x_out, a, a2, qkv, att, x2, hid32, hid)
            x = x_out
        a = st["a"][:M]
        _C.ln_timeshift(x, self.layer_norm.weight, self.layer_norm.bias, a, T, eps=self.layer_norm.eps)
        linear(a, ops["head"], logits.view(M, V))

    # ---- operand copies -------------------------------------------------------------------------
    def _operand_copies(self, dt: torch.dtype):
        """the GEMM weights in the operand format `dt` (torch.float32: the exact mode's packed f32 q|k|v), built once from the fp32 masters and
        rebuilt when a master was replaced or written in place (load_state_dict): the masters' version counters are the key.  Under a GPTAdam
        (`_arena`) the 16-bit operands are views into the optimizer's arena, which its step kernel rewrites with the masters: nothing is rebuilt, and
        a module whose parameters were moved or replaced since, or whose operand format changed, is refused."""
        ar = getattr(self, "_arena", None)
        if ar is not None and dt != torch.float32:
            if dt != ar["dt"]:
                raise RuntimeError(f"GPT: the optimizer's operand arena holds {ar['dt']} but the engine's operand format (ENH_PRECISION) is now {dt}: "
                                   "build a new GPTAdam (configure_optimizers) under the format you train in")
            if tuple(p.data_ptr() for p in self.parameters()) != ar["ptrs"]:
                raise RuntimeError("GPT: the parameters were moved or replaced after GPTAdam was built (.to(), .half(), assigning .data): the optimizer's "
                                   "flat buffers and operand arena no longer belong to them; build a new GPTAdam (configure_optimizers)")
            if tuple(p._version for p in self.parameters()) != ar["versions"]:      # torch wrote a master in place (load_state_dict): recast the arena
                ar["refresh"]()
            return ar["ops"]
        masters = [p for _, p in sorted(self.named_parameters())]
        key = tuple((p.data_ptr(), p._version) for p in masters)
        hit = self._operands.get(dt)
        if hit is not None and hit[0] == key:
            return hit[1]
        cast = (lambda w: w.detach().to(dt).contiguous())
        ops = dict(layers=_layer_operands(self.blocks, cast), head=cast(self.head.weight))
        self._operands[dt] = (key, ops)
        return ops

    # ---- sampling -------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, conds: torch.Tensor, top_k: Optional[float] = None, top_p: Optional[float] = None, softmax_temperature: float = 1.0,
               use_fp16: bool = True, *, seed: Optional[int] = None, forced_codes: Optional[torch.Tensor] = None, return_logits: bool = True,
               call: int = 0, row_offset: int = 0) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """reference layers.py:213-266: returns (logits [B, T*V] after the temperature and the top-k mask, codes [B, T]).

        use_fp16=True runs the 16-bit operand format of ENH_PRECISION (default fp16) with f32 accumulation; False the exact mode (f32 operands on the vector ALU, f32 cache and
        row kernels).  The draw is an inverse-CDF walk in index order with one uniform per (seed, call, step, row_offset + row): the distribution of
        the reference's torch.multinomial, not its bits; a seed gives the same codes on every run (seed=None draws one from torch's generator).
        forced_codes [B, T] feeds the given codes to the next step instead of the drawn ones (codes are still drawn and returned).
        Batches above 64 rows run in chunks of 64 rows.
        Side effect: a module whose parameters are not on the device of `conds` is MOVED there (`self.to(conds.device)`) on the first call, as the
        stage-1 engine moves its model; the reference leaves that to the caller."""
        if not conds.is_cuda:
            raise RuntimeError("GPT.sample runs on a ROCm device only: conds must be a device tensor (there is no CPU path)")
        dev = conds.device
        conds = self._on_device_conds(conds, conds.shape[0], "GPT.sample")
        B, T, V = conds.shape[0], self.img_num_tokens, self.vocab_img_size
        if top_k is not None and not 1 <= int(top_k) <= V:
            raise ValueError(f"GPT.sample: top_k must be in [1, {V}], got {top_k}")
        if forced_codes is not None:
            forced_codes = forced_codes.to(device=dev, dtype=torch.int64).reshape(B, T).contiguous()
            if int(forced_codes.min()) < 0 or int(forced_codes.max()) >= V:
                raise ValueError(f"GPT.sample: forced_codes outside [0, {V})")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        dt = self._operand_dtype(use_fp16, "GPT.sample")
        codes = torch.empty(B, T, dtype=torch.int64, device=dev)
        logits = torch.empty(B, T * V, dtype=torch.float32, device=dev) if return_logits else None
        for s in range(0, B, MAX_BATCH):
            e = min(s + MAX_BATCH, B)
            self._sample_rows(conds[s:e], codes[s:e], None if logits is None else logits[s:e], None if forced_codes is None else forced_codes[s:e],
                              dt, top_k, top_p, float(softmax_temperature), seed, call, row_offset + s)
        return logits, codes

    def _sample_rows(self, conds, codes, logits, forced, dt, top_k, top_p, temperature, seed, call, row0):
        from ... import _C
        T, V = self.img_num_tokens, self.vocab_img_size
        st = self._decode_state(conds.shape[0], dt, conds.device)
        feed = codes if forced is None else forced
        for t in range(T):
            self._decode_step(st, t, conds if t == 0 else feed[:, t - 1])
            _C.sample_logits(st["logits"], codes[:, t], temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, call=call, step=t, row0=row0,
                             logits_out=None if logits is None else logits[:, t * V:(t + 1) * V])

    def _decode_state(self, b: int, dt: torch.dtype, dev, cache_len: Optional[int] = None) -> dict:
        """the buffers of one chunk of b <= 64 rows: residual stream, activations, the step's logits and every layer's k / v cache [b, H, T, hs]"""
        f32, C, H = torch.float32, self.embed_dim, self.n_heads
        T = cache_len or self.img_num_tokens
        e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
        return dict(dt=dt, b=b, x=e(b, C, dtype=f32), x2=e(b, C, dtype=f32), a=e(b, C), qkv=e(b, 3 * C), att=e(b, C), hid=e(b, 4 * C),
                    logits=e(b, self.vocab_img_size, dtype=f32), caches=[(e(b, H, T, C // H), e(b, H, T, C // H)) for _ in self.blocks],
                    ops=self._operand_copies(dt))

    def _decode_step(self, st: dict, t: int, ids: torch.Tensor) -> None:
        """one token per row: ids (int64, on the device: the condition at t == 0, else the previous step's codes) -> st["logits"] [b, V] f32"""
        from ... import _C
        x, x2, a, qkv, att, hid = st["x"], st["x2"], st["a"], st["qkv"], st["att"], st["hid"]
        linear = _C.skinny_gemm_f32 if st["dt"] == torch.float32 else _C.skinny_gemm
        if t == 0:
            _C.gpt_embed(self.tok_emb_cond.weight.detach(), ids, self.pos_emb_cond.detach()[0, 0], x)
        else:
            _C.gpt_embed(self.tok_emb_code.weight.detach(), ids, self.pos_emb_code.detach()[0, t - 1], x)
        for blk, W, (kc, vc) in zip(self.blocks, st["ops"]["layers"], st["caches"]):
            _C.row_ln_scale(x, blk.ln1.weight, blk.ln1.bias, a, colscale=W["time_mix"], eps=blk.ln1.eps)
            linear(a, W["wqkv"], qkv, bias=W["bqkv"])
            _C.decode_attention(qkv, kc, vc, t, att)
            linear(att, W["wproj"], x2, bias=blk.attn.proj.bias, res=x)
            _C.row_ln_scale(x2, blk.ln2.weight, blk.ln2.bias, a, eps=blk.ln2.eps)
            linear(a, W["w0"], hid, bias=blk.mlp.p0.bias, relu_sq=True)
            linear(hid, W["w1"], x, bias=blk.mlp.p1.bias, res=x2)
        _C.row_ln_scale(x, self.layer_norm.weight, self.layer_norm.bias, a, eps=self.layer_norm.eps)
        linear(a, st["ops"]["head"], st["logits"])


MAX_DEPTH = 8           # enh_rq_embed_seq, enh_short_causal_attention_forward: the stage-1 residual quantizer's cap on num_quantizers
CODE_SUMS = ("depth", "channels")


class RQTransformer(nn.Module):
    """reference layers.py:306-395: a spatial transformer over the T positions of an image, whose input at a position is built from the D residual
    codes of the position before it, and a depth transformer over the D slots of every position: slot 0 is ln_spatial of the spatial output, slot
    d >= 1 is built from codes 0 .. d - 1 of the position; logits [B T, D, V].  The reference's constructor arguments, parameter names, shapes and
    init.  Built here: the teacher-forced forward and the validation loss.  Not built: sampling, the backward, the optimizer step.

    The code-sum quirk.  The reference's forward computes `codes.cumsum(-1)` on the [B, T, D, C] embeddings: a running sum along the embedding
    CHANNELS, not along depth.  Its own sampler (sample_spatial_step / sample_depth_step: `codes.sum(1)`) and the RQ-VAE formulation sum over
    DEPTH, so a model trained through the reference's forward is not the model its sampler draws from.  Keyword `code_sum` selects:
      "depth" (default)   spatial row t + 1 = sum_j emb(code[b, t, j]) + pos_emb_code[t]; slot d >= 1 = sum_{j < d} emb(code[b, t, j]) +
                          pos_emb_depth[d - 1]: what the sampler assumes; one launch (enh_rq_embed_seq)
      "channels"          the reference's line in meaning: spatial row t + 1 = cumsum_C(emb(code[b, t, D - 1])) + pos_emb_code[t]; slot d =
                          cumsum_C(emb(code[b, t, d - 1])) + pos_emb_depth[d - 1].  A parity instrument (the reference's own forward is then the
                          golden of everything behind the embedding): the two input tensors are built with torch ops on the device, every launch
                          after them is the default mode's."""

    def __init__(self, vocab_cond_size: int, vocab_img_size: int, embed_dim: int, cond_num_tokens: int, img_num_tokens: int, depth_num_tokens: int,
                 spatial_n_heads: int, depth_n_heads: int, spatial_n_layers: int, depth_n_layers: int, mlp_bias: bool = True, attn_bias: bool = True,
                 *, code_sum: str = "depth") -> None:
        super().__init__()
        if cond_num_tokens != 1:
            raise ValueError(f"RQTransformer: cond_num_tokens must be 1 (class conditioning), got {cond_num_tokens}")
        if depth_num_tokens == 1:
            raise ValueError("RQTransformer: depth_num_tokens == 1 is one code per position: use GPT")
        if not 2 <= depth_num_tokens <= MAX_DEPTH:
            raise ValueError(f"RQTransformer: depth_num_tokens must be in [2, {MAX_DEPTH}] (the residual quantizer's num_quantizers), got {depth_num_tokens}")
        for who, n in (("spatial_n_heads", spatial_n_heads), ("depth_n_heads", depth_n_heads)):
            if embed_dim % n:
                raise ValueError(f"RQTransformer: embed_dim {embed_dim} is not a multiple of {who} {n}")
            if (embed_dim // n) % 64 or embed_dim // n > MAX_HEAD:
                raise ValueError(f"RQTransformer: the head size embed_dim / {who} must be a multiple of 64 up to {MAX_HEAD}, got {embed_dim // n}")
        if vocab_img_size > MAX_VOCAB:
            raise ValueError(f"RQTransformer: vocab_img_size must be at most {MAX_VOCAB}, got {vocab_img_size}")
        if embed_dim > MAX_EMBED:
            raise ValueError(f"RQTransformer: embed_dim must be at most {MAX_EMBED}, got {embed_dim}")
        if vocab_img_size % 8:
            raise ValueError(f"RQTransformer: vocab_img_size must be a multiple of 8 (the head's GEMM), got {vocab_img_size}")
        if img_num_tokens > MAX_TOKENS:
            raise ValueError(f"RQTransformer: img_num_tokens must be at most {MAX_TOKENS}, got {img_num_tokens}")
        if code_sum not in CODE_SUMS:
            raise ValueError(f"RQTransformer: code_sum must be one of {CODE_SUMS}, got {code_sum!r}")
        self.img_num_tokens = img_num_tokens
        self.depth_num_tokens = depth_num_tokens
        self.vocab_cond_size = vocab_cond_size
        self.vocab_img_size = vocab_img_size
        self.embed_dim = embed_dim
        self.spatial_n_heads = spatial_n_heads
        self.depth_n_heads = depth_n_heads
        self.code_sum = code_sum
        self.tok_emb_cond = nn.Embedding(vocab_cond_size, embed_dim)
        self.pos_emb_cond = nn.Parameter(torch.rand(1, cond_num_tokens, embed_dim))
        self.tok_emb_code = nn.Embedding(vocab_img_size, embed_dim)
        self.pos_emb_code = nn.Parameter(torch.rand(1, img_num_tokens, embed_dim))
        self.pos_emb_depth = nn.Parameter(torch.rand(1, depth_num_tokens - 1, embed_dim))
        self.spatial_transformer = nn.Sequential(*[Block(ctx_len=cond_num_tokens + img_num_tokens, cond_len=cond_num_tokens, embed_dim=embed_dim,
                                                         n_heads=spatial_n_heads, mlp_bias=mlp_bias, attn_bias=attn_bias)
                                                   for _ in range(spatial_n_layers)])
        self.depth_transformer = nn.Sequential(*[Block(ctx_len=depth_num_tokens, cond_len=0, embed_dim=embed_dim, n_heads=depth_n_heads,
                                                       mlp_bias=mlp_bias, attn_bias=attn_bias) for _ in range(depth_n_layers)])
        self.ln_spatial = nn.LayerNorm(embed_dim)
        self.ln_depth = nn.LayerNorm(embed_dim)
        self.head = nn.Linear(embed_dim, vocab_img_size, bias=False)
        self.apply(self._init_weights)
        self._operands = {}       # operand format -> (versions of the masters, operand copies)
        self._fwd_states = {}     # (chunk, dtype, device) -> the buffers of forward()
        self.forward_hidden_cap = FORWARD_HIDDEN_CAP

    _init_weights = GPT._init_weights
    _on_device_conds = GPT._on_device_conds
    _operand_dtype = staticmethod(GPT._operand_dtype)

    @torch.no_grad()
    def forward(self, codes: torch.Tensor, conds: torch.Tensor, *, use_fp16: bool = True, return_loss: bool = False):
        """reference layers.py:370-395: logits [B T, D, V] (f32) of every code given the condition, the positions before it and the shallower
        codes of its own position; with return_loss=True (logits, nll [B T, D], mean): the cross-entropy against `codes` and its mean (the
        reference's val/total_loss), both on the device.  codes [B, T, D] (or [B, h, w, D]), conds [B] or [B, 1].

        Inference only: the call runs under torch.no_grad.  The spatial stream has S = T rows (the condition and the first T - 1 positions:
        position T - 1's codes reach only its own depth slots).  use_fp16=True runs the 16-bit operand format of ENH_PRECISION as GPT.forward
        does, with the short-sequence attention (csrc/rq_prefill.hip) in the depth transformer; ENH_RQ_DEPTH_ATTN=tile runs it on the tile kernel
        of the spatial transformer at N = D instead (A/B only).  False is the exact mode.  Device tensors only.  Batches run in chunks of whole
        images sized so that the depth transformer's hidden activation ([chunk T D, 4C], f32 and its operand copy) stays under
        `forward_hidden_cap` bytes.  A module whose parameters are not on the device of `codes` is moved there."""
        if not (torch.is_tensor(codes) and torch.is_tensor(conds) and codes.is_cuda and conds.is_cuda):
            raise NotImplementedError("RQTransformer.forward runs on a ROCm device only: codes and conds must be device tensors (there is no CPU path "
                                      "for the teacher-forced forward)")
        from ... import _C
        dev = codes.device
        B, T, D, V = codes.shape[0], self.img_num_tokens, self.depth_num_tokens, self.vocab_img_size
        if codes.shape[-1] != D or codes.numel() != B * T * D:
            raise ValueError(f"RQTransformer.forward: codes must be [B, img_num_tokens = {T}, depth_num_tokens = {D}], got {tuple(codes.shape)}")
        codes = codes.reshape(B, T, D).to(torch.int64).contiguous()
        conds = self._on_device_conds(conds, B, "RQTransformer.forward")
        if int(codes.min()) < 0 or int(codes.max()) >= V:
            raise ValueError(f"RQTransformer.forward: codes outside [0, {V})")
        if int(conds.min()) < 0 or int(conds.max()) >= self.vocab_cond_size:
            raise ValueError(f"RQTransformer.forward: conds outside [0, {self.vocab_cond_size})")
        dt = self._operand_dtype(use_fp16, "RQTransformer.forward")
        chunk = max(1, min(B, int(self.forward_hidden_cap) // (T * D * 4 * self.embed_dim * (4 + (2 if use_fp16 else 0)))))
        logits = torch.empty(B * T, D, V, dtype=torch.float32, device=dev)
        nll = torch.empty(B * T, D, dtype=torch.float32, device=dev) if return_loss else None
        st = self._forward_state(chunk, dt, dev)
        for s in range(0, B, chunk):
            e = min(s + chunk, B)
            self._forward_rows(st, codes[s:e], conds[s:e], logits[s * T:e * T], dt)
            if return_loss:
                _C.cross_entropy_rows(logits[s * T:e * T].view(-1, V), codes[s:e].reshape(-1), nll[s * T:e * T].view(-1))
        if not return_loss:
            return logits
        mean = torch.empty(1, dtype=torch.float32, device=dev)
        _C.mean_f32(nll.view(-1), mean)
        return logits, nll, mean[0]

    def _forward_state(self, b: int, dt: torch.dtype, dev) -> dict:
        """the buffers of a chunk of b images, kept per (b, dtype): the spatial stream xs [b T, C], the depth stream xd [b T D, C] and the
        activations at the depth transformer's row count, whose leading b T rows serve the spatial transformer"""
        key = (b, dt, str(dev))
        st = self._fwd_states.get(key)
        if st is None:
            f32, C, Ms = torch.float32, self.embed_dim, b * self.img_num_tokens
            M = Ms * self.depth_num_tokens
            e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
            st = dict(xs=e(Ms, C, dtype=f32), xd=e(M, C, dtype=f32), x2=e(M, C, dtype=f32), a=e(M, C), qkv=e(M, 3 * C), att=e(M, C),
                      hid32=e(M, 4 * C, dtype=f32), hid=e(M, 4 * C) if dt != f32 else None)
            self._fwd_states = {key: st}      # one chunk size at a time
        return st

    def _embed_channels(self, codes, conds, xs, xd) -> None:
        """code_sum="channels": the reference's cumsum along the embedding channels, with torch ops on the device"""
        b, T, D = codes.shape
        C = self.embed_dim
        cs = self.tok_emb_code.weight.detach()[codes].cumsum(-1)      # [b, T, D, C]
        xs = xs.view(b, T, C)
        xs[:, 0] = self.tok_emb_cond.weight.detach()[conds] + self.pos_emb_cond.detach()[0, 0]
        xs[:, 1:] = cs[:, :T - 1, D - 1] + self.pos_emb_code.detach()[0, :T - 1]
        xd.view(b * T, D, C)[:, 1:] = cs[:, :, :D - 1].reshape(b * T, D - 1, C) + self.pos_emb_depth.detach()[0]

    def _forward_rows(self, st, codes, conds, logits, dt) -> None:
        """one chunk of b whole images: logits [b T, D, V] f32.  The embedding stage, the spatial Blocks over b sequences of T rows (GPT's launches),
        ln_spatial into slot 0 of the depth stream, the depth Blocks over b T sequences of D rows, ln_depth and the head."""
        from ... import _C
        b, T, D, C, V = codes.shape[0], self.img_num_tokens, self.depth_num_tokens, self.embed_dim, self.vocab_img_size
        Ms, M = b * T, b * T * D
        Hs, Hd = self.spatial_n_heads, self.depth_n_heads
        ops = self._operand_copies(dt)
        xs, xd = st["xs"][:Ms], st["xd"][:M]
        if self.code_sum == "depth":
            _C.rq_embed_seq(conds, codes, self.tok_emb_cond.weight.detach(), self.pos_emb_cond.detach()[0, 0], self.tok_emb_code.weight.detach(),
                            self.pos_emb_code.detach()[0], self.pos_emb_depth.detach()[0], xs.view(b, T, C), xd.view(Ms, D, C))
        else:
            self._embed_channels(codes, conds, xs, xd)
        x2, a, qkv, att, hid32, hid = (None if st[k] is None else st[k][:Ms] for k in ("x2", "a", "qkv", "att", "hid32", "hid"))
        linear = _row_linear(Ms, dt)
        for blk, W in zip(self.spatial_transformer, ops["spatial"]):
            _block_rows(blk, W, linear, dt, T, lambda q, o: _C.causal_attention(q, b, T, Hs, C // Hs, o), xs, xs, a, a, qkv, att, x2, hid32, hid)
        _C.ln_rows_strided(xs, self.ln_spatial.weight, self.ln_spatial.bias, xd, D * C, eps=self.ln_spatial.eps)
        x2, a, qkv, att, hid32, hid = (None if st[k] is None else st[k][:M] for k in ("x2", "a", "qkv", "att", "hid32", "hid"))
        linear = _row_linear(M, dt)
        if dt == torch.float32 or os.environ.get("ENH_RQ_DEPTH_ATTN") == "tile":
            attention = lambda q, o: _C.causal_attention(q, Ms, D, Hd, C // Hd, o)
        else:
            attention = lambda q, o: _C.short_causal_attention(q, Ms, D, Hd, C // Hd, o)
        for blk, W in zip(self.depth_transformer, ops["depth"]):
            _block_rows(blk, W, linear, dt, D, attention, xd, xd, a, a, qkv, att, x2, hid32, hid)
        _C.ln_timeshift(xd, self.ln_depth.weight, self.ln_depth.bias, a, D, eps=self.ln_depth.eps)
        linear(a, ops["head"], logits.view(M, V))

    def _operand_copies(self, dt: torch.dtype):
        """the GEMM weights in the operand format `dt`, built once from the fp32 masters and rebuilt when a master was replaced or written in
        place (load_state_dict): the masters' version counters are the key, as in GPT._operand_copies"""
        masters = [p for _, p in sorted(self.named_parameters())]
        key = tuple((p.data_ptr(), p._version) for p in masters)
        hit = self._operands.get(dt)
        if hit is not None and hit[0] == key:
            return hit[1]
        cast = (lambda w: w.detach().to(dt).contiguous())
        ops = dict(spatial=_layer_operands(self.spatial_transformer, cast), depth=_layer_operands(self.depth_transformer, cast),
                   head=cast(self.head.weight))
        self._operands[dt] = (key, ops)
        return ops
