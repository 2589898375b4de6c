"""The stage-2 priors (reference enhancing/modules/stage2/layers.py): parameter containers with the reference's names, shapes and init, so its
checkpoints and yaml load, and what runs them on the device.  What the two priors share (one Block's launches forward and backward, the operand
copies, the input checks, the chunked teacher-forced driver, the limits) is prior.py; the optimizer step is engine/optim.py GPTAdam.

`GPT` (reference layers.py:23-303), three entries:
  * `sample` is the reference's cached sampling loop restated per step, one token per batch row.  Under the cache the block
    sees T == 1, where `time_shift(x)` is all zeros and the mix `x * time_mix + time_shift(x) * (1 - time_mix)` is `ln1(x) * time_mix`.  That is
    NOT what the teacher-forced `forward` computes (there the shifted term is the previous token's ln1 row): two contracts, two goldens
    (tests/golden/gpt_<case>.npz, gpt_fwd_<case>.npz).  Nothing in the loop reads a device value on the host.
  * `forward` runs whole sequences (§3.6): the embedding of [B, S, C] in one launch, the Blocks (`_block_rows`), the final LayerNorm and the
    head; optionally the per-position cross-entropy and its mean.  Inference only: no autograd graph.
  * `forward_backward` is that forward with its activations kept per layer, then a hand-written backward (§3.7; `_block_rows_backward`): weight
    gradients accumulate in f32 into one flat buffer that every `p.grad` is a view into.  16-bit operand formats only.

`RQTransformer` (reference layers.py:306-547), the prior over a residual quantizer's [B, T, D] codes: `forward` (§3.9), `forward_backward`
(§3.10) and `sample` (§3.11).  Its spatial and depth transformers are stacks of the same Blocks; the embedding stage, ln_spatial into slot 0 of the
depth sequences and the attention over B T sequences of D <= 8 slots are csrc/rq_prefill.hip, their backward csrc/rq_backward.hip.  `sample` is the
spatial / depth decode loop: both stacks run GPT's decode launches (prior.py `_block_step`), the spatial one under a cache of T slots, the depth
one under a cache of D slots; a step's input row and the attention over the short cache are csrc/rq_decode.hip.

Both `sample` entries take `graph=` (None: ENH_GRAPHS == "1"): position 0 runs as above, then ONE position is captured into a
HIP graph per chunk and replayed T - 1 times (prior.py `_sample_graphed`).  The captured launches take the position from a device int32, the
cursor: the attention over the long cache, the step's input row and the draw have cursor forms (enh_decode_attention_at, enh_embed_step_at,
enh_sample_logits_at) that run the bodies of their by-value siblings, and enh_cursor_advance ends the position.  The same bits as the loop.

Both also take `weights=` (None: ENH_SAMPLE_WEIGHTS, default "h16"): "fp8" streams every Linear of every Block as an MXFP8
operand (e4m3fn codes, one E8M0 scale per 32 k; prior.py `_sample_operands`) through enh_skinny_gemm_w8 (csrc/gpt_decode_w8.hip); the head,
the activations and the caches stay 16-bit.  "fp4" does the same with MXFP4 operands (two e2m1 codes per byte, the same scales)
through enh_skinny_gemm_w4 (csrc/gpt_decode_w4.hip): a quarter of the weight bytes, and a format that moves the logits far more.  "fp6" lies between them: MXFP6 operands (e2m3 codes, 32 to 24
bytes in the order the product consumes them, the same scales) through enh_skinny_gemm_w6 (csrc/gpt_decode_w6.hip), 0.76 of fp8's
weight bytes at fp8's accuracy on block-scaled weights.  The three step methods choose their product through prior.py `_step_linear`.

Both also take `cache=` (None: ENH_SAMPLE_CACHE, default "h16"): "fp8" holds every cache that enh_decode_attention serves (all
Blocks of GPT, the spatial stack of RQTransformer) as MXFP8 codes and scales with the blocks along the head dimension (prior.py `_kv_caches`)
and attends through enh_decode_attention_kv8 (csrc/gpt_decode_kv8.hip), which quantizes the step's k / v rows as it appends them; the RQ depth
caches stay 16-bit.  The step methods choose the launch through prior.py `_step_attention`.

Both also take `prefix_codes=`: the first P positions are GIVEN and the rest is drawn, which is image completion and the
resumption of a partly drawn image.  The given codes enter the caches through one batched prefill per chunk (`_prefill`; prior.py
`_prefill_stack`): the teacher-forced forward's launches at S = 1, i.e. under the SAMPLER's model, with the rows' k / v written into slots
0 .. P - 1 by enh_kv_cache_fill / enh_kv_cache_fill_kv8 (csrc/gpt_prefill_cache.hip) and the tile attention over N = P; the loop then runs
positions P .. T - 1 unchanged, under graph=True from a cursor that starts at P + 1.  CondTransformer.complete is the public form.

Left out: per-row prefix lengths, a prefix for the RQ depth stack, caches kept from call to call, a wide (prefill-shaped) product for MX
weights, an exact-f32 backward, more than one condition token, HIP-graph capture of position 0 and of the teacher-forced entries, graphs kept
from call to call, relu^2 / LayerNorm fused into GEMM epilogues, 8-bit activations (W8A8), an 8-bit form of the RQ depth caches, the e3m2
form of MXFP6, a quantized head, MXFP8 / MXFP6 / MXFP4 in the teacher-forced entries, W4A8 / W6A8 on the scaled MFMA, quantized checkpoints on disk."""
import os
from typing import Optional, Tuple

import torch
import torch.nn as nn

from .prior import (FORWARD_HIDDEN_CAP, MAX_BATCH, MAX_EMBED, MAX_HEAD, MAX_TOKENS, MAX_VOCAB, OPERAND_DTYPE, Prior,  # noqa: F401  (re-exported)
                    _block_rows, _block_rows_backward, _block_step, _grad_linears, _kv_caches, _prefill_buffers, _prefill_stack, _row_linear,
                    _step_attention, _step_linear)

BACKWARD_SAVED_CAP = 16 << 30  # bytes of forward_backward()'s saved activations: shipped size 24 x 172,096 B per token, 4 sequences of 1024 per chunk
MAX_DEPTH = 8           # enh_rq_embed_seq, enh_short_causal_attention_forward: the stage-1 residual quantizer's cap on num_quantizers
CODE_SUMS = ("depth", "channels")
SLOT0_LNS = ("once", "twice")     # RQTransformer.sample: how often ln_depth is applied to depth slot 0


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


class GPT(Prior):
    STACKS = {"layers": "blocks"}

    def __init__(self, vocab_cond_size: int, vocab_img_size: int, embed_dim: int, cond_num_tokens: int, img_num_tokens: int, n_heads: int,
                 n_layers: int, mlp_bias: bool = True, attn_bias: bool = True) -> None:
        super().__init__(vocab_cond_size, vocab_img_size, embed_dim, cond_num_tokens, img_num_tokens, n_heads=n_heads)
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
        self.backward_saved_cap = BACKWARD_SAVED_CAP      # bytes of forward_backward()'s saved activations of all layers in one chunk
        self._bwd_states = {}     # (chunk, dtype, device) -> the buffers of forward_backward()

    # ---- teacher-forced forward -------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, codes: torch.Tensor, conds: torch.Tensor, *, use_fp16: bool = True, return_loss: bool = False):
        """reference layers.py:193-211: logits [B, T, V] (f32) of every code given the condition and the codes before it; with return_loss=True
        (logits, nll [B, T], mean): the per-position cross-entropy against `codes` and its mean (the reference's val/total_loss), both on the device.

        Inference only: the call runs under torch.no_grad and the result carries no autograd graph (training is forward_backward).
        S = T rows are built, the condition and the first T - 1 codes: the causal mask keeps the last code's row from every logit that is kept.
        use_fp16=True runs the 16-bit operand format of ENH_PRECISION (default fp16) through enh_gemm_h16 and the MFMA causal attention; biases,
        residuals and LayerNorms stay on the f32 residual stream.  False is the exact mode: f32 operands, tree-ordered sums (enh_skinny_gemm_f32
        in 64-row pieces), the f32 attention instrument.  Device tensors only.  Batches run in chunks of whole sequences sized so that the hidden
        activation of the MLP ([chunk T, 4C], f32 and its operand copy) stays under `forward_hidden_cap` bytes.
        Side effect, as in sample(): a module whose parameters are not on the device of `codes` is moved there."""
        return self._teacher_forced("GPT.forward", codes, conds, use_fp16, return_loss, "there is no CPU path for the teacher-forced forward; note "
                                    "that the cached sample() does not compute the same logits: time_shift")

    def _forward_buffers(self, b: int, dt: torch.dtype, dev) -> dict:
        """the buffers of a chunk of b sequences"""
        f32, C, M = torch.float32, self.embed_dim, b * self.img_num_tokens
        e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
        return dict(x=e(M, C, dtype=f32), x2=e(M, C, dtype=f32), a=e(M, C), qkv=e(M, 3 * C), att=e(M, C), hid32=e(M, 4 * C, dtype=f32),
                    hid=e(M, 4 * C) if dt != f32 else None)

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

        def bufs(i: int):
            """_block_rows' buffers of layer i (x, x_out, a, a2, qkv, att, x2, hid32, hid), then the attention's lse"""
            if saved is None:
                return x, x, a, a, qkv, att, x2, hid32, hid, None
            sv = saved[i]
            return (sv["x"][:M], saved[i + 1]["x"][:M] if i + 1 < len(saved) else x, sv["a"][:M], sv["a2"][:M], sv["qkv"][:M], sv["att"][:M],
                    sv["x2"][:M], hid32, sv["hid"][:M], sv["lse"][:b * H * T])

        _C.gpt_embed_seq(conds, codes, self.tok_emb_cond.weight.detach(), self.pos_emb_cond.detach()[0, 0], self.tok_emb_code.weight.detach(),
                         self.pos_emb_code.detach()[0], bufs(0)[0].view(b, T, C))
        for i, (blk, W) in enumerate(zip(self.blocks, ops["layers"])):
            *rows, lse = bufs(i)
            _block_rows(blk, W, linear, dt, T, lambda qkv_, att_: _C.causal_attention(qkv_, b, T, H, hs, att_, lse=lse), *rows)
        _C.ln_timeshift(x, self.layer_norm.weight, self.layer_norm.bias, a, T, eps=self.layer_norm.eps)
        linear(a, ops["head"], logits.view(M, V))

    # ---- teacher-forced loss and its gradients -----------------------------------------------------
    def saved_bytes_per_token(self) -> int:
        """bytes forward_backward keeps per token row for ALL layers: per layer the f32 inputs of ln1 and ln2 (4C + 4C), the
        16-bit operands a, qkv, att, a2 and hid (2C + 6C + 2C + 2C + 8C) and the attention's lse (4 H)"""
        return len(self.blocks) * (28 * self.embed_dim + 4 * self.n_heads)

    def _backward_buffers(self, b: int, dt: torch.dtype, dev) -> dict:
        """the buffers of a chunk of b sequences: row counts rounded up to 8 (the contraction length of a weight-gradient product), everything
        zero at first so that the tail rows of an operand are finite; the tail rows of the gradient operands are zeroed again for a shorter chunk"""
        f32, C, H, V, T = torch.float32, self.embed_dim, self.n_heads, self.vocab_img_size, self.img_num_tokens
        Mp = (b * T + 7) // 8 * 8
        z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype, device=dev)
        saved = [dict(x=z(Mp, C, dtype=f32), a=z(Mp, C), qkv=z(Mp, 3 * C), att=z(Mp, C), lse=z(b * H * T, dtype=f32), x2=z(Mp, C, dtype=f32),
                      a2=z(Mp, C), hid=z(Mp, 4 * C)) for _ in self.blocks]
        return dict(saved=saved, x=z(Mp, C, dtype=f32), a=z(Mp, C), hid32=z(Mp, 4 * C, dtype=f32), logits=z(Mp, V, dtype=f32), dlogits=z(Mp, V),
                    g=z(Mp, C, dtype=f32), g2=z(Mp, C, dtype=f32), d32=z(Mp, C, dtype=f32), g16=z(Mp, C), dh16=z(Mp, 4 * C), dqkv=z(Mp, 3 * C),
                    datt=z(Mp, C), dbqkv=z(3 * C, dtype=f32))

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
        return self._teacher_forced_backward("GPT.forward_backward", codes, conds, use_fp16, loss_scale, accumulate,
                                             self.img_num_tokens * self.saved_bytes_per_token())

    def _backward_rows(self, st, codes, conds, nll, dt, gscale: float, accumulate: bool, gscale_dev=None) -> None:
        """one chunk: the saving forward, then the backward of DESIGN.md §3.7, setting (accumulate=False) or adding to every parameter's gradient:
        the head, the final LayerNorm, the Blocks last to first (`_block_rows_backward`), the embedding"""
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
        wgrad, dgrad = _grad_linears(M, Mp, accumulate)
        if gscale_dev is None:
            _C.cross_entropy_backward(logits, codes.reshape(-1), nll.view(-1), dlogits, gscale)
        else:
            _C.cross_entropy_backward(logits, codes.reshape(-1), nll.view(-1), dlogits, gscale, gscale_dev=gscale_dev)
        wgrad(st["dlogits"], st["a"], self.head.weight.grad, V, C)
        dgrad(dlogits, ops["head"], d32)
        ln = self.layer_norm
        _C.ln_timeshift_backward(d32, st["x"][:M], ln.weight, T, g, ln.weight.grad, ln.bias.grad, dx16=g16, eps=ln.eps, accumulate=accumulate)

        def attention_backward(sv, datt_, dqkv_):
            _C.causal_attention_backward(sv["qkv"][:M], sv["att"][:M], datt_, sv["lse"][:b * H * T], b, T, H, hs, dqkv_)

        for i in range(len(self.blocks) - 1, -1, -1):
            _block_rows_backward(self.blocks[i], ops["layers"][i], wgrad, dgrad, accumulate, T, attention_backward, saved[i], st,
                                 g, g2, d32, g16, dh16, dqkv, datt, hid32)
        _C.gpt_embed_seq_backward(g.view(b, T, C), conds, codes, self.tok_emb_cond.weight.grad, self.pos_emb_cond.grad.view(-1), self.tok_emb_code.weight.grad,
                                  self.pos_emb_code.grad.view(-1, C), accumulate)

    # ---- sampling -------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, conds: torch.Tensor, top_k: Optional[float] = None, top_p: Optional[float] = None, softmax_temperature: float = 1.0,
               use_fp16: bool = True, *, seed: Optional[int] = None, forced_codes: Optional[torch.Tensor] = None, return_logits: bool = True,
               call: int = 0, row_offset: int = 0, graph: Optional[bool] = None, weights: Optional[str] = None,
               cache: Optional[str] = None, prefix_codes: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """reference layers.py:213-266: returns (logits [B, T*V] after the temperature and the top-k mask, codes [B, T]).

        prefix_codes [B, P] (anything with B rows that reshapes to it, e.g. [B, h', w]; 0 <= P < T, ids in [0, V), else a ValueError) CONTINUES an
        image: positions < P are given, positions >= P are drawn (or fed from forced_codes) exactly as without it, under the step
        numbers t and so the uniforms of a full run.  The given codes enter the k / v caches through one batched prefill per chunk instead of P
        weight-streaming steps: the rows of the condition and of codes 0 .. P - 2 go through every Block but the last layer's attention, proj and
        MLP under the SAMPLER's model (every row is ln1(x) * time_mix, no previous-row term), their k / v rows fill slots 0 .. P - 1
        (enh_kv_cache_fill, for cache="fp8" enh_kv_cache_fill_kv8) and enh_causal_attention_forward attends over them; the products are enh_gemm_h16
        over all rows, or under weights="fp8" | "fp6" | "fp4" the step's own product in pieces of 64 rows (the codes are re-read once per piece).
        The returned codes[:, :P] is the prefix; the logits of positions < P are NOT computed and are returned as NaN.  With forced_codes its
        first P positions must equal the prefix (a ValueError).  P == 0 is the call without a prefix, launch for launch.  Under graph=True the
        prefill and position P run eagerly, and the captured position is replayed T - P - 1 times.

        graph=True replays every position after the first from ONE captured HIP graph per chunk: the launches of a position
        in their cursor forms, which read the position from device memory; the same bits as the loop.  None reads ENH_GRAPHS == "1", False is the
        loop.  Captured per call, nothing is cached between calls; while per-kernel timing is on (_C.TIMER) the loop runs.

        weights="fp8" streams every Linear of every Block (q|k|v, proj, p0, p1) as its MXFP8 operand (e4m3fn codes and one
        E8M0 scale per 32 k, quantized once from the f32 masters) through enh_skinny_gemm_w8: half the weight bytes of a step and of the operand
        copies; the head, activations and caches stay in the 16-bit format.  "h16" is the 16-bit weights; None reads ENH_SAMPLE_WEIGHTS (default
        "h16").  It needs use_fp16=True and composes with graph=True (a different launch in the captured position).
        weights="fp4" is the same with MXFP4 operands (two e2m1 codes per byte and the same scales) through enh_skinny_gemm_w4: a
        quarter of the weight bytes, at 0.14 - 0.19 relative logit shift on random Gaussian models against fp8's 0.04 - 0.05.
        weights="fp6" is the same with MXFP6 operands (e2m3 codes, 0.78 bytes per weight, the same scales) through
        enh_skinny_gemm_w6: 0.76 of fp8's weight bytes at 0.036 - 0.046 relative logit shift on the same models, which is fp8's.

        cache="fp8" holds every layer's k / v cache as MXFP8 codes and scales (blocks of 32 along the head dimension, 1 + 1/32 bytes
        per element instead of 2) and attends through enh_decode_attention_kv8: the step's k / v rows are quantized as they are appended, and the
        step's own attention reads them quantized too.  "h16" is the 16-bit caches; None reads ENH_SAMPLE_CACHE (default "h16").  It needs
        use_fp16=True and composes with graph=True and weights="fp8".

        use_fp16=True runs the 16-bit operand format of ENH_PRECISION (default fp16) with f32 accumulation; False the exact mode (f32 operands on the vector ALU, f32 cache and
        row kernels).  The draw is an inverse-CDF walk in index order with one uniform per (seed, call, step, row_offset + row): the distribution of
        the reference's torch.multinomial, not its bits; a seed gives the same codes on every run (seed=None draws one from torch's generator).
        forced_codes [B, T] feeds the given codes to the next step instead of the drawn ones (codes are still drawn and returned).
        Batches above 64 rows run in chunks of 64 rows.
        Side effect: a module whose parameters are not on the device of `conds` is MOVED there (`self.to(conds.device)`) on the first call, as the
        stage-1 engine moves its model; the reference leaves that to the caller."""
        prefix_codes = self._check_prefix(prefix_codes, conds.shape[0], "GPT.sample")
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
        weights = self._sample_weights(weights, use_fp16, "GPT.sample")
        cache = self._sample_cache(cache, use_fp16, "GPT.sample")
        codes = torch.empty(B, T, dtype=torch.int64, device=dev)
        logits = torch.empty(B, T * V, dtype=torch.float32, device=dev) if return_logits else None
        if prefix_codes is not None:
            prefix_codes = self._place_prefix(prefix_codes, forced_codes, codes, logits, "GPT.sample")
        if self._use_graph(graph):
            state = lambda b: self._decode_state(b, dt, dev, weights=weights, cache=cache)
            self._sample_graphed(B, dev, state, lambda st, s, e, positions: self._sample_rows_graphed(
                st, positions, conds[s:e], codes[s:e], None if logits is None else logits[s:e], None if forced_codes is None else forced_codes[s:e],
                top_k, top_p, float(softmax_temperature), seed, call, row_offset + s, None if prefix_codes is None else prefix_codes[s:e]))
            return logits, codes
        for s in range(0, B, MAX_BATCH):
            e = min(s + MAX_BATCH, B)
            self._sample_rows(conds[s:e], codes[s:e], None if logits is None else logits[s:e], None if forced_codes is None else forced_codes[s:e],
                              dt, top_k, top_p, float(softmax_temperature), seed, call, row_offset + s, weights, cache,
                              None if prefix_codes is None else prefix_codes[s:e])
        return logits, codes

    def _sample_rows(self, conds, codes, logits, forced, dt, top_k, top_p, temperature, seed, call, row0, weights: str = "h16", cache: str = "h16",
                     prefix=None):
        from ... import _C
        T, V = self.img_num_tokens, self.vocab_img_size
        st = self._decode_state(conds.shape[0], dt, conds.device, weights=weights, cache=cache)
        feed = codes if forced is None else forced
        P = 0 if prefix is None else prefix.shape[1]
        if P:
            self._prefill(st, conds, prefix)
        for t in range(P, T):
            self._decode_step(st, t, conds if t == 0 else feed[:, t - 1])
            _C.sample_logits(st["logits"], codes[:, t], temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, call=call, step=t, row0=row0,
                             logits_out=None if logits is None else logits[:, t * V:(t + 1) * V])

    def _sample_rows_graphed(self, st, positions, conds, codes, logits, forced, top_k, top_p, temperature, seed, call, row0, prefix=None):
        """_sample_rows for Prior._sample_graphed: position 0 (under a prefix of P positions the prefill and position P) as there, every later one
        the same launches in their cursor forms"""
        from ... import _C
        V = self.vocab_img_size
        feed = codes if forced is None else forced
        draw = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, call=call, row0=row0)
        P = 0 if prefix is None else prefix.shape[1]

        def first():
            if P:
                self._prefill(st, conds, prefix)
            self._decode_step(st, P, feed[:, P - 1] if P else conds)
            _C.sample_logits(st["logits"], codes[:, P], step=P, logits_out=None if logits is None else logits[:, P * V:(P + 1) * V], **draw)

        def later(cursor):
            self._decode_step(st, None, feed, cursor=cursor)
            _C.sample_logits_at(st["logits"], codes, cursor, logits_out=logits, **draw)

        positions(self.img_num_tokens, first, later, P)

    def _prefill(self, st: dict, conds, prefix) -> None:
        """the given codes prefix [b, P] of a chunk put into slots 0 .. P - 1 of every layer's cache of `st` (prior.py `_prefill_stack`): rows
        s = 0 .. P - 1 (the condition, then codes 0 .. P - 2) are built in one embedding launch per group of whole sequences"""
        from ... import _C
        (b, P), C = prefix.shape, self.embed_dim
        pf = _prefill_buffers(b, P, C, st["dt"], prefix.device, self.forward_hidden_cap)
        for b0 in range(0, b, pf["g"]):
            n = min(pf["g"], b - b0)
            _C.gpt_embed_seq(conds[b0:b0 + n], prefix[b0:b0 + n], self.tok_emb_cond.weight.detach(), self.pos_emb_cond.detach()[0, 0],
                             self.tok_emb_code.weight.detach(), self.pos_emb_code.detach()[0], pf["x"][:n * P].view(n, P, C))
            _prefill_stack(self.blocks, st["ops"]["layers"], st["caches"], b0, n, P, self.n_heads, st["dt"], pf)

    def _decode_state(self, b: int, dt: torch.dtype, dev, cache_len: Optional[int] = None, weights: str = "h16", cache: str = "h16") -> dict:
        """the buffers of one chunk of b <= 64 rows: residual stream, activations, the step's logits and every layer's k / v cache [b, H, T, hs]
        in the form of `cache` (prior.py `_kv_caches`); ops: the operands of `weights` (prior.py `_sample_operands`)"""
        f32, C, H = torch.float32, self.embed_dim, self.n_heads
        T = cache_len or self.img_num_tokens
        e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
        return dict(dt=dt, b=b, x=e(b, C, dtype=f32), x2=e(b, C, dtype=f32), a=e(b, C), qkv=e(b, 3 * C), att=e(b, C), hid=e(b, 4 * C),
                    logits=e(b, self.vocab_img_size, dtype=f32), caches=_kv_caches(len(self.blocks), b, H, T, C // H, dt, dev, cache),
                    ops=self._sample_operands(dt, weights))

    def _decode_step(self, st: dict, t: Optional[int], ids: torch.Tensor, cursor: Optional[torch.Tensor] = None) -> None:
        """one token per row: ids (int64, on the device: the condition at t == 0, else the previous step's codes) -> st["logits"] [b, V] f32.
        The cursor form (cursor: device int32 [1], t is None): the step t >= 1 the cursor holds; ids is then the whole [b, T] tensor of the codes
        that are fed forward, whose column t - 1 the embedding reads on the device."""
        from ... import _C
        x, x2, a, qkv, att, hid = st["x"], st["x2"], st["a"], st["qkv"], st["att"], st["hid"]
        linear = _step_linear(st["dt"])
        if cursor is not None:
            C = self.embed_dim
            _C.embed_step_at(self.tok_emb_code.weight.detach(), ids, 1, 1, -1, self.pos_emb_code.detach()[0], C, -C, cursor, 1, self.img_num_tokens, x)
        else:
            if t == 0:
                _C.gpt_embed(self.tok_emb_cond.weight.detach(), ids, self.pos_emb_cond.detach()[0, 0], x)
            else:
                _C.gpt_embed(self.tok_emb_code.weight.detach(), ids, self.pos_emb_code.detach()[0, t - 1], x)
        attend = _step_attention(t, cursor)
        for blk, W, kv in zip(self.blocks, st["ops"]["layers"], st["caches"]):
            _block_step(blk, W, linear, lambda q, o: attend(q, kv, o), x, x2, a, qkv, att, hid)
        _C.row_ln_scale(x, self.layer_norm.weight, self.layer_norm.bias, a, eps=self.layer_norm.eps)
        linear(a, st["ops"]["head"], st["logits"])


class RQTransformer(Prior):
    """reference layers.py:306-395: a spatial transformer over the T positions of an image, whose input at a position is built from the D residual
    codes of the position before it, and a depth transformer over the D slots of every position: slot 0 is ln_spatial of the spatial output, slot
    d >= 1 is built from codes 0 .. d - 1 of the position; logits [B T, D, V].  The reference's constructor arguments, parameter names, shapes and
    init.  Built here: the teacher-forced forward, the validation loss, forward_backward (training: engine/optim.py GPTAdam) and sample.

    The code-sum quirk.  The reference's forward computes `codes.cumsum(-1)` on the [B, T, D, C] embeddings: a running sum along the embedding
    CHANNELS, not along depth.  Its own sampler (sample_spatial_step / sample_depth_step: `codes.sum(1)`) and the RQ-VAE formulation sum over
    DEPTH, so a model trained through the reference's forward is not the model its sampler draws from.  Keyword `code_sum` selects:
      "depth" (default)   spatial row t + 1 = sum_j emb(code[b, t, j]) + pos_emb_code[t]; slot d >= 1 = sum_{j < d} emb(code[b, t, j]) +
                          pos_emb_depth[d - 1]: what the sampler assumes; one launch (enh_rq_embed_seq)
      "channels"          the reference's line in meaning: spatial row t + 1 = cumsum_C(emb(code[b, t, D - 1])) + pos_emb_code[t]; slot d =
                          cumsum_C(emb(code[b, t, d - 1])) + pos_emb_depth[d - 1].  A parity instrument (the reference's own forward is then the
                          golden of everything behind the embedding): the two input tensors are built with torch ops on the device, every launch
                          after them is the default mode's."""
    STACKS = {"spatial": "spatial_transformer", "depth": "depth_transformer"}

    def __init__(self, vocab_cond_size: int, vocab_img_size: int, embed_dim: int, cond_num_tokens: int, img_num_tokens: int, depth_num_tokens: int,
                 spatial_n_heads: int, depth_n_heads: int, spatial_n_layers: int, depth_n_layers: int, mlp_bias: bool = True, attn_bias: bool = True,
                 *, code_sum: str = "depth") -> None:
        super().__init__(vocab_cond_size, vocab_img_size, embed_dim, cond_num_tokens, img_num_tokens, spatial_n_heads=spatial_n_heads,
                         depth_n_heads=depth_n_heads)
        if depth_num_tokens == 1:
            raise ValueError("RQTransformer: depth_num_tokens == 1 is one code per position: use GPT")
        if not 2 <= depth_num_tokens <= MAX_DEPTH:
            raise ValueError(f"RQTransformer: depth_num_tokens must be in [2, {MAX_DEPTH}] (the residual quantizer's num_quantizers), got {depth_num_tokens}")
        if code_sum not in CODE_SUMS:
            raise ValueError(f"RQTransformer: code_sum must be one of {CODE_SUMS}, got {code_sum!r}")
        self.depth_num_tokens = depth_num_tokens
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
        self.backward_saved_cap = BACKWARD_SAVED_CAP      # bytes of forward_backward()'s saved activations of all layers in one chunk
        self._bwd_states = {}     # (chunk, dtype, device) -> the buffers of forward_backward()

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
        return self._teacher_forced("RQTransformer.forward", codes, conds, use_fp16, return_loss, "there is no CPU path for the teacher-forced forward")

    def _forward_buffers(self, b: int, dt: torch.dtype, dev) -> dict:
        """the buffers of a chunk of b images: the spatial stream xs [b T, C], the depth stream xd [b T D, C] and the activations at the depth
        transformer's row count, whose leading b T rows serve the spatial transformer"""
        f32, C, Ms = torch.float32, self.embed_dim, b * self.img_num_tokens
        M = Ms * self.depth_num_tokens
        e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
        return dict(xs=e(Ms, C, dtype=f32), xd=e(M, C, dtype=f32), x2=e(M, C, dtype=f32), a=e(M, C), qkv=e(M, 3 * C), att=e(M, C),
                    hid32=e(M, 4 * C, dtype=f32), hid=e(M, 4 * C) if dt != f32 else None)

    def _embed_channels(self, codes, conds, xs, xd) -> None:
        """code_sum="channels": the reference's cumsum along the embedding channels, with torch ops on the device"""
        b, T, D = codes.shape
        C = self.embed_dim
        cs = self.tok_emb_code.weight.detach()[codes].cumsum(-1)      # [b, T, D, C]
        xs = xs.view(b, T, C)
        xs[:, 0] = self.tok_emb_cond.weight.detach()[conds] + self.pos_emb_cond.detach()[0, 0]
        xs[:, 1:] = cs[:, :T - 1, D - 1] + self.pos_emb_code.detach()[0, :T - 1]
        xd.view(b * T, D, C)[:, 1:] = cs[:, :, :D - 1].reshape(b * T, D - 1, C) + self.pos_emb_depth.detach()[0]

    def _forward_rows(self, st, codes, conds, logits, dt, saved=None) -> None:
        """one chunk of b whole images: logits [b, T D, V] f32.  The embedding stage, the spatial Blocks over b sequences of T rows (GPT's launches),
        ln_spatial into slot 0 of the depth stream, the depth Blocks over b T sequences of D rows, ln_depth and the head.  saved (forward_backward):
        dict(spatial=[...], depth=[...]), one dict of buffers per layer as in GPT._forward_rows; a layer's input x, a, qkv, att, lse, x2, a2 and hid
        then stay there (the embedding stage and ln_spatial write the first layers' x), and the stacks' outputs go to st["xs"] (the input of
        ln_spatial) and st["xd"] (of ln_depth).  The launches and their arguments are the same: so are the bits."""
        from ... import _C
        b, T, D, C, V = codes.shape[0], self.img_num_tokens, self.depth_num_tokens, self.embed_dim, self.vocab_img_size
        Ms, M = b * T, b * T * D
        Hs, Hd = self.spatial_n_heads, self.depth_n_heads
        ops = self._operand_copies(dt)
        xs, xd = st["xs"][:Ms], st["xd"][:M]

        def bufs(stack: str, i: int, R: int, x_last, n_lse: int):
            """_block_rows' buffers of layer i of a stack over R rows (x, x_out, a, a2, qkv, att, x2, hid32, hid), then the attention's lse"""
            x2, a, qkv, att, hid32, hid = (None if st[k] is None else st[k][:R] for k in ("x2", "a", "qkv", "att", "hid32", "hid"))
            if saved is None:
                return x_last, x_last, a, a, qkv, att, x2, hid32, hid, None
            sv, nxt = saved[stack][i], saved[stack][i + 1:i + 2]
            return (sv["x"][:R], nxt[0]["x"][:R] if nxt else x_last, sv["a"][:R], sv["a2"][:R], sv["qkv"][:R], sv["att"][:R], sv["x2"][:R], hid32,
                    sv["hid"][:R], sv["lse"][:n_lse])

        xs_in = bufs("spatial", 0, Ms, xs, 0)[0] if len(self.spatial_transformer) else xs
        xd_in = bufs("depth", 0, M, xd, 0)[0] if len(self.depth_transformer) else xd
        if self.code_sum == "depth":
            _C.rq_embed_seq(conds, codes, self.tok_emb_cond.weight.detach(), self.pos_emb_cond.detach()[0, 0], self.tok_emb_code.weight.detach(),
                            self.pos_emb_code.detach()[0], self.pos_emb_depth.detach()[0], xs_in.view(b, T, C), xd_in.view(Ms, D, C))
        else:
            self._embed_channels(codes, conds, xs_in, xd_in)
        linear = _row_linear(Ms, dt)
        for i, (blk, W) in enumerate(zip(self.spatial_transformer, ops["spatial"])):
            *rows, lse = bufs("spatial", i, Ms, xs, b * Hs * T)
            _block_rows(blk, W, linear, dt, T, lambda q, o: _C.causal_attention(q, b, T, Hs, C // Hs, o, lse=lse), *rows)
        _C.ln_rows_strided(xs, self.ln_spatial.weight, self.ln_spatial.bias, xd_in, D * C, eps=self.ln_spatial.eps)
        linear = _row_linear(M, dt)
        tile = dt == torch.float32 or os.environ.get("ENH_RQ_DEPTH_ATTN") == "tile"
        for i, (blk, W) in enumerate(zip(self.depth_transformer, ops["depth"])):
            *rows, lse = bufs("depth", i, M, xd, Ms * Hd * D)
            if tile:
                attention = lambda q, o: _C.causal_attention(q, Ms, D, Hd, C // Hd, o, lse=lse)
            else:
                attention = lambda q, o: _C.short_causal_attention(q, Ms, D, Hd, C // Hd, o, lse=lse)
            _block_rows(blk, W, linear, dt, D, attention, *rows)
        _C.ln_timeshift(xd, self.ln_depth.weight, self.ln_depth.bias, st["a"][:M], D, eps=self.ln_depth.eps)
        linear(st["a"][:M], ops["head"], logits.view(M, V))

    # ---- teacher-forced loss and its gradients -----------------------------------------------------
    def saved_bytes_per_image(self) -> int:
        """bytes forward_backward keeps per image for ALL layers: T rows per spatial layer and T D rows per depth layer, each row
        GPT.saved_bytes_per_token()'s 28 C + 4 H of its stack"""
        T, D, C = self.img_num_tokens, self.depth_num_tokens, self.embed_dim
        return (len(self.spatial_transformer) * T * (28 * C + 4 * self.spatial_n_heads) +
                len(self.depth_transformer) * T * D * (28 * C + 4 * self.depth_n_heads))

    def _backward_buffers(self, b: int, dt: torch.dtype, dev) -> dict:
        """the buffers of a chunk of b images.  Row counts are rounded up to 8 (the contraction length of a weight-gradient product): Mp for the
        depth stage's b T D rows, Mps for the spatial stage's b T rows, which runs in the leading rows of the depth stage's gradient buffers
        (`spatial`: their views of Mps rows) with a gradient stream of its own (gs: the depth stream's gradient g stays for the embedding).
        Everything is zero at first so that the tail rows of an operand are finite."""
        f32, C, V, T, D = torch.float32, self.embed_dim, self.vocab_img_size, self.img_num_tokens, self.depth_num_tokens
        Hs, Hd = self.spatial_n_heads, self.depth_n_heads
        Ms, M = b * T, b * T * D
        Mps, Mp = (Ms + 7) // 8 * 8, (M + 7) // 8 * 8
        z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype, device=dev)
        layer = lambda R, n_lse: dict(x=z(R, C, dtype=f32), a=z(R, C), qkv=z(R, 3 * C), att=z(R, C), lse=z(n_lse, dtype=f32), x2=z(R, C, dtype=f32),
                                      a2=z(R, C), hid=z(R, 4 * C))
        saved = dict(spatial=[layer(Mps, b * Hs * T) for _ in self.spatial_transformer], depth=[layer(Mp, Ms * Hd * D) for _ in self.depth_transformer])
        st = dict(saved=saved, xs=z(Mps, C, dtype=f32), xd=z(Mp, C, dtype=f32), a=z(Mp, C), hid32=z(Mp, 4 * C, dtype=f32), logits=z(Mp, V, dtype=f32),
                  dlogits=z(Mp, V), g=z(Mp, C, dtype=f32), gs=z(Mps, C, dtype=f32), g2=z(Mp, C, dtype=f32), d32=z(Mp, C, dtype=f32), g16=z(Mp, C),
                  dh16=z(Mp, 4 * C), dqkv=z(Mp, 3 * C), datt=z(Mp, C), dbqkv=z(3 * C, dtype=f32), x2=None, qkv=None, att=None, hid=None)
        st["spatial"] = dict(g16=st["g16"][:Mps], dh16=st["dh16"][:Mps], dqkv=st["dqkv"][:Mps], dbqkv=st["dbqkv"])
        return st

    @torch.no_grad()
    def forward_backward(self, codes: torch.Tensor, conds: torch.Tensor, *, use_fp16: bool = True, loss_scale=1.0, accumulate: bool = False) -> torch.Tensor:
        """GPT.forward_backward's contract for the RQ prior: returns the unscaled mean cross-entropy over all B T D codes (0-dim f32 on the device:
        what forward(..., return_loss=True)[2] returns, and with the same chunking the same bits) and leaves in `p.grad` of EVERY parameter
        loss_scale x the gradient of that mean (f32, views into `flat_grad`).  loss_scale is a float or a device f32 [1] tensor; the call SETS the
        gradients, or with accumulate=True ADDS to them; rows of the token tables whose id is never fed are exactly zero when set.

        use_fp16=True runs the 16-bit operand format of ENH_PRECISION; the exact-f32 backward is not built: use_fp16=False raises.  Device tensors
        only.  The backward: the cross-entropy and the head, ln_depth, the depth Blocks last to first (`_block_rows_backward`
        over sequences of D rows, with the short-sequence attention backward of csrc/rq_backward.hip; ENH_RQ_DEPTH_ATTN=tile runs the tile kernels
        of the spatial stack at N = D instead: the A/B and the cross-check), ln_spatial through slot 0 of the depth stream's gradient
        (enh_ln_rows_strided_backward), the spatial Blocks last to first over sequences of T rows, the embedding (enh_rq_embed_seq_backward).
        Batches run in chunks of whole images sized so that the saved activations stay under `backward_saved_cap` bytes
        (saved_bytes_per_image()); weight gradients accumulate across the chunks in a fixed order, so two runs give the same bits.

        code_sum="channels" builds the embedding tables' gradients with torch ops (the reverse cumsum along the channels, index_add_): its
        tok_emb_code.grad is then NOT bit-reproducible from run to run (index_add_ uses atomics).  Every launch behind the embedding is the
        default mode's."""
        return self._teacher_forced_backward("RQTransformer.forward_backward", codes, conds, use_fp16, loss_scale, accumulate,
                                             self.saved_bytes_per_image())

    def _embed_channels_backward(self, codes, conds, gs, gd, accumulate: bool) -> None:
        """code_sum="channels": the backward of _embed_channels with torch ops on the device"""
        b, T, D = codes.shape
        C = self.embed_dim
        gs, gd = gs.view(b, T, C), gd.view(b, T, D, C)
        gcs = torch.zeros(b, T, D, C, dtype=torch.float32, device=gs.device)
        gcs[:, :, :D - 1] = gd[:, :, 1:]
        gcs[:, :T - 1, D - 1] += gs[:, 1:]
        gemb = gcs.flip(-1).cumsum(-1).flip(-1)       # the gradient of cumsum along the channels
        grads = (self.tok_emb_code.weight.grad, self.tok_emb_cond.weight.grad, self.pos_emb_code.grad, self.pos_emb_depth.grad, self.pos_emb_cond.grad)
        if not accumulate:
            for t in grads:
                t.zero_()
        grads[0].index_add_(0, codes.reshape(-1), gemb.view(-1, C))
        grads[1].index_add_(0, conds, gs[:, 0])
        grads[2][0, :T - 1] += gs[:, 1:].sum(0)
        grads[3][0] += gd[:, :, 1:].sum((0, 1))
        grads[4][0, 0] += gs[:, 0].sum(0)

    def _backward_rows(self, st, codes, conds, nll, dt, gscale: float, accumulate: bool, gscale_dev=None) -> None:
        """one chunk: the saving forward, then the backward of DESIGN.md §3.10, setting (accumulate=False) or adding to every parameter's gradient"""
        from ... import _C
        b, T, D, C, V = codes.shape[0], self.img_num_tokens, self.depth_num_tokens, self.embed_dim, self.vocab_img_size
        Hs, Hd = self.spatial_n_heads, self.depth_n_heads
        Ms, M = b * T, b * T * D
        Mps, Mp = (Ms + 7) // 8 * 8, (M + 7) // 8 * 8
        ops = self._operand_copies(dt)
        saved = st["saved"]
        for k in ("dlogits", "g16", "dh16", "dqkv"):      # rows M .. Mp - 1 of the gradient operands may hold a longer chunk's rows
            st[k][M:Mp].zero_()
        logits = st["logits"][:M]
        self._forward_rows(st, codes, conds, logits.view(b, T * D, V), dt, saved=saved)
        # the head, ln_depth and the depth Blocks: M rows, sequences of D
        dlogits, g, g2, d32, g16, dh16, dqkv, datt, hid32 = (st[k][:M] for k in ("dlogits", "g", "g2", "d32", "g16", "dh16", "dqkv", "datt", "hid32"))
        wgrad, dgrad = _grad_linears(M, Mp, accumulate)
        if gscale_dev is None:
            _C.cross_entropy_backward(logits, codes.reshape(-1), nll.view(-1), dlogits, gscale)
        else:
            _C.cross_entropy_backward(logits, codes.reshape(-1), nll.view(-1), dlogits, gscale, gscale_dev=gscale_dev)
        wgrad(st["dlogits"], st["a"], self.head.weight.grad, V, C)
        dgrad(dlogits, ops["head"], d32)
        ln = self.ln_depth
        _C.ln_timeshift_backward(d32, st["xd"][:M], ln.weight, D, g, ln.weight.grad, ln.bias.grad, dx16=g16, eps=ln.eps, accumulate=accumulate)
        if os.environ.get("ENH_RQ_DEPTH_ATTN") == "tile":
            def depth_attention_backward(sv, datt_, dqkv_):
                _C.causal_attention_backward(sv["qkv"][:M], sv["att"][:M], datt_, sv["lse"][:Ms * Hd * D], Ms, D, Hd, C // Hd, dqkv_)
        else:
            def depth_attention_backward(sv, datt_, dqkv_):
                _C.short_causal_attention_backward(sv["qkv"][:M], sv["att"][:M], datt_, sv["lse"][:Ms * Hd * D], Ms, D, Hd, C // Hd, dqkv_)
        for i in range(len(self.depth_transformer) - 1, -1, -1):
            _block_rows_backward(self.depth_transformer[i], ops["depth"][i], wgrad, dgrad, accumulate, D, depth_attention_backward, saved["depth"][i], st,
                                 g, g2, d32, g16, dh16, dqkv, datt, hid32)
        # ln_spatial through slot 0 of the depth stream's gradient, then the spatial Blocks: Ms rows, sequences of T, in the leading rows of the
        # same buffers.  The weight-gradient products now contract over Mps rows: the depth stage left its rows Ms .. Mps - 1 there.
        for k in ("g16", "dh16", "dqkv"):
            st[k][Ms:Mps].zero_()
        gs, g2, d32, g16, dh16, dqkv, datt, hid32 = (st[k][:Ms] for k in ("gs", "g2", "d32", "g16", "dh16", "dqkv", "datt", "hid32"))
        ln = self.ln_spatial
        _C.ln_rows_strided_backward(st["g"], D * C, st["xs"][:Ms], ln.weight, gs, ln.weight.grad, ln.bias.grad, dx16=g16, eps=ln.eps, accumulate=accumulate)
        wgrad, dgrad = _grad_linears(Ms, Mps, accumulate)

        def spatial_attention_backward(sv, datt_, dqkv_):
            _C.causal_attention_backward(sv["qkv"][:Ms], sv["att"][:Ms], datt_, sv["lse"][:b * Hs * T], b, T, Hs, C // Hs, dqkv_)

        for i in range(len(self.spatial_transformer) - 1, -1, -1):
            _block_rows_backward(self.spatial_transformer[i], ops["spatial"][i], wgrad, dgrad, accumulate, T, spatial_attention_backward,
                                 saved["spatial"][i], st["spatial"], gs, g2, d32, g16, dh16, dqkv, datt, hid32)
        if self.code_sum == "depth":
            _C.rq_embed_seq_backward(gs.view(b, T, C), g.view(Ms, D, C), conds, codes, self.tok_emb_cond.weight.grad, self.pos_emb_cond.grad.view(-1),
                                     self.tok_emb_code.weight.grad, self.pos_emb_code.grad.view(-1, C), self.pos_emb_depth.grad.view(-1, C), accumulate)
        else:
            self._embed_channels_backward(codes, conds, gs, g, accumulate)

    # ---- sampling -------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, conds: torch.Tensor, top_k: Optional[float] = None, top_p: Optional[float] = None, softmax_temperature: float = 1.0,
               use_fp16: bool = True, *, seed: Optional[int] = None, forced_codes: Optional[torch.Tensor] = None, return_logits: bool = True,
               call: int = 0, row_offset: int = 0, slot0_ln: str = "once", graph: Optional[bool] = None,
               weights: Optional[str] = None, cache: Optional[str] = None,
               prefix_codes: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """reference layers.py:397-547 (sample, sample_spatial_step, sample_depth_step) with one condition token: returns (logits [B T, D, V] f32
        after the temperature and the top-k mask, codes [B, T, D] int64).  GPT.sample's contract: the loop is restated per
        step, one row per batch element.  Per position t the spatial Blocks run under a cache of T slots on the input row
        tok_emb_cond[cond] + pos_emb_cond[0] (t == 0) or sum_j tok_emb_code[code[b, t - 1, j]] + pos_emb_code[t - 1], and ln_spatial gives the hidden
        row; then D depth steps under a cache of D slots whose slot d is overwritten at every position: the input row is the hidden row (d == 0)
        or sum_{j < d} tok_emb_code[code[b, t, j]] + pos_emb_depth[d - 1]; ln_depth, the head, the filter and the draw of code[b, t, d].

        Two contracts.  Under the cache every Block of BOTH transformers sees one row, where `time_shift(x)` is all zeros and the mix is
        ln1(x) * time_mix.  That is NOT what the teacher-forced `forward` computes on the same codes (there the shifted term is the previous row's
        ln1): the sampler's logits differ from forward's, as GPT's do, and each has its golden (tests/golden/rq_sample_<case>.npz, rq_fwd_<case>.npz).

        The slot-0 quirk.  The reference's sample_depth_step applies ln_depth inside its `codes is None` branch and again in the common line behind
        it: depth slot 0 is normalised twice, slots d >= 1 once; the teacher-forced forward (so training) normalises every slot once.  Keyword
        `slot0_ln` selects "once" (default: what the trained model computes) or "twice" (the reference's sampler line for line: a parity instrument
        whose golden is the reference's own sample loop; one more enh_row_ln_scale launch at d == 0, nothing else differs).

        The sampler sums the code embeddings over depth: a module built with code_sum="channels" is refused (the reference's sampler has no such form).

        use_fp16=True runs the 16-bit operand format of ENH_PRECISION with f32 accumulation; False the exact mode (f32 caches, enh_skinny_gemm_f32,
        f32 row kernels).  The draw is GPT.sample's: one uniform per (seed, call, step = t D + d, row_offset + row); seed=None draws one from torch's
        generator.  forced_codes [B, T, D] are fed forward instead of the draws (codes are still drawn and returned).  Batches above 64 rows run in
        chunks of 64 rows; a chunk equals a separate call with its `row_offset`.  Nothing in the loop reads a device value on the host.  The depth
        transformer's attention is enh_short_decode_attention; ENH_RQ_DEPTH_DECODE=cache runs enh_decode_attention at Tmax = D instead (A/B only).
        Device tensors only.  Side effect: a module whose parameters are not on the device of `conds` is moved there.

        graph=True replays every position after the first from ONE captured HIP graph per chunk: the spatial step, the D depth
        steps and their draws, with the spatial attention, the input rows and the draws in their cursor forms (the depth attention keeps its
        constant slot d); the same bits as the loop.  None reads ENH_GRAPHS == "1", False is the loop.  Captured per call, nothing is cached between
        calls; while per-kernel timing is on (_C.TIMER) the loop runs.

        weights="fp8" is GPT.sample's: every Linear of every Block of BOTH stacks as its MXFP8 operand through enh_skinny_gemm_w8, the head in the
        16-bit format; weights="fp6" / "fp4" the same with MXFP6 / MXFP4 operands through enh_skinny_gemm_w6 / enh_skinny_gemm_w4; None reads
        ENH_SAMPLE_WEIGHTS (default "h16"); all three need use_fp16=True.

        cache="fp8" is GPT.sample's for the SPATIAL stack: its k / v caches are MXFP8 codes and scales behind enh_decode_attention_kv8 (DESIGN.md
        §3.14); the depth caches (D <= 8 slots, enh_short_decode_attention) stay 16-bit.  None reads ENH_SAMPLE_CACHE (default "h16"); it needs
        use_fp16=True.

        prefix_codes [B, P, D] (anything with B rows and a last axis of D that reshapes to it, e.g. [B, h', w, D]; 0 <= P < T, ids in [0, V), else
        a ValueError) is GPT.sample's for the SPATIAL stack: positions < P are given with all their D codes, one batched prefill
        per chunk puts the spatial rows of the condition and of positions 0 .. P - 2 (the spatial stream of enh_rq_embed_seq) into slots
        0 .. P - 1 of the spatial caches under the sampler's model, and the loop runs positions P .. T - 1 unchanged under their step numbers
        t D + d.  The depth stack needs no prefix: its caches are rewritten at every position.  codes[:, :P] is the prefix, the logits of positions
        < P are NOT computed and are returned as NaN; with forced_codes its first P positions must equal the prefix."""
        prefix_codes = self._check_prefix(prefix_codes, conds.shape[0] if torch.is_tensor(conds) else 0, "RQTransformer.sample")
        if not (torch.is_tensor(conds) and conds.is_cuda):
            raise NotImplementedError("RQTransformer.sample: sampling runs on a ROCm device only: conds must be a device tensor (the spatial / depth "
                                      "decode loop is HIP kernels: there is no CPU path)")
        if slot0_ln not in SLOT0_LNS:
            raise ValueError(f"RQTransformer.sample: slot0_ln must be one of {SLOT0_LNS}, got {slot0_ln!r}")
        if self.code_sum != "depth":
            raise ValueError(f"RQTransformer.sample: this module was built with code_sum={self.code_sum!r}, but the sampler sums the code embeddings over "
                             "depth (the reference's sample_spatial_step / sample_depth_step have no other form): build it with code_sum=\"depth\"")
        depth_decode = os.environ.get("ENH_RQ_DEPTH_DECODE", "short")
        if depth_decode not in ("short", "cache"):
            raise ValueError(f"RQTransformer.sample: ENH_RQ_DEPTH_DECODE must be 'short' or 'cache', got {depth_decode!r}")
        dev = conds.device
        conds = self._on_device_conds(conds, conds.shape[0], "RQTransformer.sample")
        B, T, D, V = conds.shape[0], self.img_num_tokens, self.depth_num_tokens, self.vocab_img_size
        if top_k is not None and not 1 <= int(top_k) <= V:
            raise ValueError(f"RQTransformer.sample: top_k must be in [1, {V}], got {top_k}")
        if forced_codes is not None:
            if forced_codes.numel() != B * T * D:
                raise ValueError(f"RQTransformer.sample: forced_codes must be [B = {B}, img_num_tokens = {T}, depth_num_tokens = {D}], got "
                                 f"{tuple(forced_codes.shape)}")
            forced_codes = forced_codes.to(device=dev, dtype=torch.int64).reshape(B, T, D).contiguous()
            if int(forced_codes.min()) < 0 or int(forced_codes.max()) >= V:
                raise ValueError(f"RQTransformer.sample: forced_codes outside [0, {V})")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        dt = self._operand_dtype(use_fp16, "RQTransformer.sample")
        weights = self._sample_weights(weights, use_fp16, "RQTransformer.sample")
        cache = self._sample_cache(cache, use_fp16, "RQTransformer.sample")
        codes = torch.empty(B, T, D, dtype=torch.int64, device=dev)
        logits = torch.empty(B * T, D, V, dtype=torch.float32, device=dev) if return_logits else None
        if prefix_codes is not None:
            prefix_codes = self._place_prefix(prefix_codes, forced_codes, codes, logits, "RQTransformer.sample")
        if self._use_graph(graph):
            self._sample_graphed(B, dev, lambda b: self._decode_state(b, dt, dev, weights, cache), lambda st, s, e, positions: self._sample_rows_graphed(
                st, positions, conds[s:e], codes[s:e], None if logits is None else logits.view(B, T, D, V)[s:e],
                None if forced_codes is None else forced_codes[s:e], top_k, top_p, float(softmax_temperature), seed, call, row_offset + s,
                slot0_ln == "twice", depth_decode == "cache", None if prefix_codes is None else prefix_codes[s:e]))
            return logits, codes
        for s in range(0, B, MAX_BATCH):
            e = min(s + MAX_BATCH, B)
            self._sample_rows(conds[s:e], codes[s:e], None if logits is None else logits.view(B, T, D, V)[s:e],
                              None if forced_codes is None else forced_codes[s:e], dt, top_k, top_p, float(softmax_temperature), seed, call,
                              row_offset + s, slot0_ln == "twice", depth_decode == "cache", weights, cache,
                              None if prefix_codes is None else prefix_codes[s:e])
        return logits, codes

    def _decode_state(self, b: int, dt: torch.dtype, dev, weights: str = "h16", cache: str = "h16") -> dict:
        """the buffers of one chunk of b <= 64 rows: the spatial and the depth residual stream, activations, the step's logits, every spatial
        layer's k / v cache [b, Hs, T, C / Hs] in the form of `cache` (prior.py `_kv_caches`) and every depth layer's [b, Hd, D, C / Hd], always
        16-bit; ops: the operands of `weights` (prior.py `_sample_operands`)"""
        f32, C, T, D = torch.float32, self.embed_dim, self.img_num_tokens, self.depth_num_tokens
        Hs, Hd = self.spatial_n_heads, self.depth_n_heads
        e = lambda *shape, dtype=dt: torch.empty(*shape, dtype=dtype, device=dev)
        return dict(dt=dt, b=b, xs=e(b, C, dtype=f32), xd=e(b, C, dtype=f32), x2=e(b, C, dtype=f32), a=e(b, C), qkv=e(b, 3 * C), att=e(b, C),
                    hid=e(b, 4 * C), logits=e(b, self.vocab_img_size, dtype=f32),
                    spatial=_kv_caches(len(self.spatial_transformer), b, Hs, T, C // Hs, dt, dev, cache),
                    depth=[(e(b, Hd, D, C // Hd), e(b, Hd, D, C // Hd)) for _ in self.depth_transformer], ops=self._sample_operands(dt, weights))

    def _sample_rows(self, conds, codes, logits, forced, dt, top_k, top_p, temperature, seed, call, row0, ln_twice: bool, depth_cache: bool,
                     weights: str = "h16", cache: str = "h16", prefix=None):
        """one chunk of b <= 64 rows: codes [b, T, D] (a view the draws are written into), logits [b, T, D, V] (a view) or None; prefix [b, P, D]
        or None: the given positions, which `_prefill` puts into the spatial caches"""
        from ... import _C
        T, D = self.img_num_tokens, self.depth_num_tokens
        st = self._decode_state(conds.shape[0], dt, conds.device, weights, cache)
        feed = codes if forced is None else forced
        P = 0 if prefix is None else prefix.shape[1]
        if P:
            self._prefill(st, conds, prefix)
        for t in range(P, T):
            self._spatial_step(st, t, conds if t == 0 else feed[:, t - 1, :])
            for d in range(D):
                self._depth_step(st, t, d, None if d == 0 else feed[:, t, :d], ln_twice, depth_cache)
                _C.sample_logits(st["logits"], codes[:, t, d], temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, call=call, step=t * D + d,
                                 row0=row0, logits_out=None if logits is None else logits[:, t, d, :])

    def _sample_rows_graphed(self, st, positions, conds, codes, logits, forced, top_k, top_p, temperature, seed, call, row0, ln_twice: bool,
                             depth_cache: bool, prefix=None):
        """_sample_rows for Prior._sample_graphed: position 0 (under a prefix of P positions the prefill and position P) as there, every later
        one the same launches with the spatial attention, the input rows and the draws in their cursor forms"""
        from ... import _C
        D = self.depth_num_tokens
        feed = codes if forced is None else forced
        draw = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, call=call, row0=row0)
        P = 0 if prefix is None else prefix.shape[1]

        def first():
            if P:
                self._prefill(st, conds, prefix)
            self._spatial_step(st, P, feed[:, P - 1, :] if P else conds)
            for d in range(D):
                self._depth_step(st, P, d, None if d == 0 else feed[:, P, :d], ln_twice, depth_cache)
                _C.sample_logits(st["logits"], codes[:, P, d], step=P * D + d, logits_out=None if logits is None else logits[:, P, d, :], **draw)

        def later(cursor):
            self._spatial_step(st, None, feed, cursor=cursor)
            for d in range(D):
                self._depth_step(st, None, d, None if d == 0 else feed, ln_twice, depth_cache, cursor=cursor)
                _C.sample_logits_at(st["logits"], codes, cursor, step_mul=D, step_add=d, logits_out=logits, **draw)

        positions(self.img_num_tokens, first, later, P)

    def _prefill(self, st: dict, conds, prefix) -> None:
        """the given positions prefix [b, P, D] of a chunk put into slots 0 .. P - 1 of every spatial layer's cache of `st` (prior.py
        `_prefill_stack`): the spatial rows s = 0 .. P - 1 (the condition, then the depth sums of positions 0 .. P - 2) are the spatial stream of
        enh_rq_embed_seq at T = P, enh_rq_embed_step's bits; the depth stream it also writes is discarded (the depth caches are rewritten at every
        position)"""
        from ... import _C
        (b, P, D), C = prefix.shape, self.embed_dim
        pf = _prefill_buffers(b, P, C, st["dt"], prefix.device, self.forward_hidden_cap)
        unused = torch.empty(pf["g"] * P, D, C, dtype=torch.float32, device=prefix.device)
        for b0 in range(0, b, pf["g"]):
            n = min(pf["g"], b - b0)
            _C.rq_embed_seq(conds[b0:b0 + n], prefix[b0:b0 + n], self.tok_emb_cond.weight.detach(), self.pos_emb_cond.detach()[0, 0],
                            self.tok_emb_code.weight.detach(), self.pos_emb_code.detach()[0], self.pos_emb_depth.detach()[0],
                            pf["x"][:n * P].view(n, P, C), unused[:n * P])
            _prefill_stack(self.spatial_transformer, st["ops"]["spatial"], st["spatial"], b0, n, P, self.spatial_n_heads, st["dt"], pf)

    def _spatial_step(self, st: dict, t: Optional[int], ids: torch.Tensor, cursor: Optional[torch.Tensor] = None) -> None:
        """position t of the spatial transformer, one row per batch element: ids (int64, on the device: the condition [b] at t == 0, else the D
        codes [b, D] of position t - 1) -> ln_spatial of the stack's output in st["xd"] [b, C] f32, the input row of depth slot 0.
        The cursor form (cursor: device int32 [1], t is None): the position t >= 1 the cursor holds; ids is then the whole [b, T, D] tensor of the
        codes that are fed forward, whose row t - 1 the embedding reads on the device."""
        from ... import _C
        x, x2, a, qkv, att, hid = st["xs"], st["x2"], st["a"], st["qkv"], st["att"], st["hid"]
        linear = _step_linear(st["dt"])
        if cursor is not None:
            C, D = self.embed_dim, self.depth_num_tokens
            _C.embed_step_at(self.tok_emb_code.weight.detach(), ids, D, D, -D, self.pos_emb_code.detach()[0], C, -C, cursor, 1, self.img_num_tokens, x)
        else:
            if t == 0:
                _C.gpt_embed(self.tok_emb_cond.weight.detach(), ids, self.pos_emb_cond.detach()[0, 0], x)
            else:
                _C.rq_embed_step(self.tok_emb_code.weight.detach(), ids, self.pos_emb_code.detach()[0, t - 1], x)
        attend = _step_attention(t, cursor)
        for blk, W, kv in zip(self.spatial_transformer, st["ops"]["spatial"], st["spatial"]):
            _block_step(blk, W, linear, lambda q, o: attend(q, kv, o), x, x2, a, qkv, att, hid)
        _C.row_ln_scale(x, self.ln_spatial.weight, self.ln_spatial.bias, st["xd"], eps=self.ln_spatial.eps)

    def _depth_step(self, st: dict, t: Optional[int], d: int, ids: Optional[torch.Tensor], ln_twice: bool, depth_cache: bool,
                    cursor: Optional[torch.Tensor] = None) -> None:
        """slot d of position t of the depth transformer: the input row is st["xd"] as _spatial_step left it (d == 0), else built from ids
        (int64 [b, d] on the device: codes 0 .. d - 1 of the position) -> st["logits"] [b, V] f32.  Slot d of the depth caches is overwritten
        and slots > d are never read: the caches need no reset between positions.  The cursor form (cursor: device int32 [1], t is None): ids is
        the whole [b, T, D] tensor of the codes that are fed forward, whose row t the embedding reads on the device; the attention's slot d is a
        constant of the launch either way."""
        from ... import _C
        x, x2, a, qkv, att, hid = st["xd"], st["x2"], st["a"], st["qkv"], st["att"], st["hid"]
        linear = _step_linear(st["dt"])
        attend = _C.decode_attention if depth_cache else _C.short_decode_attention
        if d > 0 and cursor is not None:
            D = self.depth_num_tokens
            _C.embed_step_at(self.tok_emb_code.weight.detach(), ids, d, D, 0, self.pos_emb_depth.detach()[0, d - 1], 0, 0, cursor, 0, self.img_num_tokens, x)
        elif d > 0:
            _C.rq_embed_step(self.tok_emb_code.weight.detach(), ids, self.pos_emb_depth.detach()[0, d - 1], x)
        for blk, W, (kc, vc) in zip(self.depth_transformer, st["ops"]["depth"], st["depth"]):
            _block_step(blk, W, linear, lambda q, o: attend(q, kc, vc, d, o), x, x2, a, qkv, att, hid)
        ln = self.ln_depth
        if d == 0 and ln_twice:      # the reference's sampler: ln_depth in the `codes is None` branch, then the common line
            _C.row_ln_scale(x, ln.weight, ln.bias, x2, eps=ln.eps)
            x = x2
        _C.row_ln_scale(x, ln.weight, ln.bias, a, eps=ln.eps)
        linear(a, st["ops"]["head"], st["logits"])
