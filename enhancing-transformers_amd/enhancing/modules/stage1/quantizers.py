"""Vector / residual quantizer of the stage-1 tokenizer with the reference's constructor and
``forward(z) -> (z_q, loss, indices)`` contract (reference enhancing/modules/stage1/quantizers.py:19-92).

The arithmetic — l2-normalise, pairwise distance against the whole codebook, argmin, gather, commit/codebook
loss, the shared-codebook residual loop and the straight-through estimator — is ONE fused gfx950 kernel
(``enh_vq_forward``) plus its hand-derived backward (``enh_vq_backward``), wrapped in a
``torch.autograd.Function`` so the module composes with ordinary autograd.  "RQ-VAE" is
``use_residual=True, num_quantizers=D`` on this same class, exactly as in the reference."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from ... import _C


class _QuantizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, codebook, beta, depth, use_residual, use_norm):
        shp = z.shape
        z2 = z.detach().reshape(-1, shp[-1]).contiguous()
        cb = codebook.detach().contiguous()
        zq, _, idx, loss = _C.vq_forward(z2, cb, beta, depth, use_norm, want_bf16=False)
        ctx.save_for_backward(z2, cb, idx)
        ctx.cfg = (beta, depth, use_residual, use_norm, shp)
        idx_out = idx.view(*shp[:-1], depth) if use_residual else idx.view(*shp[:-1])
        ctx.mark_non_differentiable(idx_out)
        return zq.view(shp), loss.view(()), idx_out

    @staticmethod
    def backward(ctx, g_zq, g_loss, _g_idx):
        z2, cb, idx = ctx.saved_tensors
        beta, depth, use_residual, use_norm, shp = ctx.cfg
        if g_zq is None:
            g_zq = torch.zeros(shp, dtype=torch.float32, device=z2.device)
        g_out = g_zq.reshape(-1, shp[-1]).contiguous().float()
        d_cb = torch.zeros_like(cb)
        g_loss_dev = None if g_loss is None else g_loss.reshape(1).float().contiguous()
        dz, _ = _C.vq_backward(z2, cb, idx, g_out, 1.0 if g_loss is not None else 0.0, g_loss_dev, beta, depth, use_residual,
                               use_norm, d_cb, want_bf16=False)
        return dz.view(shp), d_cb, None, None, None, None


class _LookupFn(torch.autograd.Function):
    """z_qnorm = norm(E[idx]) through enh_vq_lookup; backward = the l2-normalise Jacobian scattered into the codebook gradient."""

    @staticmethod
    def forward(ctx, codebook, idx, use_norm):
        cb = codebook.detach().contiguous()
        flat = idx.reshape(-1, 1).contiguous()
        out, _ = _C.vq_lookup(cb, flat, use_norm, want_bf16=False)
        ctx.save_for_backward(cb, flat)
        ctx.use_norm = use_norm
        ctx.mark_non_differentiable(idx)
        return out.view(*idx.shape, cb.shape[1])

    @staticmethod
    def backward(ctx, g):
        cb, flat = ctx.saved_tensors
        e = cb[flat.view(-1)]
        g = g.reshape(-1, cb.shape[1]).float()
        if ctx.use_norm:
            nrm = e.norm(dim=-1, keepdim=True).clamp_min(1e-12)
            en = e / nrm
            g = (g - en * (en * g).sum(-1, keepdim=True)) / nrm
        d_cb = torch.zeros_like(cb).index_add_(0, flat.view(-1), g)
        return d_cb, None, None


class BaseQuantizer(nn.Module):
    def __init__(self, embed_dim: int, n_embed: int, straight_through: bool = True, use_norm: bool = True,
                 use_residual: bool = False, num_quantizers: Optional[int] = None) -> None:
        super().__init__()
        self.straight_through = straight_through
        self.use_norm = use_norm
        self.norm = (lambda x: torch.nn.functional.normalize(x, dim=-1)) if use_norm else (lambda x: x)
        self.use_residual = use_residual
        self.num_quantizers = num_quantizers
        self.embed_dim = embed_dim
        self.n_embed = n_embed
        self.embedding = nn.Embedding(self.n_embed, self.embed_dim)
        self.embedding.weight.data.normal_()  # quantizers.py:33


class VectorQuantizer(BaseQuantizer):
    """reference quantizers.py:66-92.  embed_dim: any multiple of 8 in [8, 256] (the fused kernel runs it on its smallest compiled
    width of 32, 64, 128 or 256 that fits, zero-padded; every reference config uses 32)."""

    def __init__(self, embed_dim: int, n_embed: int, beta: float = 0.25, use_norm: bool = True,
                 use_residual: bool = False, num_quantizers: Optional[int] = None, **kwargs) -> None:
        if not (isinstance(embed_dim, int) and 8 <= embed_dim <= 256 and embed_dim % 8 == 0):
            raise ValueError(f"the fused gfx950 quantizer kernel requires embed_dim % 8 == 0 and 8 <= embed_dim <= 256, got {embed_dim!r}")
        super().__init__(embed_dim, n_embed, True, use_norm, use_residual, num_quantizers)
        if use_residual and not num_quantizers:
            raise ValueError("use_residual=True needs num_quantizers")
        if use_residual and int(num_quantizers) > 8:
            raise ValueError("the fused gfx950 residual quantizer keeps at most 8 depths in registers (enh_vq_backward): num_quantizers <= 8")
        self.beta = beta

    @property
    def depth(self) -> int:
        return int(self.num_quantizers) if self.use_residual else 1

    def forward(self, z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return _QuantizeFn.apply(z, self.embedding.weight, float(self.beta), self.depth, bool(self.use_residual), bool(self.use_norm))

    def quantize(self, z: torch.Tensor):
        """single-level quantize (reference quantizers.py:74-92): (z_qnorm, loss, indices) where z_qnorm = norm(embedding(indices)) — the
        NORMALISED CODE itself, not the straight-through value forward() returns (quantizers.py:85-92).  Indices and loss come from the fused
        kernel; z_qnorm from the lookup kernel, differentiable with respect to the codebook like the reference's (normalise Jacobian +
        scatter-add, evaluated with torch ops in backward: this entry point is API surface, not the training hot path)."""
        _, loss, idx = _QuantizeFn.apply(z, self.embedding.weight, float(self.beta), 1, False, bool(self.use_norm))
        zqn = _LookupFn.apply(self.embedding.weight, idx, bool(self.use_norm))
        return zqn.view(z.shape), loss, idx

    def lookup(self, code: torch.Tensor) -> torch.Tensor:
        """decode_codes front half (reference vitvqgan.py:82-87): n(E[code]) summed over the depth axis."""
        depth = self.depth
        shp = code.shape[:-1] if self.use_residual else code.shape
        out, _ = _C.vq_lookup(self.embedding.weight.detach().contiguous(), code.reshape(-1, depth).contiguous(), self.use_norm,
                              want_bf16=False)
        return out.view(*shp, self.embed_dim)


class _GumbelFn(torch.autograd.Function):
    """one level of the fused Gumbel-softmax quantizer (enh_gumbel_forward / enh_gumbel_backward): no [M,K] tensor, the noise is a function of
    (seed, call, token, code) that the backward regenerates."""

    @staticmethod
    def forward(ctx, z, codebook, tau, hard, use_norm, seed, call):
        shp = z.shape
        z2 = z.detach().reshape(-1, shp[-1]).contiguous()
        cb = codebook.detach().contiguous()
        zq, zq_soft, idx, loss, stats = _C.gumbel_forward(z2, cb, tau, hard, use_norm, seed, call)
        ctx.save_for_backward(z2, cb, zq_soft, stats, idx)
        ctx.cfg = (tau, hard, use_norm, seed, call, shp)
        idx_out = idx.view(*shp[:-1])
        ctx.mark_non_differentiable(idx_out)
        return zq.view(shp), loss.view(()), idx_out

    @staticmethod
    def backward(ctx, g_zq, g_loss, _g_idx):
        z2, cb, zq_soft, stats, idx = ctx.saved_tensors
        tau, hard, use_norm, seed, call, shp = ctx.cfg
        if g_zq is None:
            g_zq = torch.zeros(shp, dtype=torch.float32, device=z2.device)
        g_out = g_zq.reshape(-1, shp[-1]).contiguous().float()
        d_cb = torch.zeros_like(cb)
        g_loss_dev = None if g_loss is None else g_loss.reshape(1).float().contiguous()
        dz = _C.gumbel_backward(z2, cb, zq_soft, stats, g_out, 1.0 if g_loss is not None else 0.0, g_loss_dev, tau, hard, idx, use_norm, seed, call,
                                d_cb)
        return dz.view(shp), d_cb, None, None, None, None, None


class GumbelQuantizer(BaseQuantizer):
    """Gumbel-softmax relaxation of the codebook lookup (reference quantizers.py:95-126; used by ViTVQGumbel).  Semantics restated from the reference:
      logits_k = -(|zn|^2 + |en_k|^2 - 2 zn.en_k)      soft = gumbel_softmax(logits, tau, hard = not training)      z_q = soft @ en
      loss = mean_tokens sum_k p_k (log p_k + log K), p = softmax(logits)  (KL to the uniform prior)            indices = argmax soft
    and BaseQuantizer.forward's residual loop without the straight-through estimator (quantizers.py:38-63, straight_through = False).

    fused=False (the default) is plain PyTorch on the device tensors, differentiated by torch autograd between the two halves of the HIP schedule
    (Stage1Engine.differentiable_encode / _decode): it draws its noise from torch's generator exactly as the reference does, and builds the [M, K]
    logits, noise and both softmaxes in memory.
    fused=True (embed_dim a multiple of 8 up to 32, device tensors only) runs each level as one fused gfx950 kernel and its hand-derived backward
    (enh_gumbel_forward / enh_gumbel_backward, csrc/gumbel.hip): no [M, K] tensor exists, and the noise is a counter-based function of
    (seed, call, token, code) — include/enh_hip.h states its layout — which the backward regenerates.  `call` is a host counter, one per level per
    forward (``noise_call`` is the next one); ``fused_noise(call, M)`` returns the [M, K] noise of a call.  seed=None derives the seed from
    torch.initial_seed() and the process's rank at the first fused call, drawing from no generator: construction consumes what the reference's
    does, and the ranks of a data-parallel run get different noise.  The residual loop stays a host loop over the levels.
    Not kept in the state dict (its keys are the reference's): ``noise_call`` and a derived seed are Python attributes, so a run resumed from a
    checkpoint starts again at call 0 with a seed derived from the new process's torch.initial_seed() — set ``noise_call`` (and pass ``seed``) after
    loading to continue a noise sequence instead of replaying it.  The fused ``lookup`` goes through enh_vq_lookup on the detached codebook (an
    inference entry: no gradient reaches the codebook through it), while the torch path's lookup stays differentiable."""

    def __init__(self, embed_dim: int, n_embed: int, temp_init: float = 1.0, use_norm: bool = True, use_residual: bool = False,
                 num_quantizers: Optional[int] = None, fused: bool = False, seed: Optional[int] = None, **kwargs) -> None:
        if fused and not (isinstance(embed_dim, int) and 8 <= embed_dim <= 32 and embed_dim % 8 == 0):
            raise ValueError(f"the fused gfx950 Gumbel quantizer kernel requires embed_dim % 8 == 0 and 8 <= embed_dim <= 32, got {embed_dim!r}")
        super().__init__(embed_dim, n_embed, False, use_norm, use_residual, num_quantizers)
        if use_residual and not num_quantizers:
            raise ValueError("use_residual=True needs num_quantizers")
        self.temperature = temp_init
        self.fused = bool(fused)
        self.seed = None if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self.noise_call = 0      # the noise call index the next fused level will use

    @property
    def depth(self) -> int:
        return int(self.num_quantizers) if self.use_residual else 1

    def noise_seed(self) -> int:
        """the 64-bit key of the fused path's noise: the constructor's seed, or (once, at first use) torch.initial_seed() offset per rank"""
        if self.seed is None:
            import os
            dist = torch.distributed
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else int(os.environ.get("RANK", "0"))
            self.seed = (torch.initial_seed() + 0x9E3779B97F4A7C15 * rank) & 0xFFFFFFFFFFFFFFFF
        return self.seed

    def fused_noise(self, call: int, M: int) -> torch.Tensor:
        """[M, n_embed] f32: the noise the fused path adds to the logits of token rows 0..M-1 at noise call `call` (enh_gumbel_noise)"""
        return _C.gumbel_noise(self.noise_seed(), call, M, self.n_embed, self.embedding.weight.device)

    def quantize(self, z: torch.Tensor, temp: Optional[float] = None):
        import math
        tau = self.temperature if temp is None else temp
        if self.fused:
            if not z.is_cuda:
                raise RuntimeError(f"GumbelQuantizer(fused=True) runs on a ROCm device only (got a {z.device} tensor): there is no CPU form of the "
                                   "fused kernel; construct with fused=False for the torch path")
            call = self.noise_call
            self.noise_call = (call + 1) & 0xFFFFFFFF
            return _GumbelFn.apply(z.float(), self.embedding.weight, float(tau), not self.training, bool(self.use_norm), self.noise_seed(), call)
        zn = self.norm(z.reshape(-1, self.embed_dim))
        en = self.norm(self.embedding.weight)
        logits = (2.0 * zn @ en.t() - zn.pow(2).sum(1, keepdim=True) - en.pow(2).sum(1)).view(*z.shape[:-1], self.n_embed)
        soft = torch.nn.functional.gumbel_softmax(logits, tau=tau, dim=-1, hard=not self.training)
        z_q = soft @ en
        logp = torch.log_softmax(logits, dim=-1)
        loss = (logp.exp() * (logp + math.log(self.n_embed))).sum(-1).mean()
        return z_q, loss, soft.argmax(dim=-1)

    def forward(self, z: torch.Tensor):
        if not self.use_residual:
            return self.quantize(z)
        z_q, residual = torch.zeros_like(z), z.detach().clone()
        losses, idxs = [], []
        for _ in range(int(self.num_quantizers)):
            z_qi, l_i, i_i = self.quantize(residual.clone())
            residual = residual - z_qi
            z_q = z_q + z_qi
            losses.append(l_i)
            idxs.append(i_i)
        return z_q, torch.stack(losses, dim=-1).mean(), torch.stack(idxs, dim=-1)

    def lookup(self, code: torch.Tensor) -> torch.Tensor:
        """decode_codes front half (reference vitvqgan.py:82-87): n(E[code]), summed over the depth axis when residual"""
        if self.fused:
            shp = code.shape[:-1] if self.use_residual else code.shape
            out, _ = _C.vq_lookup(self.embedding.weight.detach().contiguous(), code.reshape(-1, self.depth).contiguous(), self.use_norm,
                                  want_bf16=False)
            return out.view(*shp, self.embed_dim)
        q = self.norm(torch.nn.functional.embedding(code, self.embedding.weight))
        return q.sum(-2) if self.use_residual else q
