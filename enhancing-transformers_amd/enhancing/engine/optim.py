"""Optimizer facade over the engine's flat buffers (what ``ViTVQ.configure_optimizers`` returns in place of
``torch.optim.AdamW``, reference vitvqgan.py:160)."""
from __future__ import annotations

from typing import Optional, Tuple


class _GradClip:
    """Lightning's gradient_clip_val / gradient_clip_algorithm / track_grad_norm for one optimizer (Lightning 1.5 clips each optimizer's own parameters with
    the same threshold).  "norm": torch.nn.utils.clip_grad_norm_(params, gradient_clip_val); "value": clamp to +-gradient_clip_val.  track_grad_norm: the
    2-norm of the final gradient is measured whether or not it is clipped.  All off by default: the step is then today's launches, argument for argument."""
    gradient_clip_val: Optional[float] = None
    gradient_clip_algorithm: str = "norm"
    track_grad_norm: bool = False

    def _clip_args(self) -> Tuple[Optional[float], Optional[float]]:
        """(clip_norm, clip_value) of this step: clip_norm = inf measures the norm and clips nothing"""
        val = self.gradient_clip_val or None          # Lightning: 0 / None = no clipping
        if val is not None and val < 0:
            raise ValueError(f"gradient_clip_val must be >= 0, got {val!r}")
        if self.gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm must be 'norm' or 'value', got {self.gradient_clip_algorithm!r}")
        by_norm = val is not None and self.gradient_clip_algorithm == "norm"
        clip_norm = float(val) if by_norm else (float("inf") if self.track_grad_norm else None)
        return clip_norm, (float(val) if val is not None and not by_norm else None)

    _clip_out = None      # (total_norm, clip coefficient) on the device, allocated by the first step that wants the norm

    def _clip_buf(self, clip, device):
        if clip[0] is not None and self._clip_out is None:
            import torch
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=device)
        return self._clip_out

    @property
    def grad_norm(self):
        """2-norm of the gradient the last step applied, before clipping (device f32 [1]; None until a step ran with clipping by norm or tracking on)"""
        return None if self._clip_out is None else self._clip_out[:1]


class LossScaler:
    """torch.cuda.amp.GradScaler's state machine with every quantity on the device: the one scaler under the three optimizers (the fp16 engine's, the
    discriminator's ParamStore, GPTAdam's), stepped by `scaled_step` below.  `enabled` False is the identity everywhere; the discriminator's is switched
    by the forward that builds the graph (fp16 operands in the loss networks: gradients of ~1e-5 would sit in fp16's subnormal range).
    Initial scale: the environment variable `env` names.  ENH_LOSS_SCALE (2^16, GradScaler's) for the engine and GPTAdam; ENH_LOSS_NET_SCALE (2^12) for
    the loss networks: a gradient of 1 per logit, times the scale, has to fit fp16 itself, and 2^16 would spend its first steps backing off.  Growth x2
    after ENH_LOSS_SCALE_INTERVAL (2000, GradScaler's; 0 = never) clean steps, x0.5 on an inf / nan (that step is skipped: it writes nothing and does
    not count as an AdamW step, see `step_operand`).
    check=False scales but does not check (the engine's ENH_NONFINITE_CHECK=0): found_inf is None, no step is dropped and the scale never moves.
    count_skipped: keep `skipped_steps`, a device count of the dropped steps (the engine's; read it with .item() outside the step).
    state_dict / load_state_dict: scale, tracker and skipped_steps on the host, what an optimizer's checkpoint carries as its `scaler` entry."""
    DEFAULT_SCALE = dict(ENH_LOSS_SCALE=65536.0, ENH_LOSS_NET_SCALE=4096.0)

    def __init__(self, device, init_scale: float = None, growth_interval: int = None, env: str = "ENH_LOSS_NET_SCALE", enabled: bool = False,
                 check: bool = True, count_skipped: bool = False) -> None:
        import os
        import torch
        init_scale = float(os.environ.get(env, self.DEFAULT_SCALE[env])) if init_scale is None else float(init_scale)
        self.growth_interval = int(os.environ.get("ENH_LOSS_SCALE_INTERVAL", 2000)) if growth_interval is None else int(growth_interval)
        self.scale_t = torch.full((1,), init_scale, dtype=torch.float32, device=device)
        self.tracker = torch.zeros(1, dtype=torch.int32, device=device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=device) if check else None      # written by the flag / norm pass, read by the Adam launch
        self.skipped_steps = torch.zeros(1, dtype=torch.float32, device=device) if check and count_skipped else None
        self.enabled = enabled

    def scale(self, t):
        return t * self.scale_t.view(()) if self.enabled else t

    def unscale(self, t):
        return t / self.scale_t.view(()) if self.enabled else t

    @property
    def value(self) -> float:
        return float(self.scale_t.item()) if self.enabled else 1.0

    @property
    def checks(self) -> bool:
        """this scaler can drop the step it is handed"""
        return self.enabled and self.found_inf is not None

    def state_dict(self) -> dict:
        return dict(scale=self.scale_t.detach().cpu(), tracker=self.tracker.detach().cpu(),
                    skipped_steps=None if self.skipped_steps is None else self.skipped_steps.detach().cpu())

    def load_state_dict(self, sd: dict) -> None:
        self.scale_t.copy_(sd["scale"]); self.tracker.copy_(sd["tracker"])
        if self.skipped_steps is not None and sd.get("skipped_steps") is not None:
            self.skipped_steps.copy_(sd["skipped_steps"])


def step_operand(store, scaler=None):
    """The `step` operand of the AdamW launch `store`'s next optimizer step makes, and the bookkeeping that goes with it.
    Without a scaler that can drop the step (bf16 / fp32, a disabled scaler, ENH_NONFINITE_CHECK=0) every step is applied: the host count
    `store.step_count` advances and goes in by value.  Under a scaler that checks the host cannot know whether this step will be applied, and
    GradScaler.step does not call AdamW's step on an overflow: the count moves to the device (`store.step_state`, f64 [4] = applied steps and the two
    bias-correction factors of _C.adamw_step) where the launch advances it only when the flag is clear — no host read, nothing to synchronise on.  From
    its first such step on a store keeps the device count (an unchecked step then advances it unconditionally); `store.step_count` reads it."""
    if getattr(store, "step_state", None) is None and (scaler is None or not scaler.checks):
        store.step_count += 1
        return store.step_count
    return device_step_count(store)


def applied_steps(store) -> int:
    """the number of steps `store`'s optimizer has applied, wherever it is counted (reads the device count when there is one: synchronises)"""
    state = getattr(store, "step_state", None)
    return store.step_count if state is None else int(state[0].item())


def device_step_count(store):
    """move `store`'s step number to the device, once (the fp16 engine does at construction, so that its step never allocates) -> store.step_state"""
    if getattr(store, "step_state", None) is None:
        import torch
        state = torch.zeros(4, dtype=torch.float64, device=store.p.device)
        state[0] = store.step_count
        store.step_state = state
    return store.step_state


def scaled_step(g, grad_scale: float, clip, clip_out, scaler, adam, grads_unscaled: bool = False) -> None:
    """The clipped, loss-scaled optimizer step all three optimizers take: GradScaler.step + GradScaler.update around the caller's Adam launch, with no
    host read and no allocation, so a HIP graph can capture it.
    g: the flat f32 gradient, already reduced; grad_scale: what the launch multiplies it by (1 / accumulation window / world size).
    clip: _GradClip._clip_args()'s (clip_norm, clip_value): clip_norm = inf measures the norm and clips nothing, clip_value None / 0 is off.
    clip_out: the caller's (total_norm, coefficient) f32 [2]; touched only when clip_norm is not None.
    scaler: a LossScaler; None or a disabled one: no scale, no check.  grads_unscaled: the scale was already divided out of g (Stage1Engine.unscale_grads):
    neither launch gets the loss_scale operand, the flag and the update still run.
    adam: the caller's Adam launch; called once, with exactly those of skip_flag / loss_scale / clip_coef / clip_value that apply (none: the plain call).
    Under a scaler that checks: one pass over g sets found_inf (the norm pass when there is one: the sum of squares and the flag ride on the same loads),
    the Adam launch reads it and writes nothing when it is set — its step number included, which therefore lives on the device (step_operand below,
    GPTAdam's `state`) — and enh_loss_scale_update halves / doubles the scale on the device."""
    from .. import _C
    clip_norm, clip_value = clip
    sc = scaler if scaler is not None and scaler.enabled else None
    norm_kw, kw = {}, {}      # the scaler's operands of the norm pass; the scaler's and the clip operands of the Adam launch
    flag = sc.found_inf if sc is not None else None
    if flag is not None:
        flag.zero_()
        norm_kw["found_inf"] = kw["skip_flag"] = flag
    if sc is not None and not grads_unscaled:
        norm_kw["loss_scale"] = kw["loss_scale"] = sc.scale_t
    if clip_norm is not None:
        _C.grad_clip_coef(g, clip_norm, grad_scale, clip_out, **norm_kw)
        if clip_norm != float("inf"):
            kw["clip_coef"] = clip_out[1:]
    elif flag is not None:
        _C.nonfinite_flag(g, flag)
    if clip_value:
        kw["clip_value"] = float(clip_value)
    adam(**kw)
    if flag is not None:
        _C.loss_scale_update(sc.scale_t, flag, sc.tracker, 2.0, 0.5, sc.growth_interval)
        if sc.skipped_steps is not None:      # (the update and the Adam kernels only read the flag)
            sc.skipped_steps.add_(flag)


class _StoreAdamW(_GradClip):
    """what FusedAdamW and FlatAdamW share: AdamW's state lives in `self.store` (a ParamStore: step_count, m, v), GradScaler's in `self.scaler`
    (the engine's or the store's LossScaler, or None).  `step` is torch's state["step"]: the number of APPLIED steps; a step the scaler drops does not
    count (step_operand above).  An enabled scaler is part of the state: a run restored without it would restart at the initial scale and drop a burst
    of steps the uninterrupted run does not drop."""

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.store.zero_grad()

    def state_dict(self) -> dict:
        s, sc = self.store, self.scaler
        sd = dict(step=applied_steps(s), m=s.m.detach().cpu(), v=s.v.detach().cpu(), param_groups=self.param_groups)
        if sc is not None and sc.enabled:
            sd["scaler"] = sc.state_dict()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        s, sc = self.store, self.scaler
        s.step_count = int(sd["step"])
        s.m.copy_(sd["m"]); s.v.copy_(sd["v"])
        self.param_groups = sd["param_groups"]
        if sc is not None and "scaler" in sd:      # (a checkpoint written before the scaler was part of it has no entry: the scale starts over)
            sc.load_state_dict(sd["scaler"])


class FusedAdamW(_StoreAdamW):
    """torch.optim.AdamW over the engine's flat buffers (Stage1Engine.optimizer_step).  Under the fp16 engine step() is GradScaler.step +
    GradScaler.update around it, on the device: an overflow drops the step, which then writes nothing, is counted in engine.skipped_steps and leaves
    AdamW's step number where it was, so the next applied update carries the bias corrections torch's would.  state_dict() holds the scaler."""

    def __init__(self, engine, lr: float, betas=(0.9, 0.99), eps: float = 1e-8, weight_decay: float = 1e-4) -> None:
        self.engine = engine
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        self.grad_scale = 1.0  # 1 / accumulate_grad_batches

    @property
    def store(self):
        return self.engine.store

    @property
    def scaler(self):
        return getattr(self.engine, "scaler", None)

    @property
    def grad_norm(self):
        """2-norm of the gradient the last step applied, before clipping (device f32 [1]; meaningful once a step ran with clipping by norm or tracking on)"""
        return self.engine.grad_norm

    def step(self) -> None:
        g = self.param_groups[0]
        clip_norm, clip_value = self._clip_args()
        self.engine.optimizer_step(g["lr"], g["betas"], g["eps"], g["weight_decay"], self.grad_scale, clip_norm=clip_norm, clip_value=clip_value)


class FlatAdamW(_StoreAdamW):
    """The same fused AdamW launch over any ``ParamStore`` (here: the discriminator's, the second optimizer of reference
    vitvqgan.py:163-164).  Under DDP the gradient buckets are all-reduced behind the discriminator's own backward (``attach_sync``: an
    ``AutogradGradSync`` whose hooks fire as autograd finishes each bucket; ``step`` only waits for what is still in flight) — a process group
    without an attached sync falls back to ONE blocking all-reduce of the flat buffer right before the step."""

    def __init__(self, store, lr: float, betas=(0.9, 0.99), eps: float = 1e-8, weight_decay: float = 1e-4) -> None:
        self.store = store
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        self.grad_scale = 1.0
        self.comm = None

    @property
    def scaler(self):
        """the store's LossScaler (the discriminator's: losses/vqperceptual.py disc_store), or None"""
        return getattr(self.store, "loss_scaler", None)

    def attach_sync(self, module, **kw):
        """bucketed asynchronous gradient all-reduce for this store, driven by autograd hooks on `module`'s parameters (engine/ddp.py)"""
        from .ddp import AutogradGradSync
        # one sync per store: a previous attach (Trainer.fit calls configure_optimizers + attach_sync on every invocation) left post-accumulate-grad hooks on
        # the same parameters — still live, they would all-reduce every bucket a second time and the step would divide by the world size only once
        # (ADVICE r5); the old object's hooks are removed and its in-flight handles drained before it is replaced
        old = getattr(self.store, "_grad_sync", None) or self.comm
        if old is not None:
            old.finish()
            old.remove_hooks()
        self.comm = AutogradGradSync(self.store, list(module.named_parameters()), **kw)
        self.store._grad_sync = self.comm
        return self.comm

    def detach_sync(self) -> None:
        """remove the autograd hooks of attach_sync (end of Trainer.fit: the module may be fitted again, or used without a process group)"""
        if self.comm is not None:
            self.comm.finish()
            self.comm.remove_hooks()
            self.comm = None
            self.store._grad_sync = None

    def step(self) -> None:
        import torch.distributed as dist
        from .. import _C
        s, g = self.store, self.param_groups[0]
        scale = self.grad_scale
        if self.comm is not None:
            self.comm.finish()
            scale /= self.comm.world
        elif dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(s.g)
            scale /= dist.get_world_size()
        clip, step = self._clip_args(), step_operand(s, self.scaler)
        scaled_step(s.g, scale, clip, self._clip_buf(clip, s.g.device), self.scaler, lambda **kw: _C.adamw_step(
            s.p, s.g, s.m, s.v, None, step, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], scale, **kw))
        from ..losses.op.conv_nhwc import invalidate_packed_weights
        invalidate_packed_weights()          # the kernel wrote the weights through raw pointers: cached operand images are stale


def gpt_param_groups(gpt):
    """(decay, no_decay): the sorted parameter names of the reference's two Adam groups (modules/stage2/transformer.py:140-180, after minGPT): the
    weights of the Linear layers get the L2 decay; biases, LayerNorm and Embedding weights, the position tables and time_mix get none.  Every
    parameter is in exactly one group (the reference asserts it; so does this)."""
    import torch.nn as nn
    decay, no_decay = set(), set()
    for mn, mod in gpt.named_modules():
        for pn, _ in mod.named_parameters(recurse=False):
            fpn = f"{mn}.{pn}" if mn else pn
            if pn.endswith("bias"):
                no_decay.add(fpn)
            elif pn.endswith("weight") and isinstance(mod, nn.Linear):
                decay.add(fpn)
            elif pn.endswith("weight") and isinstance(mod, (nn.LayerNorm, nn.Embedding)):
                no_decay.add(fpn)
            elif "time_" in pn or pn in ("pos_emb_cond", "pos_emb_code", "pos_emb_depth"):
                no_decay.add(fpn)
    names = {n for n, _ in gpt.named_parameters()}
    if decay & no_decay or names != decay | no_decay:
        raise RuntimeError(f"gpt_param_groups: parameters in both groups {sorted(decay & no_decay)} or in neither {sorted(names - decay - no_decay)}")
    return sorted(decay), sorted(no_decay)


class GPTAdam(_GradClip):
    """The reference's stage-2 optimizer (modules/stage2/transformer.py:176-181: torch.optim.Adam(betas=(0.9, 0.96)), L2 weight decay 0.01 on the
    Linear weights, 0 on everything else) as ONE launch of enh_adam_step_segments (csrc/gpt_adam.hip) over the GPT's flat buffers.

    Building it changes where the GPT's tensors live, not their values:
      * the parameters are re-homed, one by one (never two copies of the model), into one flat f32 buffer `p` with `GPT.flat_grad`'s layout
        (modules/stage2/prior.py `flat_layout`); state_dict keys and load_state_dict keep working (load_state_dict copies in place);
      * flat `m` and `v` are allocated, and the flat gradient (`GPT._flat_grads`);
      * the 16-bit GEMM operands move into one arena ([3C, C] wqkv | wproj | w0 | w1 per layer: prior.py `ARENA_LAYER`, then the head) that the
        step kernel rewrites in the same pass as the masters; `GPT._operand_copies` returns views into it and the per-layer copies it kept before are dropped.  The small f32
        copies that are no view of a master (the q | k | v bias concatenation) are rebuilt with torch after every step.
    Moving or replacing the parameters afterwards, or changing ENH_PRECISION, is refused with an error by the GPT and by step().

    With the fp16 operand format step() is GradScaler's step on the device (`scaled_step` above: found-inf, or the norm pass, which also finds it, the
    update with skip / unscale, enh_loss_scale_update); initial scale ENH_LOSS_SCALE (65536), growth interval ENH_LOSS_SCALE_INTERVAL (2000): torch's defaults.
    Under bf16 there is no scale and no skip.  The step count lives on the device (a dropped step does not advance it, and the host cannot know of
    a drop); only state_dict() reads it.  state_dict() copies m and v to the host: 88 GB at the shipped size (10.98 G parameters).

    state: "f32" (the default) or "bf16"; None reads ENH_ADAM_STATE.  "bf16" holds m and v as torch.bfloat16 (22 GB each at the shipped size instead
    of 44) and steps through enh_adam_step_segments_s16: 22 bytes per element instead of 30.  The moments are widened exactly, p is updated from the
    unrounded f32 new moments, and what is stored for the next step is rounded stochastically with Philox words of (state_seed, element group,
    applied step count): round-to-nearest would stall v once (1 - beta2) g^2 falls under half a bf16 ulp of v.  Same seed, same bits; a dropped step
    consumes no randomness.  Measured at the shipped size (profiles/gpt_train_adam16.txt): the launch 53.8 -> 43.6 ms, the training step 176 -> 166 ms
    at batch 1, peak memory 201 -> 160 GiB; convergence of a real run with bf16 moments has not been measured.  state_dict() stores m and v in the dtype they have, with `state_format` and `state_seed`; load_state_dict() accepts
    either form (bf16 -> f32 widens exactly, f32 -> bf16 rounds to nearest even once, no `state_format` = f32) and restores the seed, so a resumed
    run continues the stream.  Everything else (found-inf, unscale, clipping, the arena) is the f32 path's.

    Not built: 8-bit or block-scaled moments, a 16-bit master `p`, bf16 state for the stage-1 optimizers (FusedAdamW, FlatAdamW)."""
    STATE_FORMATS = ("f32", "bf16")

    @classmethod
    def _state_format(cls, state) -> str:
        """the `state` keyword resolved: None reads ENH_ADAM_STATE (default "f32"); anything but "f32" / "bf16" is a ValueError naming the value"""
        import os
        if state is None:
            state = os.environ.get("ENH_ADAM_STATE", "f32")
            if state not in cls.STATE_FORMATS:
                raise ValueError(f"ENH_ADAM_STATE={state!r}: expected one of {cls.STATE_FORMATS}")
        if state not in cls.STATE_FORMATS:
            raise ValueError(f"GPTAdam: state must be one of {cls.STATE_FORMATS} (or None: ENH_ADAM_STATE), got {state!r}")
        return state

    def __init__(self, gpt, lr: float, betas=(0.9, 0.96), eps: float = 1e-8, weight_decay: float = 0.01, init_scale: float = None,
                 growth_interval: int = None, state: Optional[str] = None, state_seed: int = 0) -> None:
        import torch
        self.state_format = self._state_format(state)      # before anything touches the device
        self.state_seed = int(state_seed)
        from .. import _C
        from ..modules.stage2.prior import ARENA_LAYER, ARENA_LAYER_SIZE, flat_layout, qkv_bias
        params = list(gpt.named_parameters())
        if not params or not all(p.is_cuda for _, p in params):
            raise RuntimeError("GPTAdam: the GPT's parameters must be on a ROCm device (model.to('cuda') first): the optimizer step is a HIP kernel and "
                               "there is no CPU path")
        if any(p.dtype != torch.float32 for _, p in params):
            raise RuntimeError("GPTAdam: the GPT's parameters must be float32 (the masters; the 16-bit operands are the optimizer's arena)")
        if any(p.numel() % 64 for _, p in params):      # a segment of the step kernel begins and ends on a multiple of 64 elements
            raise RuntimeError("GPTAdam: every parameter's element count must be a multiple of 64 (embed_dim is one for every GPT this package builds)")
        dev = params[0][1].device
        self.gpt = gpt
        self.dt = gpt._operand_dtype(True, "GPTAdam")
        decay, no_decay = gpt_param_groups(gpt)
        self.param_groups = [dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, names=decay),
                             dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0.0, names=no_decay)]
        self.grad_scale = 1.0
        # ---- flat masters: the gradients' layout ----
        layout, total = flat_layout(gpt)
        self.p = torch.zeros(total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for (_, p), (o, n) in zip(params, layout):
                dst = self.p[o:o + n].view(p.shape)
                dst.copy_(p.data)
                p.data = dst          # the old storage is released here, one parameter at a time
        sdt = torch.bfloat16 if self.state_format == "bf16" else torch.float32
        self.m = torch.zeros(total, dtype=sdt, device=dev)
        self.v = torch.zeros(total, dtype=sdt, device=dev)
        self.state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=dev)      # t, beta1^t, beta2^t
        # ---- operand arena: one ARENA_LAYER slice per Block, stack after stack, then the head ----
        C, V, stacks = gpt.embed_dim, gpt.vocab_img_size, gpt._block_stacks()
        CC = C * C
        head = sum(len(stack) for _, stack in stacks.values()) * ARENA_LAYER_SIZE * CC
        self.arena = torch.zeros(head + V * C, dtype=self.dt, device=dev)
        gpt._operands.clear()          # the per-layer copies (22 GB at the shipped size)
        where, ops, base = {"head.weight": head}, dict(head=self.arena[head:].view(V, C)), 0      # where: master -> its offset in the arena
        for key, (attr, stack) in stacks.items():
            ops[key] = []
            for i, blk in enumerate(stack):
                W = dict(bqkv=qkv_bias(blk.attn), time_mix=blk.attn.time_mix.detach().reshape(-1))
                for operand, masters, off, r, c in ARENA_LAYER:
                    o = base + off * CC
                    W[operand] = self.arena[o:o + r * c * CC].view(r * C, c * C)
                    for j, nm in enumerate(masters):
                        where[f"{attr}.{i}.{nm}.weight"] = o + j * (r * c * CC // len(masters))
                ops[key].append(W)
                base += ARENA_LAYER_SIZE * CC
        wd_of = {n: weight_decay for n in decay}
        segs = [(o, o + n_el, where.get(n, -1), wd_of.get(n, 0.0)) for (n, _), (o, n_el) in zip(params, layout)]
        self._dst = [(p, where[n]) for n, p in params if n in where]
        self.table = _C.adam_segment_table(segs, total, self.arena.numel(), dev)
        self._ptrs = tuple(p.data_ptr() for _, p in params)
        gpt._arena = dict(dt=self.dt, ptrs=self._ptrs, ops=ops, versions=None, refresh=self.refresh_operands)
        self.refresh_operands()
        gpt._flat_grads(dev)
        # ---- GradScaler on the device (fp16 operands only) ----
        self.scaler = LossScaler(dev, init_scale, growth_interval, env="ENH_LOSS_SCALE", enabled=True) if self.dt == torch.float16 else None

    @property
    def loss_scale(self):
        """device f32 [1]: what forward_backward(loss_scale=...) takes; None under bf16"""
        return None if self.scaler is None else self.scaler.scale_t

    def refresh_operands(self) -> None:
        """the arena and the q | k | v bias copies rebuilt from the masters with torch (one rounding from f32, as the copies the arena replaces).
        Runs at construction and whenever torch wrote a master in place (load_state_dict, an init): GPT._operand_copies sees the masters' version
        counters move and calls it.  The step kernel writes masters and arena together and moves no counter, so a step never comes here."""
        import torch
        gpt = self.gpt
        with torch.no_grad():
            for p, d in self._dst:
                self.arena[d:d + p.numel()].copy_(p.detach().view(-1))
            self._refresh_bias_copies()
        gpt._arena["versions"] = tuple(p._version for p in gpt.parameters())

    def _refresh_bias_copies(self) -> None:
        from ..modules.stage2.prior import qkv_bias
        for key, (_, stack) in self.gpt._block_stacks().items():
            for blk, W in zip(stack, self.gpt._arena["ops"][key]):
                qkv_bias(blk.attn, out=W["bqkv"])

    def zero_grad(self, set_to_none: bool = False) -> None:
        if self.gpt.flat_grad is not None:
            self.gpt.flat_grad.zero_()

    def _check_home(self) -> None:
        gpt = self.gpt
        if gpt._arena is None or gpt._arena["ptrs"] is not self._ptrs or tuple(p.data_ptr() for p in gpt.parameters()) != self._ptrs:
            raise RuntimeError("GPTAdam.step: the GPT's parameters were moved or replaced after this optimizer was built (or a newer GPTAdam owns them): "
                               "its flat buffers no longer belong to them; build a new GPTAdam (configure_optimizers)")
        if gpt._operand_dtype(True, "GPTAdam.step") != self.dt:
            raise RuntimeError(f"GPTAdam.step: the operand arena holds {self.dt} but the engine's operand format (ENH_PRECISION) changed; build a new GPTAdam")

    def step(self) -> None:
        from .. import _C
        self._check_home()
        gpt, g, h = self.gpt, self.gpt.flat_grad, self.param_groups[0]
        if g is None or g.numel() != self.p.numel():
            raise RuntimeError("GPTAdam.step: no gradients (run GPT.forward_backward / CondTransformer.training_step first)")
        clip = self._clip_args()
        launch, extra = (_C.adam_step_segments_s16, dict(seed=self.state_seed)) if self.state_format == "bf16" else (_C.adam_step_segments, {})
        scaled_step(g, self.grad_scale, clip, self._clip_buf(clip, g.device), self.scaler, lambda **kw: launch(
            self.p, g, self.m, self.v, self.arena, self.table, self.state, lr=h["lr"], beta1=h["betas"][0], beta2=h["betas"][1], eps=h["eps"],
            grad_scale=self.grad_scale, **extra, **kw))
        # the kernel wrote the masters through raw pointers: the f32 copies that are no view of a master are rebuilt (3C elements per layer), and
        # operand copies of any other format (the exact mode's f32 q | k | v) are dropped so that their next use rebuilds them
        self._refresh_bias_copies()
        gpt._operands.clear()

    def state_dict(self) -> dict:
        """step count, m, v and the scaler's state on the host (m and v in the dtype they have: 88 GB at the shipped size, 44 GB with bf16 state), the
        state's format and the seed of its rounding stream.  The one place the device step count is read."""
        st = self.state.detach().cpu()
        sd = dict(step=int(st[0].item()), state=st, m=self.m.detach().cpu(), v=self.v.detach().cpu(),
                  param_groups=[{k: v for k, v in g.items()} for g in self.param_groups], state_format=self.state_format, state_seed=self.state_seed)
        if self.scaler is not None:
            sd["scaler"] = dict(scale=self.scaler.scale_t.detach().cpu(), tracker=self.scaler.tracker.detach().cpu())
        return sd

    @staticmethod
    def _checkpoint_format(sd: dict) -> str:
        """the format of a checkpoint's moments, checked against their dtype; a dict without `state_format` (written before there was one) is f32"""
        import torch
        fmt = sd.get("state_format", "f32")
        if fmt not in GPTAdam.STATE_FORMATS:
            raise ValueError(f"GPTAdam.load_state_dict: state_format {fmt!r} is not one of {GPTAdam.STATE_FORMATS}")
        want = torch.bfloat16 if fmt == "bf16" else torch.float32
        for k in ("m", "v"):
            if sd[k].dtype != want:
                raise ValueError(f"GPTAdam.load_state_dict: state_format is {fmt!r} but {k} is {sd[k].dtype}")
        return fmt

    def load_state_dict(self, sd: dict) -> None:
        """either form of checkpoint into either form of state: bf16 -> f32 widens exactly, f32 -> bf16 rounds to nearest even once (copy_'s
        conversion); the seed of the rounding stream is restored when the checkpoint has one"""
        import torch
        self._checkpoint_format(sd)
        if "state" in sd:
            self.state.copy_(sd["state"])
        else:
            t, (b1, b2) = int(sd["step"]), self.param_groups[0]["betas"]
            self.state.copy_(torch.tensor([float(t), b1 ** t, b2 ** t, 0.0], dtype=torch.float64))
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
        if "state_seed" in sd:
            self.state_seed = int(sd["state_seed"])
        self.param_groups = [dict(g) for g in sd["param_groups"]]
        if self.scaler is not None and "scaler" in sd:
            self.scaler.scale_t.copy_(sd["scaler"]["scale"]); self.scaler.tracker.copy_(sd["scaler"]["tracker"])
