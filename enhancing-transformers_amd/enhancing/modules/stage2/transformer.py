"""CondTransformer (reference enhancing/modules/stage2/transformer.py:23-95): a condition model, a frozen stage-1 tokenizer and the prior (GPT, or
RQTransformer over a residual stage 1's codes [B, N, D]); `sample` draws codes on the device and decodes them with the tokenizer, `complete`
keeps the top token rows of given images and draws the rest; `forward` /
`validation_step` give the teacher-forced logits and the reference's val/total_loss; `loss_and_grads` returns the training loss and leaves the
gradient of every parameter of the prior on the device (forward_backward); `configure_optimizers` returns the reference's Adam as one device launch
(engine/optim.py GPTAdam) and `training_step` runs the loss-scaled forward + backward against it (Trainer.fit drives both, on one GPU).

With an `RQTransformer`, sampling and training exist on a ROCm device only: `sample` with conditions that are not on the device raises
NotImplementedError, and a prior that is elsewhere is refused by the training entries before the tokenizer runs."""
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from ...utils.general import initialize_from_config
from .layers import GPT, RQTransformer  # noqa: F401  (the reference's `from .layers import *`)


class CondTransformer(nn.Module):
    def __init__(self, cond_key: str, cond, stage1, transformer, path: Optional[str] = None, ignore_keys: List[str] = list(),
                 code_shape: Optional[List[int]] = None, scheduler=None) -> None:
        super().__init__()
        self.cond_key = cond_key
        self.code_shape = code_shape
        self.scheduler = scheduler
        self.logged = {}
        self.cond_model = initialize_from_config(cond)
        self.stage1_model = initialize_from_config(stage1)
        self.transformer = initialize_from_config(transformer)
        # the tokenizer is frozen by never being stepped: its engine keeps the operand copies of the parameters that require a gradient (engine/stage1.py
        # ParamStore), so the reference's requires_grad = False loop would take the decoder's weights out of that store
        self.stage1_model.eval()
        self.cond_model.eval()
        for p in self.cond_model.parameters():
            p.requires_grad = False
        if path is not None:
            self.init_from_ckpt(path, ignore_keys)

    def init_from_ckpt(self, path: str, ignore_keys: List[str] = list()):
        """reference transformer.py:67-76"""
        sd = torch.load(path, map_location="cpu")["state_dict"]
        for k in list(sd.keys()):
            for ik in ignore_keys:
                if k.startswith(ik):
                    print("Deleting key {} from state_dict.".format(k))
                    del sd[k]
        self.load_state_dict(sd, strict=False)
        print(f"Restored from {path}")

    @torch.no_grad()
    def forward(self, codes: torch.Tensor, conds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """reference transformer.py:56-65: (teacher-forced logits [B, T, V], the codes as [B', T']).  Inference only (GPT.forward): no autograd graph."""
        conds = conds.view(conds.shape[0], -1)
        logits = self.transformer(codes, conds)
        return logits, codes.view(-1, codes.shape[-1])

    @torch.no_grad()
    def sample(self, conds: torch.Tensor, top_k: Optional[float] = None, top_p: Optional[float] = None, softmax_temperature: float = 1.0,
               use_fp16: bool = True, **kw) -> torch.Tensor:
        """reference transformer.py:78-95, for both priors: GPT draws codes [B, T], RQTransformer [B, T, D] (for a residual tokenizer), and
        `code_shape` is applied to them as the reference does (e.g. [32, 32] or [32, 32, 4]).  **kw goes to the prior's sample (seed, forced_codes,
        slot0_ln, graph, weights, cache, prefix_codes, ...); prefix_codes may have the code_shape's axes ([B, h', w] or [B, h', w, D]: whole token
        rows from the top).  The codes, given and drawn, are kept in `last_codes`.  An RQ prior that is off the device refuses (sampling runs on a ROCm device only)."""
        conds = conds.view(conds.shape[0], -1)
        kw.setdefault("return_logits", False)
        _, codes = self.transformer.sample(conds=conds, top_k=top_k, top_p=top_p, softmax_temperature=softmax_temperature, use_fp16=use_fp16, **kw)
        if self.code_shape is not None:
            codes = codes.view(codes.shape[0], *self.code_shape)
        self.last_codes = codes
        return self.stage1_model.decode_codes(codes).clamp(0, 1)

    @torch.no_grad()
    def complete(self, images: torch.Tensor, conds: torch.Tensor, keep: float = 0.5, **kw) -> torch.Tensor:
        """image completion: tokenizes `images` with the frozen stage 1 (encode_codes), keeps the first floor(keep * rows) token rows in raster
        order (rows: code_shape[0], or sqrt(img_num_tokens) without a code_shape) and samples the rest given them (the prior's
        sample(prefix_codes=): one batched prefill instead of a step per kept token); returns the decoded pixels as `sample` does and leaves the
        codes, kept and drawn, in `last_codes`.  **kw goes to `sample` (top_k, seed, graph, weights, cache, ...).  keep * rows below 1 keeps
        nothing (a plain sample); keeping every row is a ValueError: nothing is left to draw."""
        T = self.transformer.img_num_tokens
        rows = int(self.code_shape[0]) if self.code_shape is not None else int(round(T ** 0.5))
        if not float(keep) >= 0.0 or rows < 1 or T % rows:
            raise ValueError(f"CondTransformer.complete: keep must be >= 0 and the {T} tokens whole rows of a grid of {rows} rows, got keep = {keep}")
        codes = self.stage1_model.encode_codes(images).detach()
        B = codes.shape[0]
        codes = codes.reshape(B, T, -1) if isinstance(self.transformer, RQTransformer) else codes.reshape(B, T)
        prefix = codes[:, :int(float(keep) * rows) * (T // rows)]
        return self.sample(conds.to(codes.device), prefix_codes=prefix, **kw)

    def get_input(self, batch, key: str) -> torch.Tensor:
        """reference transformer.py:97-105"""
        x = batch[key]
        if len(x.shape) == 3:
            x = x[..., None]
        if x.dtype == torch.double:
            x = x.float()
        return x.contiguous()

    def _rq_on_device(self, what: str) -> None:
        """with an RQTransformer: refuses a prior that is not on a ROCm device, before anything is tokenized (the batch itself may come from the
        host, as Trainer.fit's does: the tokenizer moves it)"""
        tr = getattr(self, "transformer", None)
        if isinstance(tr, RQTransformer) and not tr.head.weight.is_cuda:
            raise NotImplementedError(f"CondTransformer.{what} with an RQTransformer: RQ training runs on a ROCm device only (the RQ prior's backward "
                                      "and its optimizer step are HIP kernels: there is no CPU path); move the transformer to the device first")

    def log(self, name: str, value, **_) -> None:
        """Lightning's ``self.log`` as the stage-1 module keeps it: the last value per name, in `logged`"""
        self.logged[name] = value

    @torch.no_grad()
    def _tokenize(self, batch) -> Tuple[torch.Tensor, torch.Tensor]:
        """reference transformer.py:107-113: (codes of the batch's images from the frozen tokenizer, the encoded condition [B, 1]) on the device"""
        images = self.get_input(batch, self.stage1_model.image_key)
        conds = self.get_input(batch, self.cond_key)
        codes = self.stage1_model.encode_codes(images).detach()
        conds = self.cond_model.encode_codes(conds).detach()
        return codes, conds.to(codes.device).view(conds.shape[0], -1)

    @torch.no_grad()
    def shared_step(self, batch, batch_idx: int) -> torch.Tensor:
        """reference transformer.py:107-118: tokenize the images, encode the condition, run the teacher-forced forward and take the mean
        cross-entropy of every code given the condition and the codes before it, on the device (enh_cross_entropy_rows)"""
        codes, conds = self._tokenize(batch)
        _, _, loss = self.transformer(codes, conds, return_loss=True)
        return loss

    def loss_and_grads(self, batch, batch_idx: int = 0, *, loss_scale: float = 1.0) -> torch.Tensor:
        """shared_step's prologue, then the prior's forward_backward: returns the unscaled training loss (also logged as train/total_loss) and leaves
        loss_scale x its gradient in `.grad` of every parameter of the transformer.  training_step is this with the optimizer's device loss scale."""
        self._rq_on_device("loss_and_grads")
        codes, conds = self._tokenize(batch)
        loss = self.transformer.forward_backward(codes, conds, loss_scale=loss_scale)
        self.log("train/total_loss", loss, on_step=True, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def validation_step(self, batch, batch_idx: int) -> torch.Tensor:
        """reference transformer.py:126-130: the loss, also logged as val/total_loss"""
        loss = self.shared_step(batch, batch_idx)
        self.log("val/total_loss", loss, on_step=True, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def training_step(self, batch, batch_idx: int, optimizer_idx: int = 0, *, zero_grad: bool = True) -> torch.Tensor:
        """reference transformer.py:120-124 with Lightning's backward folded in: tokenize the batch, run the prior's forward_backward with the optimizer's
        device loss scale (fp16 operands; none under bf16), log train/total_loss and return the unscaled loss.  zero_grad=False adds to the
        gradients of the batches before it (accumulate_grad_batches).  The optimizer of configure_optimizers() then steps: Trainer.fit, or
        `opt.step()` by hand."""
        self._rq_on_device("training_step")
        opt = self.__dict__.get("_optimizer")
        if opt is None:
            who = "RQ training" if isinstance(getattr(self, "transformer", None), RQTransformer) else "stage-2 training"
            raise NotImplementedError(f"{who} needs its optimizer first: set `learning_rate` and call configure_optimizers() before "
                                      "training_step (it builds the flat buffers and the loss scale the step runs against)")
        codes, conds = self._tokenize(batch)
        scale = opt.loss_scale
        loss = self.transformer.forward_backward(codes, conds, loss_scale=1.0 if scale is None else scale, accumulate=not zero_grad)
        self.log("train/total_loss", loss, on_step=True, on_epoch=True, prog_bar=True, logger=True)
        return loss

    def configure_optimizers(self):
        """reference transformer.py:132-194: Adam(lr, betas=(0.9, 0.96)) with the L2 decay 0.01 on the Linear weights only -> ([GPTAdam], schedulers)
        (engine/optim.py; one launch over the prior's flat buffers).  The transformer must be on the device.  Calling it again builds a new optimizer
        (fresh moments) over the same parameters."""
        self._rq_on_device("configure_optimizers")
        lr = self.__dict__.get("learning_rate")
        if lr is None:
            raise NotImplementedError("stage-2 training needs a learning rate: set `model.learning_rate` (main.py does) before configure_optimizers()")
        from ...engine.optim import GPTAdam
        # adam_state: "f32" | "bf16" moments (main.py --adam_state); unset = ENH_ADAM_STATE, default f32
        opt = GPTAdam(self.transformer, lr=lr, betas=(0.9, 0.96), weight_decay=0.01, state=self.__dict__.get("adam_state"))
        self.__dict__["_optimizer"] = opt
        schedulers = []
        if self.scheduler is not None:
            self.scheduler.params.start = lr
            sched = initialize_from_config(self.scheduler)
            schedulers = [{"scheduler": sched, "interval": "step", "frequency": 1}]
        return [opt], schedulers
