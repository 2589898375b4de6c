"""What the stage-2 training tests share (tests/test_gpt_train_cpu.py, test_gpt_adam_kernel_gpu.py, test_gpt_train_gpu.py): the host restatement
of csrc/gpt_adam.hip's arithmetic, torch.optim.Adam as the reference over a list of segments, and the limit the issue sets for the step:

    error of the device <= 4 x the error of torch.optim.Adam run in f32 on the CPU, both against torch.optim.Adam in fp64 on the CPU fed the same
    f32 gradients, + one f32 ulp of the value

applied per tensor (2-norms: the floor is the 2-norm of the ulps) and to the worst element (every element's error <= 4 x the f32 run's WORST
element error of that tensor + that element's ulp).  4 x is the project's margin over "the reference's own error" (tests/test_gpt_forward_gpu.py)."""
import json
import os

import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BETAS, EPS, WD = (0.9, 0.96), 1e-8, 0.01


def golden_groups(case: str) -> dict:
    with open(os.path.join(GOLD, "gpt_optim_groups.json")) as f:
        return json.load(f)[case]


def adam_step64(p, g, m, v, t: int, lr: float, wd, betas=BETAS, eps: float = EPS):
    """the arithmetic of enh_adam_step_segments, in the dtype of its operands (fp64 here), in place; t = the step count AFTER this step; wd a scalar
    or a tensor like p"""
    b1, b2 = betas
    gg = g + wd * p
    m.add_((gg - m) * (1.0 - b1))
    v.mul_(b2).add_(gg * gg * (1.0 - b2))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p.sub_((lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps)))


class TorchAdam:
    """torch.optim.Adam(betas, two groups: weight_decay per tensor 0.01 / 0) on the CPU in `dtype` over a list of tensors; step(grads) feeds the given
    gradients (converted to `dtype`), optionally clipped on the host first the way Lightning does"""

    def __init__(self, tensors, wds, lr: float, dtype, betas=BETAS, eps: float = EPS):
        self.params = [torch.nn.Parameter(t.detach().cpu().to(dtype).clone()) for t in tensors]
        dec = [p for p, w in zip(self.params, wds) if w != 0.0]
        nod = [p for p, w in zip(self.params, wds) if w == 0.0]
        groups = [dict(params=dec, weight_decay=WD)] if dec else []
        groups += [dict(params=nod, weight_decay=0.0)] if nod else []
        assert all(w in (0.0, WD) for w in wds)
        self.opt = torch.optim.Adam(groups, lr=lr, betas=betas, eps=eps)
        self.dtype = dtype

    def step(self, grads, scale: float = 1.0, clip_norm=None, clip_value=None, lr=None):
        if lr is not None:
            for g in self.opt.param_groups:
                g["lr"] = lr
        for p, g in zip(self.params, grads):
            p.grad = g.detach().cpu().to(self.dtype) * scale
        if clip_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.params, clip_norm)
        if clip_value is not None:
            torch.nn.utils.clip_grad_value_(self.params, clip_value)
        self.opt.step()

    def p(self):
        return [q.detach() for q in self.params]

    def m(self):
        return [self.opt.state[q]["exp_avg"] for q in self.params]

    def v(self):
        return [self.opt.state[q]["exp_avg_sq"] for q in self.params]


def ulp32(x64: torch.Tensor) -> torch.Tensor:
    """the spacing of f32 at |x| (fp64 tensor): one ulp of the value; the smallest normal's spacing below it"""
    a = x64.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def check_limit(dev, f32, ref64, what: str):
    """the limit of this module's docstring for one tensor; returns (norm ratio, worst-element ratio) = error / limit, asserting both <= 1"""
    dev, f32, ref64 = dev.detach().double().cpu().reshape(-1), f32.detach().double().cpu().reshape(-1), ref64.detach().double().cpu().reshape(-1)
    u = ulp32(ref64)
    e_dev, e_f32 = (dev - ref64).abs(), (f32 - ref64).abs()
    assert bool(torch.isfinite(dev).all()), f"{what}: non-finite values"
    norm_ratio = (e_dev.norm() / (4.0 * e_f32.norm() + u.norm())).item()
    elem_ratio = (e_dev / (4.0 * e_f32.max() + u)).max().item()
    assert norm_ratio <= 1.0, f"{what}: ||error|| is {norm_ratio:.3f} x (4 x the f32 reference's + one ulp)"
    assert elem_ratio <= 1.0, f"{what}: the worst element's error is {elem_ratio:.3f} x (4 x the f32 reference's worst + one ulp)"
    return norm_ratio, elem_ratio
