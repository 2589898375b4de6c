"""The reference of the stage-1 optimizers' loss-scaled step, shared by tests/test_amp_protocol_cpu.py and tests/test_amp_protocol_gpu.py: torch's own
torch.amp.GradScaler around torch.optim.AdamW on the CPU (what the reference runs under --use_amp), and ONE schedule of steps that visits the places
where a scaled optimizer goes wrong — the first update applied after a dropped step above all: GradScaler.step does not call optimizer.step() on an
overflow, so AdamW's step number, and with it both bias corrections, are those of the APPLIED steps.

No device code here.  Limits: gpt_train_util.check_limit through step_helpers_util.adamw_check (4 x the error of the f32 torch run + one ulp, on the
norm and on the worst element, both against the fp64 torch run); tests/test_amp_protocol_cpu.py shows that an optimizer whose step number also counts
the dropped steps lands more than 10 x outside that limit at these learning rates (at the shipped 4.5e-6 the update is too small against p for the
limit to see it: 1.1 - 2 x, which is why the schedule does not use it)."""
import torch

from step_helpers_util import F32, F64, f32v
from test_step_helpers_gpu import _adamw_case

INF, NAN = float("inf"), float("nan")
INIT_SCALE, GROWTH_INTERVAL = 65536.0, 3
BETAS, EPS, WD = (0.9, 0.99), 1e-8, 0.1
BAD_INDEX = 1234            # where a bad step's inf / nan sits (modulo the length)
CLIP_NORM, CLIP_VALUE = ("norm", 100.0), ("value", 0.01)      # the gradient's norm is >= 500 (one element of 1e3, grad_scale >= 0.5): the norm clip always bites

# step:        1      2     3      4      5     6     7      8     9     10    11     12    13    14    15    16
_BAD = ["inf", None, "nan", "inf", None, None, "nan", None, None, None, "inf", None, None, None, None, None]
# scale  2^:  15     15    14     13     13    13    12     12    12    13    12     12    12    13    13    13      (after the step)
# tracker:     0      1     0      0      1     2     0      1     2     0     0      1     2     0     1     2
APPLIED = [0, 1, 1, 1, 2, 3, 3, 4, 5, 6, 6, 7, 8, 9, 10, 11]      # AdamW's state["step"] after each step, written down by hand from the rule above
SCALES = [2.0 ** e for e in (15, 15, 14, 13, 13, 13, 12, 12, 12, 13, 12, 12, 12, 13, 13, 13)]
TRACKERS = [0, 1, 0, 0, 1, 2, 0, 1, 2, 0, 0, 1, 2, 0, 1, 2]


def _lr(i: int) -> float:
    """1e-2 and 1e-3 in turn, under a linear warm-up over the first ten steps: no two successive steps share a learning rate"""
    return (1e-2 if i % 2 else 1e-3) * min(1.0, i / 10.0)


# (bad, lr, clip, grad_scale) per step; bad: None | "inf" | "nan"; clip: None | ("norm", max_norm) | ("value", clip_value)
SCHEDULE = [(_BAD[i - 1], _lr(i), (None, CLIP_NORM, CLIP_VALUE)[i % 3], 0.5 if i % 4 in (2, 3) else 1.0) for i in range(1, 17)]


def case(n: int, seed: int = 5):
    """(p0, g, ordinary): _adamw_case's parameters, base gradient (most ~1e-2, a slice ~1e-8, a slice exactly zero, one element 1e3) and the mask of
    the parameters that are not the four of extreme size (70000 .. 5e-8), whose f32 rounding otherwise sets the worst-element limit for everyone"""
    return _adamw_case(n, seed)


def scaled_grad(g: torch.Tensor, i: int, scale: float, bad) -> torch.Tensor:
    """what the backward of step i (0-based) leaves in the flat gradient: the f32 gradient g (1 + 0.25 (i % 3)) times the current loss scale (a power
    of two: exact), with one inf / nan at BAD_INDEX on a bad step"""
    gs = (g * (1.0 + 0.25 * (i % 3))).to(F32) * scale
    if bad:
        gs[BAD_INDEX % gs.numel()] = INF if bad == "inf" else NAN
    return gs


class TorchAmpAdamW:
    """torch.amp.GradScaler("cpu") around torch.optim.AdamW over one tensor in `dtype`.  The hyper-parameters enter as the f32 values the C ABI
    carries (step_helpers_util.TorchAdamW).  AdamW's state exists from the start (zeros, as torch makes it on its first step), so p, m, v and the
    applied count can be read after a dropped first step too."""

    def __init__(self, p0, dtype, betas=BETAS, eps: float = EPS, wd: float = WD, init_scale: float = INIT_SCALE, growth_interval: int = GROWTH_INTERVAL):
        self.q = torch.nn.Parameter(p0.detach().cpu().to(dtype).clone())
        self.opt = torch.optim.AdamW([self.q], lr=1.0, betas=(f32v(betas[0]), f32v(betas[1])), eps=f32v(eps), weight_decay=f32v(wd))
        self.opt.state[self.q] = dict(step=torch.tensor(0.0), exp_avg=torch.zeros_like(self.q.data), exp_avg_sq=torch.zeros_like(self.q.data))
        self.scaler = torch.amp.GradScaler("cpu", init_scale=init_scale, growth_interval=growth_interval)
        self.dtype = dtype
        self.scaler.scale(torch.zeros(()))      # creates the scale tensor

    def step(self, g_scaled, lr: float, grad_scale: float, clip=None):
        self.opt.param_groups[0]["lr"] = f32v(lr)
        self.scaler.scale(torch.zeros(()))
        self.q.grad = (g_scaled.detach().cpu() * grad_scale).to(self.dtype)
        self.scaler.unscale_(self.opt)
        if clip is not None and clip[0] == "norm":
            torch.nn.utils.clip_grad_norm_([self.q], clip[1])
        elif clip is not None:
            self.q.grad.clamp_(-clip[1], clip[1])
        self.scaler.step(self.opt)
        self.scaler.update()
        return self

    def run(self, g, upto: int = len(SCHEDULE)):
        """the first `upto` steps of SCHEDULE on base gradient g; yields (i, record, self) after each"""
        for i, (bad, lr, clip, grad_scale) in enumerate(SCHEDULE[:upto]):
            yield i, SCHEDULE[i], self.step(scaled_grad(g, i, self.scale, bad), lr, grad_scale, clip)

    def p(self):
        return self.q.detach()

    def m(self):
        return self.opt.state[self.q]["exp_avg"]

    def v(self):
        return self.opt.state[self.q]["exp_avg_sq"]

    @property
    def applied(self) -> int:
        return int(self.opt.state[self.q]["step"].item())

    @property
    def scale(self) -> float:
        return float(self.scaler.get_scale())

    @property
    def tracker(self) -> int:
        return int(self.scaler._get_growth_tracker())


def clip_fields(clip):
    """a schedule record's clip as the optimizers' two attributes (gradient_clip_val, gradient_clip_algorithm)"""
    return (None, "norm") if clip is None else (clip[1], clip[0])
