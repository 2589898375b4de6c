"""The loss-scaled AdamW protocol of the two stage-1 optimizers against torch's GradScaler + AdamW (tests/amp_protocol_util.py), the part that needs no
GPU.  (1) The reference's own trace over SCHEDULE has the events the schedule is for.  (2) The HOST logic of FlatAdamW.step and
Stage1Engine.optimizer_step, run over fp64 torch stand-ins for the launches, follows torch's classes to 1e-12.  (3) The same host logic over an f32
restatement of the kernels stays inside the limit the GPU tests apply at every step, and with the step number advanced on dropped steps too it lands
at least 10 x outside it at the first update after every drop: the GPU tests can see that fault."""
import pytest
import torch

from amp_protocol_util import (APPLIED, BETAS, EPS, GROWTH_INTERVAL, INIT_SCALE, SCALES, SCHEDULE, TRACKERS, WD, TorchAmpAdamW, case, clip_fields,
                               scaled_grad)
from gpt_train_util import ulp32
from step_helpers_util import F32, F64, adamw_check, f32v

N = 4101


def test_reference_trace_has_the_events_of_the_schedule():
    p0, g, _ = case(N)
    ref = TorchAmpAdamW(p0, F64)
    applied, scales, trackers, dropped = [], [], [], []
    for i, (bad, lr, clip, grad_scale), r in ref.run(g):
        before = applied[-1] if applied else 0
        applied.append(r.applied); scales.append(r.scale); trackers.append(r.tracker)
        dropped.append(r.applied == before)
        assert dropped[-1] == bool(bad), f"step {i + 1}: torch dropped {dropped[-1]}, the schedule says bad={bad}"
        if clip is not None and clip[0] == "norm":      # the norm clip bites: the final gradient's norm is well above the threshold
            assert (scaled_grad(g, i, 1.0, None).double() * grad_scale).norm().item() > 2 * clip[1]
    assert applied == APPLIED and scales == SCALES and trackers == TRACKERS
    assert all(2.0 <= s <= 2.0 ** 23 for s in [INIT_SCALE] + scales), "inside the range where the kernel's floor and cap play no part"
    d, before, scales0 = dropped, [0] + trackers[:-1], [INIT_SCALE] + scales[:-1]
    assert d[0], "a dropped first step"
    assert any(a and b for a, b in zip(d, d[1:])), "two dropped steps in a row"
    assert any(x and t == GROWTH_INTERVAL - 1 for x, t in zip(d, before)), "a drop on the step at which the tracker would have reached the interval"
    grew = [s == 2 * s0 for s, s0 in zip(scales, scales0)]
    assert any(grew) and all(up or s <= s0 for s, s0, up in zip(scales, scales0, grew)), "a growth step"
    assert any(up and x for up, x in zip(grew, d[1:])), "a drop directly after a growth"
    lrs = [r[1] for r in SCHEDULE]
    assert all(a != b for a, b in zip(lrs, lrs[1:]))
    assert all(l in (1e-2 * min(1.0, i / 10.0), 1e-3 * min(1.0, i / 10.0)) for i, l in enumerate(lrs, 1)), "1e-2 or 1e-3 times the warm-up factor"
    assert {r[3] for r in SCHEDULE} == {1.0, 0.5}
    assert {None if r[2] is None else r[2][0] for r in SCHEDULE} == {None, "norm", "value"}
    assert {r[0] for r in SCHEDULE} == {None, "inf", "nan"}
    first_after = [i + 1 for i in range(1, len(d)) if d[i - 1] and not d[i]]
    assert first_after == FIRST_AFTER_A_DROP


FIRST_AFTER_A_DROP = [2, 5, 8, 12]      # the steps (1-based) that apply the first update after a dropped one


# ---- the host logic of the two optimizers over torch stand-ins for the launches ---------------------------------------------------------------------
class _Store:
    """what FlatAdamW.step and Stage1Engine.optimizer_step touch of a ParamStore, on the CPU in `dtype`"""

    def __init__(self, p0, dtype):
        self.p = p0.to(dtype).clone()
        self.g, self.m, self.v, self.p16 = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p), None
        self.step_count, self.step_state, self.comm_done, self.grads_unscaled = 0, None, False, False

    def refresh_operands(self):
        pass


class _Launches:
    """torch stand-ins for the four launches of a step (the fifth, the skipped_steps add, is a torch call already), working in the dtype of the
    buffers they are handed: fp64 for the comparison with torch's classes, f32 as a restatement of the kernels' arithmetic (csrc/elementwise.hip
    adamw_kernel, operation for operation).  The Adam stand-in honours whatever step operand it is handed: a number goes into the bias corrections as
    it is, a device count is advanced unless the flag is set.  count_drops = True is the FAULT the GPU tests look for: the count advances on a
    dropped step too."""
    count_drops = False

    def install(self, monkeypatch):
        from enhancing import _C
        for name in ("nonfinite_flag", "grad_clip_coef", "adamw_step", "loss_scale_update"):
            monkeypatch.setattr(_C, name, getattr(self, name))
        return self

    @staticmethod
    def nonfinite_flag(x, flag):
        if not bool(torch.isfinite(x).all()):
            flag.fill_(1.0)

    def grad_clip_coef(self, g, max_norm, grad_scale, out, loss_scale=None, found_inf=None):
        if found_inf is not None:
            self.nonfinite_flag(g, found_inf)
        total = (g.double().norm() * grad_scale / (1.0 if loss_scale is None else loss_scale.item())).to(out.dtype)
        out[0] = total
        out[1] = torch.clamp(max_norm / (total + 1e-6), max=1.0) if bool(torch.isfinite(total)) else 1.0

    def adamw_step(self, p, g, m, v, p16, step, lr, b1, b2, eps, wd, grad_scale, skip_flag=None, loss_scale=None, clip_coef=None, clip_value=0.0):
        dropped = skip_flag is not None and skip_flag.item() != 0.0
        if isinstance(step, torch.Tensor):
            if not dropped or self.count_drops:
                step[0] += 1
            t = int(step[0].item())
        else:
            t = int(step)
        if dropped:
            return
        r = f32v if p.dtype == F32 else float          # a scalar operation of the kernel: in double on f32 values, rounded once
        gs = r(grad_scale)
        if loss_scale is not None:
            gs = r(gs / loss_scale.item())
        if clip_coef is not None:
            gs = r(gs * clip_coef.item())
        gg = g.to(p.dtype) * gs
        if clip_value:
            gg = gg.clamp(-r(clip_value), r(clip_value))
        inv_bc1, inv_sqrt_bc2 = r(1.0 / (1.0 - b1 ** t)), r(1.0 / (1.0 - b2 ** t) ** 0.5)
        p.mul_(r(1.0 - r(lr * wd)))
        m.copy_(m * b1 + gg * r(1.0 - b1))
        v.copy_(v * b2 + gg * gg * r(1.0 - b2))
        p.sub_(r(lr * inv_bc1) * (m / (v.sqrt() * inv_sqrt_bc2 + r(eps))))

    @staticmethod
    def loss_scale_update(scale, found_inf, tracker, growth, backoff, interval):
        if found_inf.item() != 0.0:
            scale.mul_(backoff); tracker.zero_()
        else:
            tracker.add_(1)
            if interval > 0 and int(tracker) >= interval:
                scale.mul_(growth); tracker.zero_()


def _optimizer(which: str, p0, dtype):
    """FlatAdamW over a _Store with a scaler, or FusedAdamW over a stand-in engine that runs Stage1Engine.optimizer_step itself -> (optimizer, store, scaler)"""
    from enhancing.engine.optim import FlatAdamW, FusedAdamW, LossScaler
    from enhancing.engine.stage1 import Stage1Engine
    st = _Store(p0, dtype)
    sc = LossScaler(torch.device("cpu"), init_scale=INIT_SCALE, growth_interval=GROWTH_INTERVAL, enabled=True, count_skipped=True)
    hyper = dict(lr=1.0, betas=(f32v(BETAS[0]), f32v(BETAS[1])), eps=f32v(EPS), weight_decay=f32v(WD))
    if which == "FlatAdamW":
        st.loss_scaler = sc
        opt = FlatAdamW(st, **hyper)
        opt._clip_out = torch.zeros(2, dtype=dtype)      # (the coefficient between the stand-ins in their precision)
    else:
        eng = type("Engine", (), dict(optimizer_step=Stage1Engine.optimizer_step))()
        eng.store, eng.scaler, eng.comm, eng.half, eng._clip_out = st, sc, None, False, torch.zeros(2, dtype=dtype)
        opt = FusedAdamW(eng, **hyper)
    return opt, st, sc


def _take(opt, st, gs, lr, clip, grad_scale):
    st.g.copy_(gs)
    opt.param_groups[0]["lr"], opt.grad_scale = f32v(lr), grad_scale
    opt.gradient_clip_val, opt.gradient_clip_algorithm = clip_fields(clip)
    opt.step()


def _rel(a, b) -> float:
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("which", ["FlatAdamW", "Stage1Engine"])
def test_host_protocol_follows_gradscaler_and_adamw(monkeypatch, which):
    _Launches().install(monkeypatch)
    p0, g, _ = case(N)
    ref = TorchAmpAdamW(p0, F64)
    opt, st, sc = _optimizer(which, p0, F64)
    drops = 0
    for i, (bad, lr, clip, grad_scale) in enumerate(SCHEDULE):
        S = sc.scale_t.item()
        assert S == ref.scale
        gs = scaled_grad(g, i, S, bad)
        ref.step(gs, lr, grad_scale, clip)
        _take(opt, st, gs, lr, clip, grad_scale)
        drops += bool(bad)
        what = f"{which} step {i + 1}"
        errs = [_rel(a, b) for a, b in zip((st.p, st.m, st.v), (ref.p(), ref.m(), ref.v()))]
        assert all(e <= 1e-12 for e in errs), f"{what}: p, m, v differ from GradScaler + AdamW in fp64 by {errs}"
        assert opt.state_dict()["step"] == ref.applied, f"{what}: applied steps {opt.state_dict()['step']}, torch's state['step'] {ref.applied}"
        assert (sc.scale_t.item(), int(sc.tracker), float(sc.found_inf), float(sc.skipped_steps)) == (ref.scale, ref.tracker, float(bool(bad)), float(drops)), what
    sd = opt.state_dict()
    assert sd["step"] == APPLIED[-1] and sd["scaler"]["scale"].item() == SCALES[-1] and int(sd["scaler"]["tracker"]) == TRACKERS[-1]
    assert float(sd["scaler"]["skipped_steps"]) == float(drops)


def _p_ratio(dev, f32, ref, keep) -> float:
    """check_limit's error / limit on p (the larger of the norm's and the worst element's) without its assertion, over the parameters `keep` as a
    tensor of their own, as adamw_check applies it"""
    d, a, r = dev.double()[keep], f32.p().double()[keep], ref.p().double()[keep]
    u, e_d, e_a = ulp32(r), (d - r).abs(), (a - r).abs()
    return max((e_d.norm() / (4.0 * e_a.norm() + u.norm())).item(), (e_d / (4.0 * e_a.max() + u)).max().item())


def test_a_step_count_that_advances_on_dropped_steps_is_far_outside_the_limit(monkeypatch):
    """the optimizer's host logic over the f32 restatement of the kernels: as it is, inside adamw_check's limit for p, m and v at every step of
    SCHEDULE; with the step number advanced on dropped steps too (the optimizer before the count moved to the device), at least 10 x outside the
    limit on p (the ordinary parameters: four of extreme size, 70000 .. 5e-8, otherwise set the worst-element limit for everyone) at the first
    applied step after each drop"""
    launches = _Launches().install(monkeypatch)
    p0, g, ordinary = case(N)
    ref, f32 = TorchAmpAdamW(p0, F64), TorchAmpAdamW(p0, F32)
    (good, gst, gsc), (faulty, fst, fsc) = _optimizer("FlatAdamW", p0, F32), _optimizer("FlatAdamW", p0, F32)
    worst, outside = 0.0, {}
    for i, (bad, lr, clip, grad_scale) in enumerate(SCHEDULE):
        gs = scaled_grad(g, i, ref.scale, bad)
        ref.step(gs, lr, grad_scale, clip); f32.step(gs, lr, grad_scale, clip)
        launches.count_drops = False
        _take(good, gst, gs, lr, clip, grad_scale)
        launches.count_drops = True
        _take(faulty, fst, gs, lr, clip, grad_scale)
        assert gsc.scale_t.item() == fsc.scale_t.item() == f32.scale == ref.scale and good.state_dict()["step"] == f32.applied == ref.applied
        worst = max(worst, adamw_check((gst.p, gst.m, gst.v), f32, ref, f"the f32 restatement, step {i + 1}", keep=ordinary))
        if i + 1 in FIRST_AFTER_A_DROP:
            outside[i + 1] = _p_ratio(fst.p, f32, ref, ordinary)
    print(f"f32 restatement: worst error / limit {worst:.3f}; step number advanced on dropped steps: error / limit on p at the first applied step "
          f"after a drop {({k: round(v, 1) for k, v in outside.items()})}")
    assert faulty.state_dict()["step"] == len(SCHEDULE) and good.state_dict()["step"] == APPLIED[-1]
    assert all(v >= 10.0 for v in outside.values()), outside


def test_state_dict_carries_the_scaler_and_old_checkpoints_still_load():
    from enhancing.engine.optim import FlatAdamW, LossScaler
    cpu = torch.device("cpu")
    st = _Store(torch.zeros(8), F32)
    st.loss_scaler = LossScaler(cpu, init_scale=512.0, growth_interval=3, enabled=True)
    opt = FlatAdamW(st, lr=1e-3)
    st.loss_scaler.tracker.fill_(2)
    sd = opt.state_dict()
    assert sorted(sd) == ["m", "param_groups", "scaler", "step", "v"] and sd["scaler"]["scale"].item() == 512.0 and int(sd["scaler"]["tracker"]) == 2
    assert sd["scaler"]["skipped_steps"] is None          # (the store's scaler keeps no count of the drops)
    st2 = _Store(torch.zeros(8), F32)
    st2.loss_scaler = LossScaler(cpu, init_scale=4096.0, growth_interval=3, enabled=True)
    opt2 = FlatAdamW(st2, lr=1e-3)
    opt2.load_state_dict(sd)
    assert st2.loss_scaler.scale_t.item() == 512.0 and int(st2.loss_scaler.tracker) == 2
    old = {k: v for k, v in sd.items() if k != "scaler"}      # a checkpoint from before the scaler was saved
    st2.loss_scaler.scale_t.fill_(64.0)
    opt2.load_state_dict(dict(old, step=7))
    assert st2.step_count == 7 and st2.loss_scaler.scale_t.item() == 64.0
    st.loss_scaler.enabled = False
    assert "scaler" not in opt.state_dict()
