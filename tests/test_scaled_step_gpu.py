"""The one clipped, loss-scaled step under the three optimizers (engine/optim.py scaled_step), on the device: the launches that Stage1Engine.optimizer_step
and GPTAdam.step issue are the rows of the launch table (tests/test_grad_clip_cpu.py holds the whole table on the host; FlatAdamW's rows are
test_flat_adamw_launch_sequence there), recorded here by wrappers that call through to the kernels.  fp16 is the scaler switched on, bf16 is no scaler.
No overflow is provoked: tests/test_fp16_gpu.py, test_grad_clip_gpu.py and test_gpt_train_gpu.py cover the dropped step.

Bound.  A step taken after unscale_grads() differs from the plain step only in where the division by the loss scale happens, and the scale is a power of
two: the parameters are held to the 1e-6 relative bound of the existing one-step checks (test_grad_clip_gpu.py), the scale and the tracker to equality."""
import pytest
import torch

import gpt_backward_cases as BC
from test_grad_clip_gpu import _build, _ref_norm
from util import rel

pytestmark = pytest.mark.gpu

LAUNCHES = ("grad_clip_coef", "nonfinite_flag", "adamw_step", "adam_step_segments", "loss_scale_update")


@pytest.fixture
def rec(monkeypatch):
    """the five launches of a step wrapped by recorders of (name, positional arguments, keywords) that call through"""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    monkeypatch.delenv("ENH_LOSS_SCALE_INTERVAL", raising=False)
    monkeypatch.delenv("ENH_NONFINITE_CHECK", raising=False)
    calls = []

    def wrap(name, fn):
        def recorder(*a, **kw):
            calls.append((name, a, dict(kw)))
            return fn(*a, **kw)
        return recorder
    for name in LAUNCHES:
        monkeypatch.setattr(_C, name, wrap(name, getattr(_C, name)))
    return calls


def _same(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype


def _check_row(calls, adam, g, sc, clip_norm, grad_scale, out, adam_base=(), unscaled=False):
    """calls == the table's row for (scaler `sc` or None, clip by norm `clip_norm` or None, `unscaled` gradients), operand for operand"""
    scale_operand = sc is not None and not unscaled
    first = [] if sc is None and clip_norm is None else ["grad_clip_coef" if clip_norm is not None else "nonfinite_flag"]
    assert [c[0] for c in calls] == first + [adam] + (["loss_scale_update"] if sc is not None else [])
    by_name = {c[0]: c for c in calls}
    if "nonfinite_flag" in by_name:
        a, kw = by_name["nonfinite_flag"][1:]
        assert _same(a[0], g) and a[1] is sc.found_inf and not kw
    if "grad_clip_coef" in by_name:
        a, kw = by_name["grad_clip_coef"][1:]
        assert _same(a[0], g) and a[1] == clip_norm and a[2] == grad_scale and _same(a[3][:1], out) and len(a) == 4
        assert set(kw) == ({"found_inf"} if sc is not None else set()) | ({"loss_scale"} if scale_operand else set())
        assert kw.get("found_inf") is (sc.found_inf if sc is not None else None) and kw.get("loss_scale") is (sc.scale_t if scale_operand else None)
    kw = by_name[adam][2]
    want = set(adam_base) | ({"skip_flag"} if sc is not None else set()) | ({"loss_scale"} if scale_operand else set())
    assert set(kw) == want | ({"clip_coef"} if clip_norm is not None else set()) and all(v is not None for v in kw.values())
    assert kw.get("skip_flag") is (sc.found_inf if sc is not None else None) and kw.get("loss_scale") is (sc.scale_t if scale_operand else None)
    if clip_norm is not None:
        assert kw["clip_coef"].data_ptr() == out.data_ptr() + 4 and kw["clip_coef"].numel() == 1
    if sc is not None:
        a = by_name["loss_scale_update"][1]
        assert a[0] is sc.scale_t and a[1] is sc.found_inf and a[2] is sc.tracker and a[3:] == (2.0, 0.5, 2000)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_engine_step_issues_the_rows_of_the_launch_table(rec, precision):
    import vitvq_oracle as O
    cfg = O.TINY_CFG
    eng = _build(cfg, O.make_params(cfg, 21), precision).engine
    s, sc, lr = eng.store, eng.scaler, 1e-3
    assert (sc is not None) == eng.scaled == (precision == "fp16") and eng.grad_norm is not None, "the engine's grad_norm exists from construction"
    if sc is not None:
        assert eng.scale_t is sc.scale_t and eng.found_inf is sc.found_inf and eng.skipped_steps is sc.skipped_steps and sc.enabled
        assert eng.loss_scale == 65536.0 and sc.growth_interval == 2000
    else:
        assert eng.scale_t is None and eng.found_inf is None and eng.skipped_steps is None and eng.loss_scale == 1.0
    S = eng.loss_scale

    def backward(seed):
        eng.forward_backward(O.make_images(seed, 2, cfg["image_size"]), w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
        del rec[:]

    # no clipping
    backward(30)
    eng.optimizer_step(lr)
    _check_row(rec, "adamw_step", s.g, sc, None, 1.0, eng.grad_norm)
    # clip by norm at half the measured norm
    backward(31)
    clip_norm = 0.5 * _ref_norm(s.g, 0.5, S)
    eng.optimizer_step(lr, grad_scale=0.5, clip_norm=clip_norm)
    _check_row(rec, "adamw_step", s.g, sc, clip_norm, 0.5, eng.grad_norm)
    assert 0.49 < eng._clip_out[1].item() < 0.5
    # after unscale_grads(): no loss_scale operand, the flag and the update still run, and the step is the one the scaled gradient gives
    backward(32)
    state = [t.clone() for t in (s.p, s.m, s.v, s.p16)] + ([sc.scale_t.clone(), sc.tracker.clone()] if sc is not None else [])
    count = s.step_count
    eng.optimizer_step(lr)
    plain = [t.clone() for t in (s.p, s.m, s.v)] + ([sc.scale_t.clone(), sc.tracker.clone()] if sc is not None else [])
    for t, b in zip((s.p, s.m, s.v, s.p16) + ((sc.scale_t, sc.tracker) if sc is not None else ()), state):
        t.copy_(b)
    s.step_count = count
    eng.unscale_grads()
    assert s.grads_unscaled == (sc is not None)
    del rec[:]
    eng.optimizer_step(lr)
    _check_row(rec, "adamw_step", s.g, sc, None, 1.0, eng.grad_norm, unscaled=sc is not None)
    errs = [rel(t, b) for t, b in zip((s.p, s.m, s.v), plain)]
    print(f"{precision}: step after unscale_grads() vs the plain step: p {errs[0]:.1e} m {errs[1]:.1e} v {errs[2]:.1e}")
    assert not torch.equal(s.p, state[0]) and all(e <= 1e-6 for e in errs)
    if sc is not None:
        assert torch.equal(sc.scale_t, plain[3]) and torch.equal(sc.tracker, plain[4]) and eng.skipped_steps.item() == 0.0
        # and clipped: the norm pass carries the flag but not the scale
        del rec[:]
        clip_norm = 0.5 * _ref_norm(s.g, 1.0, 1.0)
        eng.optimizer_step(lr, clip_norm=clip_norm)
        _check_row(rec, "adamw_step", s.g, sc, clip_norm, 1.0, eng.grad_norm, unscaled=True)
        assert 0.49 < eng._clip_out[1].item() < 0.5 and eng.skipped_steps.item() == 0.0 and int(sc.tracker) == 4


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_gpt_adam_step_issues_the_rows_of_the_launch_table(rec, fmt, monkeypatch):
    from enhancing.engine.optim import GPTAdam
    from enhancing.modules.stage2.layers import GPT
    monkeypatch.setenv("ENH_PRECISION", fmt)
    m = GPT(**BC.case_kwargs("tiny"))
    m.load_state_dict(BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=BC.PARAM_SEED), strict=True)
    conds, codes = (t.cuda() for t in BC.case_inputs("tiny"))
    m = m.cuda()
    opt = GPTAdam(m, lr=1e-3, init_scale=1024.0)
    sc = opt.scaler
    assert (sc is not None) == (fmt == "fp16") and opt.loss_scale is (sc.scale_t if sc is not None else None) and opt.grad_norm is None
    base = {"lr", "beta1", "beta2", "eps", "grad_scale"}
    S = 1024.0 if sc is not None else 1.0
    # no clipping: the norm is not asked for, its buffer is not allocated
    m.forward_backward(codes, conds, loss_scale=1.0 if sc is None else opt.loss_scale)
    del rec[:]
    opt.step()
    _check_row(rec, "adam_step_segments", m.flat_grad, sc, None, 1.0, None, adam_base=base)
    assert opt.grad_norm is None
    # clip by norm at half the measured norm
    m.forward_backward(codes, conds, loss_scale=1.0 if sc is None else opt.loss_scale)
    total = _ref_norm(m.flat_grad, 0.5, S)
    opt.grad_scale, opt.gradient_clip_val = 0.5, 0.5 * total
    del rec[:]
    opt.step()
    _check_row(rec, "adam_step_segments", m.flat_grad, sc, 0.5 * total, 0.5, opt.grad_norm, adam_base=base)
    assert abs(opt.grad_norm.item() - total) <= 1e-5 * total and 0.49 < opt._clip_out[1].item() < 0.5
    assert opt.state_dict()["step"] == 2 and (sc is None or (float(sc.found_inf) == 0.0 and int(sc.tracker) == 2 and sc.scale_t.item() == 1024.0))
