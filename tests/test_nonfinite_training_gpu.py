"""The loop the kernels of tests/test_nonfinite_*_kernels_gpu.py serve: fp16 training started at a loss scale far too high (2^30).

Every step either overflows somewhere in the scaled backward — then the flat gradient must hold an inf or NaN, the step is dropped (parameters,
moments, the 16-bit shadow / arena and the step count keep their bits) and the scale halves — or it is applied.  (The scaler keeps its scale inside
[1, 2^24]: the first dropped step takes the hand-set 2^30 onto that ceiling, every later one halves it; _after_drops.)  Dropped steps write nothing, so the
FIRST APPLIED step computes the gradient at the initial weights, at the largest scale that did not overflow: its intermediates sit closest to 65504,
and an overflow that a kernel swallowed or saturated on the way shows here as a wrong gradient.  That gradient, unscaled, is held to the reference and
limit the project already has for those weights:

  stage 1 (vitvq_oracle.TINY_CFG)  vitvq_oracle.train_step_grads, 5e-3 per parameter (tests/test_fp16_gpu.py, the step after its dropped step)
  GPT "tiny", RQ "rq_tiny"         the fp64 restatements behind the gpt_bwd_tiny / rq_bwd_rq_tiny goldens with the limits of
                                   tests/test_gpt_backward_gpu.py / tests/test_rq_backward_gpu.py: at most twice the emulation's error (the same
                                   restatement with the device's rounding points, at the scale reached) plus the format's floor; worst row at most twice"""
import pytest
import torch

from nonfinite_util import scrub_shared_buffers  # noqa: F401  (an autouse fixture)
from util import floor16, rel, row_err

pytestmark = pytest.mark.gpu

START = 2.0 ** 30
CEILING = 2.0 ** 24          # enh_loss_scale_update keeps the scale inside [1, 2^24] (csrc/elementwise.hip loss_scale_update_kernel)
MAX_STEPS = 32


def _after_drops(n: int) -> float:
    """the scale after n dropped steps from START: every drop halves it, and every update clamps it to the scaler's ceiling — the first drop of a
    scale set by hand above the ceiling lands ON the ceiling (2^30 -> 2^24), each later one halves"""
    s = START
    for _ in range(n):
        s = min(s * 0.5, CEILING)
    return s


def _bits(ts):
    return [t.detach().clone().contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) for t in ts]


def test_stage1_fp16_engine_from_a_scale_far_too_high():
    import vitvq_oracle as O
    from test_fp16_gpu import _build16
    cfg = O.TINY_CFG
    P = O.make_params(cfg, 21)
    m = _build16(cfg, P)
    eng = m.engine
    x = O.make_images(30, 2, cfg["image_size"])
    _, _, o_grads, _ = O.train_step_grads(x, P, cfg)
    eng.scale_t.fill_(START)
    state = lambda: _bits([eng.store.p, eng.store.m, eng.store.v, eng.store.p16])
    dropped = applied = 0
    for step in range(MAX_STEPS):
        scale = eng.loss_scale
        assert scale == _after_drops(dropped)
        eng.forward_backward(x, w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
        finite = bool(torch.isfinite(eng.store.g).all())
        before, count = state(), eng.store.step_count
        if finite:       # the first step that will be applied: the gradient at the initial weights
            eng.unscale_grads()
            errs = {k: rel(p.grad, o_grads[k]) for k, p in m.named_parameters() if k in o_grads}
            worst = max(errs, key=errs.get)
            print(f"stage 1: first applied step at scale 2^{int(torch.log2(torch.tensor(scale)).item())} after {dropped} dropped; "
                  f"worst gradient rel error vs the fp32 oracle {errs[worst]:.2e} ({worst})")
            assert set(errs) == set(o_grads) and errs[worst] <= 5e-3, (worst, errs[worst])
        eng.optimizer_step(1e-3)
        torch.cuda.synchronize()
        if eng.skipped_steps.item() == dropped + 1:
            assert not finite, "a step with a finite gradient was dropped"
            dropped += 1
            assert all(torch.equal(a, b) for a, b in zip(before, state())), f"the dropped step {step} wrote something"
            assert eng.store.step_count == count and eng.loss_scale == min(scale / 2, CEILING)
        else:
            assert finite, "a step whose flat gradient holds an inf or NaN was applied"
            applied += 1
            assert eng.store.step_count == count + 1 and eng.loss_scale == scale and not torch.equal(before[0], state()[0])
            break
    print(f"stage 1: {dropped} steps dropped, scale reached {eng.loss_scale:g}")
    assert dropped >= 1 and applied == 1 and eng.loss_scale == _after_drops(dropped)


def _prior_from_a_scale_far_too_high(kind, name, monkeypatch):
    from enhancing.engine.optim import GPTAdam
    monkeypatch.setenv("ENH_PRECISION", "fp16")
    if kind == "gpt":
        import test_gpt_backward_gpu as T
        m, P, conds, codes = T._model(name)
        ref = lambda: T._ref(name, P, conds, codes)
        emu = lambda s: T._emu(name, "fp16", s, P, conds, codes)
    else:
        import test_rq_backward_gpu as T
        monkeypatch.delenv("ENH_RQ_DEPTH_ATTN", raising=False)
        m, P, conds, codes = T._model(name, "depth")
        ref = lambda: T._ref(name, "depth", P, conds, codes)
        emu = lambda s: T._emu(name, "depth", "fp16", s, P, conds, codes)
    dt = torch.float16
    opt = GPTAdam(m, lr=1e-3, init_scale=START)
    state = lambda: _bits([opt.p, opt.m, opt.v, opt.state, opt.arena])
    dropped = applied = 0
    for step in range(MAX_STEPS):
        scale = opt.loss_scale.item()
        assert scale == _after_drops(dropped)
        m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
        finite = bool(torch.isfinite(m.flat_grad).all())
        before, count = state(), opt.state_dict()["step"]
        if finite:       # the gradient at the initial weights, at the largest scale that did not overflow
            _, G64, _ = ref()
            _, GE, _ = emu(scale)
            G = T._grads(m)
            assert sorted(G) == sorted(G64)
            qb = {k: G64[k].norm().item() for k in G64 if k.endswith("attn.query.bias")}
            worst, worst_row = (0.0, ""), (0.0, "")
            for k in sorted(G):
                g = G[k]
                got, e, r = g.double().cpu() / scale, GE[k].reshape(g.shape) / scale, G64[k].reshape(g.shape)
                assert bool(torch.isfinite(e).all()), f"{k}: the emulation overflows at the scale the device passed ({scale:g}): it sets no limit"
                if k.endswith("attn.key.bias"):
                    n = qb[k.replace("key", "query")]
                    ek, ee, fl = (got - r).norm().item() / n, (e - r).norm().item() / n, floor16(G64[k.replace("key", "query")], dt)
                else:
                    ek, ee, fl = rel(got, r), rel(e, r), floor16(r, dt)
                worst = max(worst, (ek / (2 * ee + fl), k))
                assert ek <= 2 * ee + fl, (name, k, ek, ee, fl)
                if r.dim() >= 2 and r.numel() > r.shape[-1] and not k.endswith("key.bias"):
                    wk, we = row_err(got, r, r.shape[-1]).max().item(), row_err(e, r, r.shape[-1]).max().item()
                    worst_row = max(worst_row, (wk / we, k))
                    assert wk <= 2 * we, (name, k, "worst row", wk, we)
            print(f"{name}: first applied step at scale 2^{int(torch.log2(torch.tensor(scale)).item())} after {dropped} dropped; worst kernel / (2 emulation "
                  f"+ floor) {worst[0]:.3f} ({worst[1]}); worst row / emulation's worst row {worst_row[0]:.3f} ({worst_row[1]})")
        opt.step()
        torch.cuda.synchronize()
        if opt.state_dict()["step"] == count:
            assert not finite, "a step with a finite gradient was dropped"
            dropped += 1
            assert all(torch.equal(a, b) for a, b in zip(before, state())), f"the dropped step {step} wrote something"
            assert opt.loss_scale.item() == min(scale / 2, CEILING)
        else:
            assert finite, "a step whose flat gradient holds an inf or NaN was applied"
            applied += 1
            assert opt.state_dict()["step"] == count + 1 and opt.loss_scale.item() == scale and not torch.equal(before[0], state()[0])
            break
    print(f"{name}: {dropped} steps dropped, scale reached {opt.loss_scale.item():g}")
    assert dropped >= 1 and applied == 1 and opt.loss_scale.item() == _after_drops(dropped)


def test_gpt_tiny_from_a_scale_far_too_high(monkeypatch):
    _prior_from_a_scale_far_too_high("gpt", "tiny", monkeypatch)


def test_rq_tiny_from_a_scale_far_too_high(monkeypatch):
    _prior_from_a_scale_far_too_high("rq", "rq_tiny", monkeypatch)
