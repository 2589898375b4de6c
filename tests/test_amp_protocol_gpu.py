"""The two stage-1 optimizers through a schedule of dropped steps, growths and changing learning rates, clips and accumulation factors
(tests/amp_protocol_util.py SCHEDULE) against torch.amp.GradScaler + torch.optim.AdamW on the CPU: FlatAdamW over a small fp32 ParamStore with a
LossScaler, FusedAdamW through the tiny fp16 engine (the plain road and the unscale_grads() road), the bf16 engine (no scaler: the step by value,
bit for bit), and a resume from state_dict() in the middle of the schedule for both.

Limit: step_helpers_util.adamw_check — 4 x the error of the f32 torch run + one ulp, per tensor (2-norm) and on the worst element, both against the
fp64 torch run, for p, m and v after EVERY step; scale, growth tracker, applied-step count, found-inf flag and dropped-step count are equalities;
a dropped step and a resumed run are bit equalities.  tests/test_amp_protocol_cpu.py shows that a step number which also counts dropped steps lands
178 - 4800 x outside this limit at the first update after a drop.

Measured on MI355X, the largest error / limit over the 16 steps (test_zz_report prints them; reported, not tolerances): FlatAdamW 0.993, FusedAdamW
0.509.  FlatAdamW per step: 0.000 0.210 0.210 0.210 0.304 0.180 0.180 0.286 0.509 0.879 0.879 0.734 0.822 0.993 0.209 0.290.  The f32 restatement of
tests/test_amp_protocol_cpu.py on the same case has its worst figure (0.879, step 10) on m of the one element whose gradient is 1e3: that element
is all of m's norm, torch's f32 run lands within 0.05 ulp of fp64 on it and the restatement within 1.05 ulp, so norm and worst-element limit are
both about one ulp of a single number there."""
import pytest
import torch

from amp_protocol_util import (APPLIED, BAD_INDEX, BETAS, EPS, GROWTH_INTERVAL, INIT_SCALE, SCALES, SCHEDULE, TRACKERS, WD, TorchAmpAdamW, case, clip_fields,
                               scaled_grad)
from step_helpers_util import F16, F32, F64, adamw_check, bits_equal
from test_grad_clip_gpu import _Net, _build

pytestmark = pytest.mark.gpu

RESUME_AT = [7, 13]      # steps taken before the checkpoint: 7 = directly after a dropped step (tracker 0), 13 = a clean run of two (tracker 2: step 14 grows)
WORST = {}


class _Snap:
    """p, m, v of a torch run after one step, in the shape adamw_check reads"""

    def __init__(self, r):
        self._p, self._m, self._v = r.p().clone(), r.m().clone(), r.v().clone()

    def p(self):
        return self._p

    def m(self):
        return self._m

    def v(self):
        return self._v


_REFS = {}


def reference(key: str, p0, g):
    """the f32 and the fp64 torch run over SCHEDULE from p0 on base gradient g, computed once per key -> [(f32 snapshot, fp64 snapshot)] per step.
    Their applied count, scale and tracker are held to the hand-written lists here, so every test compares with those."""
    if key not in _REFS:
        f32, ref, out = TorchAmpAdamW(p0, F32), TorchAmpAdamW(p0, F64), []
        for (i, _, a), (_, _, b) in zip(f32.run(g), ref.run(g)):
            assert (a.applied, a.scale, a.tracker) == (b.applied, b.scale, b.tracker) == (APPLIED[i], SCALES[i], TRACKERS[i])
            out.append((_Snap(a), _Snap(b)))
        _REFS[key] = out
    return _REFS[key]


def _state(store, sc, eng=None):
    """everything a step may change, cloned on the device"""
    return dict(p=store.p.clone(), m=store.m.clone(), v=store.v.clone(), p16=store.p16.clone() if eng is not None else None, scale=sc.scale_t.item(),
                tracker=int(sc.tracker), applied=store.step_count, found_inf=float(sc.found_inf), skipped=None if eng is None else eng.skipped_steps.item())


def _run(opt, store, sc, g, steps, eng=None, unscale_first: bool = False):
    """steps `steps` (0-based indices) of SCHEDULE through opt.step(), the scaled gradient written into the store's flat gradient -> [state] per step"""
    out = []
    for i in steps:
        bad, lr, clip, grad_scale = SCHEDULE[i]
        store.zero_grad()
        store.g.copy_(scaled_grad(g, i, sc.scale_t.item(), bad))
        opt.param_groups[0]["lr"], opt.grad_scale = lr, grad_scale
        opt.gradient_clip_val, opt.gradient_clip_algorithm = clip_fields(clip)
        if unscale_first and not bad:
            eng.unscale_grads()
        opt.step()
        out.append(_state(store, sc, eng))
    torch.cuda.synchronize()
    return out


def _hold_to_reference(states, initial, refs, what: str, p16_dtype=None):
    ratios, drops, prev = [], 0, initial
    for i, (st, (f32, ref)) in enumerate(zip(states, refs)):
        bad, w = SCHEDULE[i][0], f"{what} step {i + 1}"
        drops += bool(bad)
        ratios.append(adamw_check((st["p"], st["m"], st["v"]), f32, ref, w))
        assert (st["scale"], st["tracker"], st["applied"]) == (SCALES[i], TRACKERS[i], APPLIED[i]), f"{w}: scale, tracker, applied steps {st}"
        assert st["found_inf"] == float(bool(bad)), w
        if bad:
            assert all(bits_equal(st[k], prev[k]) for k in ("p", "m", "v")), f"{w}: a dropped step wrote"
        else:
            assert not torch.equal(st["p"], prev["p"]), f"{w}: a clean step left p alone"
        if p16_dtype is not None:
            assert bits_equal(st["p16"], st["p"].to(p16_dtype)), f"{w}: the 16-bit shadow is not the rounded p"
            assert not bad or bits_equal(st["p16"], prev["p16"]), f"{w}: a dropped step wrote the 16-bit shadow"
            assert st["skipped"] == float(drops), f"{w}: skipped_steps {st['skipped']}, drops so far {drops}"
        prev = st
    print(f"{what}: error / limit per step " + " ".join(f"{r:.3f}" for r in ratios))
    return max(ratios)


def _same_bits(a, b, what: str):
    scalars = ("scale", "tracker", "applied", "found_inf", "skipped")
    for k in ("p", "m", "v", "p16"):
        assert (a[k] is None and b[k] is None) or bits_equal(a[k], b[k]), f"{what}: {k} differs"
    assert all(a[k] == b[k] for k in scalars), (what, {k: (a[k], b[k]) for k in scalars})


# ---- FlatAdamW ---------------------------------------------------------------------------------------------------------------------------------------
def _flat():
    from enhancing.engine.optim import FlatAdamW, LossScaler
    from enhancing.engine.stage1 import ParamStore
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    store = ParamStore(_Net(), dev, precision="fp32")      # 37 -> 129 -> 3: segment sizes that are no multiple of 4
    sc = store.loss_scaler = LossScaler(dev, init_scale=INIT_SCALE, growth_interval=GROWTH_INTERVAL, enabled=True)
    return FlatAdamW(store, lr=1.0, betas=BETAS, eps=EPS, weight_decay=WD), store, sc


@pytest.fixture(scope="module")
def flat_run():
    """the uninterrupted run of SCHEDULE through FlatAdamW -> (initial state, [state per step], base gradient)"""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    opt, store, sc = _flat()
    g = case(store.numel)[1]
    initial = _state(store, sc)
    return initial, _run(opt, store, sc, g, range(len(SCHEDULE))), g


def test_flat_adamw_follows_gradscaler_and_adamw(flat_run):
    initial, states, g = flat_run
    assert initial["p"].numel() >= 5292 and initial["applied"] == 0
    WORST["FlatAdamW"] = _hold_to_reference(states, initial, reference("flat", initial["p"].cpu(), g), "FlatAdamW")
    print(f"FlatAdamW over SCHEDULE: worst error / limit {WORST['FlatAdamW']:.3f}")


@pytest.mark.parametrize("k", RESUME_AT)
def test_flat_adamw_resumes_from_its_state_dict(flat_run, k):
    initial, states, g = flat_run
    opt, store, sc = _flat()
    _run(opt, store, sc, g, range(k))
    sd = opt.state_dict()
    assert sd["step"] == APPLIED[k - 1] and sd["scaler"]["scale"].item() == SCALES[k - 1] and int(sd["scaler"]["tracker"]) == TRACKERS[k - 1]
    opt2, store2, sc2 = _flat()
    assert bits_equal(store2.p, initial["p"]), "a fresh store starts from the same weights"
    store2.p.copy_(store.p)
    opt2.load_state_dict(sd)
    assert store2.step_count == APPLIED[k - 1]
    for i, st in zip(range(k, len(SCHEDULE)), _run(opt2, store2, sc2, g, range(k, len(SCHEDULE)))):
        _same_bits(st, states[i], f"FlatAdamW resumed after step {k}, step {i + 1}")


# ---- FusedAdamW through the tiny engine --------------------------------------------------------------------------------------------------------------
def _engine(precision: str = "fp16"):
    """the tiny engine with GradScaler's interval at 3 -> (model, engine, optimizer)"""
    import vitvq_oracle as O
    from enhancing.engine.optim import FusedAdamW
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ENH_LOSS_SCALE_INTERVAL", str(GROWTH_INTERVAL))
        mp.delenv("ENH_LOSS_SCALE", raising=False)
        mp.delenv("ENH_NONFINITE_CHECK", raising=False)
        m = _build(O.TINY_CFG, O.make_params(O.TINY_CFG, 21), precision)
        eng = m.engine
    return m, eng, FusedAdamW(eng, lr=1.0, betas=BETAS, eps=EPS, weight_decay=WD)


def _engine_grad(store):
    """_adamw_case's gradient over the engine's flat buffer, zero in the padding between the parameters (p, m and v stay zero there, so a model
    state_dict carries all of p), its 1e3 element on the last parameter element"""
    g = case(store.numel)[1]
    live = torch.zeros(store.numel, dtype=torch.bool)
    for off, cnt, _ in store.offsets.values():
        live[off:off + cnt] = True
    g = g * live
    g[int(live.nonzero().max())] = 1e3
    assert bool(live[BAD_INDEX % store.numel])
    return g


@pytest.fixture(scope="module")
def engine_run():
    """the uninterrupted run of SCHEDULE through the fp16 engine's FusedAdamW -> (initial state, [state per step], base gradient)"""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    m, eng, opt = _engine()
    sc = eng.scaler
    assert sc.scale_t.item() == INIT_SCALE and sc.growth_interval == GROWTH_INTERVAL and eng.store.step_state is not None
    g = _engine_grad(eng.store)
    initial = _state(eng.store, sc, eng)
    return initial, _run(opt, eng.store, sc, g, range(len(SCHEDULE)), eng), g


def test_fused_adamw_follows_gradscaler_and_adamw(engine_run):
    initial, states, g = engine_run
    for i, (bad, lr, clip, grad_scale) in enumerate(SCHEDULE):
        if clip is not None and clip[0] == "norm":
            assert (scaled_grad(g, i, 1.0, None).double() * grad_scale).norm().item() > 2 * clip[1], "the norm clip bites"
    WORST["FusedAdamW"] = _hold_to_reference(states, initial, reference("engine", initial["p"].cpu(), g), "FusedAdamW (fp16 engine)", p16_dtype=F16)
    print(f"FusedAdamW over SCHEDULE: worst error / limit {WORST['FusedAdamW']:.3f}")


def test_fused_adamw_after_unscale_grads_gives_the_same_bits(engine_run):
    """every good step calls eng.unscale_grads() first (Stage1Engine's grads_unscaled road: the division by the scale happens in a pass of its own,
    the launches lose the loss_scale operand): the scale is a power of two, so p, m, v and the shadow are the first pass's bit for bit"""
    initial, states, g = engine_run
    m, eng, opt = _engine()
    for i, st in enumerate(_run(opt, eng.store, eng.scaler, g, range(len(SCHEDULE)), eng, unscale_first=True)):
        _same_bits(st, states[i], f"unscale_grads() road, step {i + 1}")


@pytest.mark.parametrize("k", RESUME_AT)
def test_fused_adamw_resumes_from_its_state_dict(engine_run, k):
    initial, states, g = engine_run
    m, eng, opt = _engine()
    _run(opt, eng.store, eng.scaler, g, range(k), eng)
    sd, weights = opt.state_dict(), {n: t.detach().cpu().clone() for n, t in m.state_dict().items()}
    assert sd["step"] == APPLIED[k - 1] and sd["scaler"]["scale"].item() == SCALES[k - 1] and int(sd["scaler"]["tracker"]) == TRACKERS[k - 1]
    assert sd["scaler"]["skipped_steps"].item() == float(sum(bool(r[0]) for r in SCHEDULE[:k]))
    m2, eng2, opt2 = _engine()
    assert bits_equal(eng2.store.p, initial["p"]), "a fresh engine starts from the same weights"
    m2.load_state_dict(weights, strict=True)      # (rebuilds the fp16 shadow from the masters)
    opt2.load_state_dict(sd)
    _same_bits(_state(eng2.store, eng2.scaler, eng2), dict(states[k - 1], found_inf=0.0), f"restored after step {k}")
    for i, st in zip(range(k, len(SCHEDULE)), _run(opt2, eng2.store, eng2.scaler, g, range(k, len(SCHEDULE)), eng2)):
        _same_bits(st, states[i], f"FusedAdamW resumed after step {k}, step {i + 1}")


def test_bf16_engine_takes_the_step_by_value():
    """no scaler under bf16: the schedule without its bad steps is the plain launch with step = 1, 2, ... handed over by value, bit for bit"""
    from enhancing import _C
    m, eng, opt = _engine("bf16")
    s = eng.store
    assert eng.scaler is None and s.step_state is None
    g = _engine_grad(s)
    p, mm, v, p16 = (t.clone() for t in (s.p, s.m, s.v, s.p16))
    out, t = torch.zeros(2, device=s.p.device), 0
    for i, (bad, lr, clip, grad_scale) in enumerate(SCHEDULE):
        if bad:
            continue
        t += 1
        gd = scaled_grad(g, i, 1.0, None).to(s.p.device)
        s.zero_grad()
        s.g.copy_(gd)
        opt.param_groups[0]["lr"], opt.grad_scale = lr, grad_scale
        opt.gradient_clip_val, opt.gradient_clip_algorithm = clip_fields(clip)
        opt.step()
        kw = {}
        if clip is not None and clip[0] == "norm":
            _C.grad_clip_coef(gd, clip[1], grad_scale, out)
            kw["clip_coef"] = out[1:]
        elif clip is not None:
            kw["clip_value"] = clip[1]
        _C.adamw_step(p, gd, mm, v, p16, t, lr, BETAS[0], BETAS[1], EPS, WD, grad_scale, **kw)
        assert all(bits_equal(a, b) for a, b in zip((s.p, s.m, s.v, s.p16), (p, mm, v, p16))), f"bf16 engine, applied step {t}"
        assert s.step_count == t and s.step_state is None
    assert t == APPLIED[-1] and opt.state_dict()["step"] == t and "scaler" not in opt.state_dict()


def test_zz_report():
    print("stage-1 optimizers over SCHEDULE, worst error / limit (4 x torch's f32 error + one ulp; p, m, v; per tensor and worst element): "
          + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
