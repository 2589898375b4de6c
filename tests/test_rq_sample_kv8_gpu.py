"""RQTransformer.sample(cache="fp8"): the spatial stack's k / v caches are MXFP8, the depth caches stay 16-bit.  The rule of
tests/test_gpt_sample_kv8_gpu.py with the RQ yardstick of tests/kv8_cases.py (only the spatial rows pass through the hook): with truth the fp64
logits of that loop and emu the same loop with every operand and cache entry rounded to the format and fp64 products,
rel(got, truth) <= 2 rel(emu, truth) + floor16(truth), over the whole tensor and over every slice of 32 positions.  rq_t70 is the case whose
spatial cache passes 64 slots, so the attention splits and merges.  Device / limit, measured on MI355X (every run prints them), worst of the whole tensor and the three slices: fp16 0.446,
bf16 0.429."""
import pytest
import torch

import kv8_cases as KC
import rq_sample_cases as SC
from util import floor16, rel

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
NAME = "rq_t70"
_TRUTH = {}


def _model():
    from enhancing.modules.stage2.layers import RQTransformer
    m = RQTransformer(**SC.case_kwargs(NAME))
    P = SC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    conds, forced = SC.case_inputs(NAME)
    return m.cuda(), P, conds, forced


def _truth(P, conds, forced):
    if NAME not in _TRUTH:
        _TRUTH[NAME] = (KC.rq_step_logits(P, NAME, conds, forced, "once", work=torch.float64, kv=KC.kv8),
                        SC.step_logits(P, NAME, conds, forced, "once", work=torch.float64))
    return _TRUTH[NAME]


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_rq_fp8_cache_against_the_quantized_cache_model(fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = H16[fmt]
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[NAME]
    m, P, conds, forced = _model()
    truth, plain = (z.view(B, T, D, V) for z in _truth(P, conds, forced))
    emu = KC.rq_step_logits(P, NAME, conds, forced, "once", rnd=lambda t: t.to(dt).to(torch.float32), prod=torch.float64, kv=KC.kv8).view(B, T, D, V)
    # only the spatial cache is quantized: the depth caches of the state are 16-bit tensors
    st = m._decode_state(B, dt, "cuda", cache="fp8")
    assert len(st["spatial"]) == Ls and len(st["depth"]) == Ld
    for kv in st["spatial"]:
        assert [tuple(z.shape) for z in kv] == [(B, Hs, T, C // Hs), (B, Hs, T, C // Hs // 32)] * 2 and all(z.dtype == torch.uint8 for z in kv)
    for kv in st["depth"]:
        assert len(kv) == 2 and all(z.dtype == dt and tuple(z.shape) == (B, Hd, D, C // Hd) for z in kv)
    logits, codes = m.sample(conds.cuda(), forced_codes=forced.cuda(), seed=1, slot0_ln="once", cache="fp8")
    assert tuple(logits.shape) == (B * T, D, V) and tuple(codes.shape) == (B, T, D)
    got = logits.view(B, T, D, V).cpu()
    for sl in [slice(None)] + [slice(t0, t0 + 32) for t0 in range(0, T, 32)]:
        ek, ee, fl = rel(got[:, sl], truth[:, sl]), rel(emu[:, sl], truth[:, sl]), floor16(truth[:, sl], dt)
        print(f"fp8 spatial cache, {fmt} {NAME} positions {sl.start or 0}..: device {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}, "
              f"device / (2 emulation + floor) {ek / (2 * ee + fl):.3f}")
        assert ek <= 2 * ee + fl, (fmt, sl, ek, ee, fl)
    h16 = m.sample(conds.cuda(), forced_codes=forced.cuda(), seed=1, slot0_ln="once")[0].view(B, T, D, V).cpu()
    print(f"{fmt} {NAME}: what the format costs (fp64 with the hook against fp64 without) {rel(truth, plain):.3e}")
    if dt == torch.float16:      # the cache really is the quantized one (under bf16 the format's own rounding is as large as the cache's: no such ordering)
        assert rel(got, truth) < rel(h16, truth) and rel(h16, plain) < rel(got, plain)
    # graph replay: the same bits, logits and codes
    lg, cg = m.sample(conds.cuda(), forced_codes=forced.cuda(), seed=1, slot0_ln="once", cache="fp8", graph=True)
    assert torch.equal(lg.view(torch.int32), logits.view(torch.int32)) and torch.equal(cg, codes)


def test_rq_value_errors():
    m, P, conds, forced = _model()
    with pytest.raises(ValueError, match="use_fp16"):
        m.sample(conds.cuda(), use_fp16=False, cache="fp8")
    with pytest.raises(ValueError, match="int4"):
        m.sample(conds.cuda(), cache="int4")
