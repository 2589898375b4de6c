"""The host side of sample(cache="fp8"): the yardstick of tests/kv8_cases.py is, with kv=None, the restatement that is pinned to the reference's
goldens, bit for bit; the hook changes what it should; and Prior._sample_cache reads and refuses what it says."""
import pytest
import torch

import gpt_cases as GC
import kv8_cases as KC
import rq_sample_cases as SC
from mxfp8_util import dequant, quant


def _params(cls, kwargs, make):
    return make({k: tuple(v.shape) for k, v in cls(**kwargs).state_dict().items()})


@pytest.mark.parametrize("rounded", [False, True])
def test_without_the_hook_the_gpt_yardstick_is_the_pinned_restatement(rounded):
    from enhancing.modules.stage2.layers import GPT
    name = "tiny"
    P = _params(GPT, GC.case_kwargs(name), GC.make_params)
    conds, forced = GC.make_inputs(name)
    kw = dict(rnd=(lambda t: t.to(torch.float16).to(torch.float32)), prod=torch.float32) if rounded else dict(work=torch.float64)
    a = GC.step_logits(P, name, conds, forced, **kw)
    b = KC.step_logits(P, name, conds, forced, kv=None, **kw)
    bits = torch.int32 if a.dtype == torch.float32 else torch.int64
    assert torch.equal(a.view(bits), b.view(bits))
    c = KC.step_logits(P, name, conds, forced, kv=KC.kv8, **kw)
    assert not torch.equal(a, c) and bool(torch.isfinite(c).all())


@pytest.mark.parametrize("rounded", [False, True])
def test_without_the_hook_the_rq_yardstick_is_the_pinned_restatement(rounded):
    from enhancing.modules.stage2.layers import RQTransformer
    name = "rq_tiny"
    P = _params(RQTransformer, SC.case_kwargs(name), SC.make_params)
    conds, forced = SC.case_inputs(name)
    kw = dict(rnd=(lambda t: t.to(torch.bfloat16).to(torch.float32)), prod=torch.float32) if rounded else dict(work=torch.float64)
    a = SC.step_logits(P, name, conds, forced, "once", **kw)
    b = KC.rq_step_logits(P, name, conds, forced, "once", kv=None, **kw)
    bits = torch.int32 if a.dtype == torch.float32 else torch.int64
    assert torch.equal(a.view(bits), b.view(bits))
    assert not torch.equal(a, KC.rq_step_logits(P, name, conds, forced, "once", kv=KC.kv8, **kw))


def test_only_the_spatial_stack_passes_through_the_rq_hook():
    from enhancing.modules.stage2.layers import RQTransformer
    name = "rq_tiny"
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    P = _params(RQTransformer, SC.case_kwargs(name), SC.make_params)
    conds, forced = SC.case_inputs(name)
    seen = []

    def spy(z):
        seen.append(tuple(z.shape))
        return z

    KC.rq_step_logits(P, name, conds, forced, "once", kv=spy)
    assert seen == [(B, Hs, C // Hs)] * (2 * Ls * T)      # k and v of every spatial layer at every position; no depth step


def test_kv8_is_the_row_quantizer_along_the_head_dimension():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2, 3, 128, generator=g, dtype=torch.float64)
    d = KC.kv8(z)
    assert d.dtype == torch.float64 and d.shape == z.shape
    want = dequant(*quant(z.float().view(6, 128)))
    assert torch.equal(d.float().view(6, 128), want)
    assert torch.equal(KC.kv8(d), d)                        # idempotent: a slot holds the same k / v for every step that reads it
    for dt in (torch.float16, torch.bfloat16):              # a dequantized entry of O(1) rows is a 16-bit value in either format
        assert torch.equal(d.to(dt).double(), d)


def test_sample_cache_reads_the_keyword_then_the_environment(monkeypatch):
    from enhancing.modules.stage2 import prior
    from enhancing.modules.stage2.prior import Prior
    assert prior.SAMPLE_CACHES == ("h16", "fp8")
    monkeypatch.delenv("ENH_SAMPLE_CACHE", raising=False)
    assert Prior._sample_cache(None, True, "t") == "h16"
    assert Prior._sample_cache(None, False, "t") == "h16"
    assert Prior._sample_cache("fp8", True, "t") == "fp8"
    monkeypatch.setenv("ENH_SAMPLE_CACHE", "fp8")
    assert Prior._sample_cache(None, True, "t") == "fp8"
    assert Prior._sample_cache("h16", True, "t") == "h16"      # the keyword wins
    with pytest.raises(ValueError, match="use_fp16"):
        Prior._sample_cache(None, False, "t")
    with pytest.raises(ValueError, match="int4"):
        Prior._sample_cache("int4", True, "t")
    monkeypatch.setenv("ENH_SAMPLE_CACHE", "nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        Prior._sample_cache(None, True, "t")
    monkeypatch.delenv("ENH_SAMPLE_CACHE")
    with pytest.raises(ValueError, match="use_fp16"):
        Prior._sample_cache("fp8", False, "t")
