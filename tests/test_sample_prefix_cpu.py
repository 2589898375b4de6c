"""The host side of sample(prefix_codes=): the yardstick of tests/prefix_cases.py is, with n_prefix = 0, the restatements that are pinned to the
reference's goldens, bit for bit, and a prefix changes only what it should; the keyword exists on both `sample` signatures and on
CondTransformer.complete; the argument checks that need no device raise before the device is looked at; tools/sample_images.py --complete parses;
the new C entries are declared, bound and exported."""
import inspect
import os
import sys

import pytest
import torch

import gpt_cases as GC
import kv8_cases as KC
import prefix_cases as PC
import rq_sample_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R16 = lambda t: t.to(torch.float16).to(torch.float32)


def _params(cls, kwargs, make):
    return make({k: tuple(v.shape) for k, v in cls(**kwargs).state_dict().items()})


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("rounded", [False, True])
def test_without_a_prefix_the_gpt_yardstick_is_the_pinned_restatement(rounded):
    from enhancing.modules.stage2.layers import GPT
    name = "tiny"
    P = _params(GPT, GC.case_kwargs(name), GC.make_params)
    conds, forced = GC.make_inputs(name)
    assert PC.CASES[name] == GC.CASES[name] and "long" not in GC.CASES and PC.case_kwargs(name) == GC.case_kwargs(name)
    for got, want in zip(PC.case_inputs(name), (conds, forced)):
        assert torch.equal(got, want)
    kw = dict(rnd=R16, prod=torch.float32) if rounded else dict(work=torch.float64)
    a = GC.step_logits(P, name, conds, forced, **kw)
    b = PC.prefix_step_logits(P, name, conds, forced, 0, **kw)
    assert torch.equal(_bits(a), _bits(b))
    c = PC.prefix_step_logits(P, name, conds, forced, 0, kv=KC.kv8, **kw)
    assert torch.equal(_bits(c), _bits(KC.step_logits(P, name, conds, forced, kv=KC.kv8, **kw)))
    # a prefix moves the rounded statement (the numerators' extra rounding) and leaves the unrounded one where it was up to its own rounding
    d = PC.prefix_step_logits(P, name, conds, forced, 7, **kw)
    if rounded:
        assert not torch.equal(a[:, 7:], d[:, 7:]) and float((a - d).abs().max()) < 2e-2
    else:
        assert float((a - d).abs().max()) < 1e-12
    # the given table is the one that is read
    e = PC.prefix_step_logits(P, name, conds, forced, 0, table=GC.CASES, **kw)
    assert torch.equal(_bits(a), _bits(e))


@pytest.mark.parametrize("rounded", [False, True])
def test_without_a_prefix_the_rq_yardstick_is_the_pinned_restatement(rounded):
    from enhancing.modules.stage2.layers import RQTransformer
    name = "rq_tiny"
    P = _params(RQTransformer, SC.case_kwargs(name), SC.make_params)
    conds, forced = SC.case_inputs(name)
    kw = dict(rnd=(lambda t: t.to(torch.bfloat16).to(torch.float32)), prod=torch.float32) if rounded else dict(work=torch.float64)
    for mode in ("once", "twice"):
        a = SC.step_logits(P, name, conds, forced, mode, **kw)
        b = PC.rq_prefix_step_logits(P, name, conds, forced, mode, 0, **kw)
        assert torch.equal(_bits(a), _bits(b))
    c = PC.rq_prefix_step_logits(P, name, conds, forced, "once", 0, kv=KC.kv8, **kw)
    assert torch.equal(_bits(c), _bits(KC.rq_step_logits(P, name, conds, forced, "once", kv=KC.kv8, **kw)))
    d = PC.rq_prefix_step_logits(P, name, conds, forced, "once", 3, **kw)
    a = SC.step_logits(P, name, conds, forced, "once", **kw)
    assert (not torch.equal(a, d)) if rounded else float((a - d).abs().max()) < 1e-12


def test_the_long_case_crosses_a_query_block_and_ends_in_a_ragged_key_tile():
    C, H, L, V, T, B = PC.CASES["long"]
    assert (C, H, L, V, T, B) == (128, 2, 2, 64, 200, 2) and PC.LONG_PREFIX == 150
    assert 128 < PC.LONG_PREFIX < 256 and PC.LONG_PREFIX % 64 and (PC.LONG_PREFIX + 63) // 64 == 3
    conds, forced = PC.case_inputs("long")
    assert tuple(conds.shape) == (B, 1) and tuple(forced.shape) == (B, T) and int(forced.max()) < V


def test_the_keyword_exists_on_both_samplers_and_on_complete():
    from enhancing.modules.stage2.layers import GPT, RQTransformer
    from enhancing.modules.stage2.transformer import CondTransformer
    for cls in (GPT, RQTransformer):
        p = inspect.signature(cls.sample).parameters["prefix_codes"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
        assert "prefix_codes" in cls.sample.__doc__ and "NaN" in cls.sample.__doc__
    sig = inspect.signature(CondTransformer.complete).parameters
    assert list(sig)[:4] == ["self", "images", "conds", "keep"] and sig["keep"].default == 0.5


def test_argument_checks_that_need_no_device_raise_before_the_device_is_looked_at():
    """the models, conds and prefixes are on the CPU: a call that got as far as the device would raise RuntimeError / NotImplementedError instead"""
    from enhancing.modules.stage2.layers import GPT, RQTransformer
    g = GPT(**GC.case_kwargs("tiny"))
    C, H, L, V, T, B = GC.CASES["tiny"]
    conds = torch.zeros(B, 1, dtype=torch.int64)
    ok = torch.zeros(B, 5, dtype=torch.int64)
    for bad, what in ((torch.zeros(B, T, dtype=torch.int64), "left to draw"), (torch.zeros(B, T + 3, dtype=torch.int64), "left to draw"),
                      (torch.full((B, 3), V, dtype=torch.int64), "outside"), (torch.full((B, 3), -1, dtype=torch.int64), "outside"),
                      (torch.zeros(B + 1, 3, dtype=torch.int64), "one row per row"), (torch.zeros((), dtype=torch.int64), "one row per row")):
        with pytest.raises(ValueError, match=what):
            g.sample(conds, prefix_codes=bad)
    with pytest.raises(RuntimeError, match="ROCm device"):      # a good prefix gets as far as the device check
        g.sample(conds, prefix_codes=ok)
    with pytest.raises(RuntimeError, match="ROCm device"):      # so does an empty one
        g.sample(conds, prefix_codes=ok[:, :0])
    assert g._check_prefix(ok[:, :0], B, "t") is None and g._check_prefix(None, B, "t") is None
    got = g._check_prefix(torch.arange(2 * B * 4, dtype=torch.int32).view(B, 2, 4), B, "t")      # [B, h', w], int64-convertible
    assert tuple(got.shape) == (B, 8) and got.dtype == torch.int64 and torch.equal(got.view(-1), torch.arange(2 * B * 4))

    r = RQTransformer(**SC.case_kwargs("rq_tiny"))
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES["rq_tiny"]
    conds = torch.zeros(B, 1, dtype=torch.int64)
    for bad, what in ((torch.zeros(B, 2, D - 1, dtype=torch.int64), "all its codes"), (torch.zeros(B, T, D, dtype=torch.int64), "left to draw"),
                      (torch.full((B, 2, D), V, dtype=torch.int64), "outside"), (torch.zeros(B + 1, 2, D, dtype=torch.int64), "one row per row")):
        with pytest.raises(ValueError, match=what):
            r.sample(conds, prefix_codes=bad)
    with pytest.raises(NotImplementedError, match="ROCm device"):
        r.sample(conds, prefix_codes=torch.zeros(B, 2, D, dtype=torch.int64))
    got = r._check_prefix(torch.zeros(B, 1, 2, D, dtype=torch.int64), B, "t")      # [B, h', w, D]
    assert tuple(got.shape) == (B, 2, D)


def test_sample_images_complete_parses():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sample_images
    ap = sample_images.build_parser()
    a = ap.parse_args(["-c", "x.yaml", "--classes", "1", "2", "--complete", "a.png", "b.png", "--keep", "0.25"])
    assert a.complete == ["a.png", "b.png"] and a.keep == 0.25
    a = ap.parse_args(["-c", "x.yaml", "--classes", "1"])
    assert a.complete is None and a.keep == 0.5
    with pytest.raises(SystemExit):
        ap.parse_args(["-c", "x.yaml", "--classes", "1", "--complete"])


def test_the_fill_entries_are_declared_bound_and_built():
    from enhancing import _C
    hdr = open(os.path.join(ROOT, "include", "enh_hip.h")).read()
    L = _C.lib()
    for name in ("enh_kv_cache_fill", "enh_kv_cache_fill_kv8"):
        assert name in _C.SIGNATURES and hasattr(L, name) and f"int {name}(" in hdr, name
    assert callable(_C.kv_cache_fill) and callable(_C.kv_cache_fill_kv8)
    src = open(os.path.join(ROOT, "enhancing-transformers_amd", "csrc", "gpt_prefill_cache.hip")).read()
    assert src.count("enh_note_kernel") == 2 and src.count("return enh_check_launch(") == 2 and "atomic" not in src.replace("no atomics", "")
    assert '#include "mxfp8.h"' in src and "mx_block_exponent(" in src and "mx_e4m3_rne(" in src      # the append's rounding, shared
