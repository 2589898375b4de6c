"""RQTransformer.sample(prefix_codes=): the batched prefill of the SPATIAL stack against the reference's golden logits of the cached spatial /
depth loop under forced codes (tests/golden/rq_sample_<case>.npz), on the positions t >= P; the logits of the given positions are NaN and
codes[:, :P] is the prefix.  The rules are those of tests/test_rq_sample_gpu.py: exact mode within EXACT_RATIO x the fp32 reference's own error
+ 1e-6; 16-bit modes rel(got, gold) <= 2 rel(emu, gold) + floor16 per (t, d) step and over the steps together, with
emu = prefix_cases.rq_prefix_step_logits(n_prefix = P, rnd = the format).

Measured on MI355X (every test prints its figure).  Exact mode, error / fp32 reference's error (the constant is 4): rq_tiny 1.049 (P = 1) |
0.861 (P = 4) | 0.746 (P = 4, twice), rq_d3 0.989 (P = 1) | 0.774 (P = 6), rq_hs384 0.799 (P = 2); the worst one is 1.049, the figure of the call
without a prefix.  16-bit modes, worst kernel / (2 emulation + floor) over the steps: 0.428 - 0.474 over the six runs and both formats."""
import os

import numpy as np
import pytest
import torch

import prefix_cases as PC
import rq_sample_cases as SC
from test_rq_sample_gpu import EXACT_RATIO
from util import floor16, rel

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
#          case, P, slot0_ln: "once" everywhere, "twice" once
RUNS = [("rq_tiny", 1, "once"), ("rq_tiny", 4, "once"), ("rq_tiny", 4, "twice"), ("rq_d3", 1, "once"), ("rq_d3", 6, "once"), ("rq_hs384", 2, "once")]


def _case(golden_dir, name):
    from enhancing.modules.stage2.layers import RQTransformer
    g = np.load(os.path.join(golden_dir, f"rq_sample_{name}.npz"))
    m = RQTransformer(**SC.case_kwargs(name))
    P = SC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    return m.cuda(), P, torch.from_numpy(g["conds"]).cuda(), torch.from_numpy(g["forced_codes"]).long().cuda(), g


def _bits(t):
    return t.view(torch.int32)


def _prefix_contract(logits, codes, forced, n, shape):
    B, T, D, V = shape
    lg = logits.view(B, T, D, V)
    assert tuple(logits.shape) == (B * T, D, V) and tuple(codes.shape) == (B, T, D) and codes.dtype == torch.int64
    assert bool(torch.isnan(lg[:, :n]).all()) and not bool(torch.isnan(lg[:, n:]).any())
    assert torch.equal(codes[:, :n], forced[:, :n]) and int(codes.min()) >= 0 and int(codes.max()) < V


@pytest.mark.parametrize("name, n, mode", RUNS)
def test_exact_mode_against_the_fp64_golden(golden_dir, name, n, mode):
    m, P, conds, forced, g = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    assert n < T
    logits, codes = m.sample(conds, use_fp16=False, forced_codes=forced, prefix_codes=forced[:, :n], seed=1, slot0_ln=mode)
    _prefix_contract(logits, codes, forced, n, (B, T, D, V))
    gold = torch.from_numpy(g[f"logits64_{mode}"]).view(B, T, D, V)
    err = (logits.view(B, T, D, V)[:, n:].cpu().double() - gold[:, n:]).abs().max().item()
    ref_err = float(g[f"ref32_err_{mode}"])
    print(f"exact {name} P={n} slot0_ln={mode}: max err {err:.3e}, fp32 reference {ref_err:.3e}, ratio {err / ref_err:.3f}")
    assert err <= EXACT_RATIO * ref_err + 1e-6, (name, n, mode, err, ref_err)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name, n, mode", RUNS)
def test_16_bit_modes_against_the_emulation(golden_dir, name, n, mode, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = H16[fmt]
    m, P, conds, forced, g = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    logits, codes = m.sample(conds, forced_codes=forced, prefix_codes=forced[:, :n], seed=1, slot0_ln=mode)
    _prefix_contract(logits, codes, forced, n, (B, T, D, V))
    got = logits.view(B, T, D, V).cpu()
    gold = torch.from_numpy(g[f"logits64_{mode}"]).view(B, T, D, V)
    emu = PC.rq_prefix_step_logits({k: v.cuda() for k, v in P.items()}, name, conds, forced, mode, n, rnd=lambda t: t.to(dt).to(torch.float32),
                                   prod=torch.float64).view(B, T, D, V).cpu()
    worst = 0.0
    for sl in [(slice(None), t, d) for t in range(n, T) for d in range(D)] + [(slice(None), slice(n, T))]:
        ek, ee, fl = rel(got[sl], gold[sl]), rel(emu[sl], gold[sl]), floor16(gold[sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        assert ek <= 2 * ee + fl, (name, n, mode, fmt, sl, ek, ee, fl)
    print(f"{fmt} {name} P={n} slot0_ln={mode}: positions {n}..{T - 1} error {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}; worst kernel / (2 emulation + "
          f"floor) over the steps {worst:.3f}")


@pytest.mark.parametrize("kw", [dict(), dict(cache="fp8", weights="fp8")], ids=["h16", "fp8cache_fp8weights"])
def test_graph_replay_equals_the_loop_with_a_prefix(golden_dir, kw):
    name, n = "rq_tiny", 2
    m, P, conds, forced, g = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    for more in (dict(forced_codes=forced), dict(top_k=20, top_p=0.9)):
        l0, c0 = m.sample(conds, seed=4, prefix_codes=forced[:, :n], graph=False, **kw, **more)
        l1, c1 = m.sample(conds, seed=4, prefix_codes=forced[:, :n], graph=True, **kw, **more)
        assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(c0, c1)
        _prefix_contract(l1, c1, forced, n, (B, T, D, V))
    l2, c2 = m.sample(conds, seed=4, prefix_codes=forced[:, :T - 1], graph=True, **kw)      # nothing is left to replay
    l3, c3 = m.sample(conds, seed=4, prefix_codes=forced[:, :T - 1], graph=False, **kw)
    assert torch.equal(_bits(l2), _bits(l3)) and torch.equal(c2, c3)


def test_the_depth_decode_switch_and_the_given_codes(golden_dir, monkeypatch):
    """ENH_RQ_DEPTH_DECODE=cache composes; a changed code of the prefix moves the logits of position P, wherever the code sits"""
    name, n = "rq_tiny", 3
    m, P, conds, forced, g = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    l0, _ = m.sample(conds, seed=1, prefix_codes=forced[:, :n], forced_codes=forced)
    monkeypatch.setenv("ENH_RQ_DEPTH_DECODE", "cache")
    l1, _ = m.sample(conds, seed=1, prefix_codes=forced[:, :n], forced_codes=forced)
    monkeypatch.delenv("ENH_RQ_DEPTH_DECODE")
    assert rel(l1.view(B, T, D, V)[:, n:], l0.view(B, T, D, V)[:, n:]) < 1e-2
    for pos in (0, n - 1):
        other = forced[:, :n].clone()
        other[:, pos, D - 1] = (other[:, pos, D - 1] + 1) % V
        l2, c2 = m.sample(conds, seed=1, prefix_codes=other)
        l3, _ = m.sample(conds, seed=1, prefix_codes=forced[:, :n])
        assert rel(l2.view(B, T, D, V)[:, n, 0], l3.view(B, T, D, V)[:, n, 0]) > 1e-3 and torch.equal(c2[:, :n], other)


def test_refusals(golden_dir):
    name = "rq_tiny"
    m, P, conds, forced, g = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    with pytest.raises(ValueError, match="all its codes"):
        m.sample(conds, prefix_codes=forced[:, :2, :D - 1])
    with pytest.raises(ValueError, match="left to draw"):
        m.sample(conds, prefix_codes=forced)
    with pytest.raises(ValueError, match="prefix_codes outside"):
        m.sample(conds, prefix_codes=forced[:, :2] + V)
    with pytest.raises(ValueError, match="one row per row"):
        m.sample(conds, prefix_codes=forced[:1, :2])
    other = forced.clone()
    other[0, 1, 0] = (other[0, 1, 0] + 1) % V
    with pytest.raises(ValueError, match="disagree"):
        m.sample(conds, forced_codes=other, prefix_codes=forced[:, :2])
    l0, c0 = m.sample(conds, seed=1, prefix_codes=forced[:, :2].reshape(B, 1, 2, D))      # [B, h', w, D]
    l1, c1 = m.sample(conds, seed=1, prefix_codes=forced[:, :2])
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(c0, c1)
    l2, c2 = m.sample(conds, seed=1, prefix_codes=forced[:, :0])      # an empty prefix is the call without one
    l3, c3 = m.sample(conds, seed=1)
    assert torch.equal(_bits(l2), _bits(l3)) and torch.equal(c2, c3)
