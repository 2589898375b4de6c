"""sample(graph=True) of both stage-2 priors (position 0 eagerly, then ONE captured position replayed T - 1 times) against
sample(graph=False) on the same module, seed and inputs: the codes are equal and the logits are equal as int32 bits.  The loop itself is held to
the reference's goldens by tests/test_gpt_sample_gpu.py and tests/test_rq_sample_gpu.py; here the draws are free (every position is fed the codes the
position before it drew, on the device), so a wrong row, slot or step of a replay changes everything behind it."""
import pytest
import torch

import gpt_cases as GC
import rq_sample_cases as SC

pytestmark = pytest.mark.gpu

MODES = ["fp16", "bf16", "exact"]


def _load(m, make_params, seed=None):
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    P = make_params(shapes) if seed is None else make_params(shapes, seed=seed)
    m.load_state_dict(P, strict=True)
    return m.cuda(), P


def _gpt(name="tiny", **over):
    from enhancing.modules.stage2.layers import GPT
    m, _ = _load(GPT(**dict(GC.case_kwargs(name), **over)), GC.make_params)
    return m, GC.make_inputs(name)[0].cuda()


def _rq(name="rq_tiny", **over):
    from enhancing.modules.stage2.layers import RQTransformer
    m, _ = _load(RQTransformer(**dict(SC.case_kwargs(name), **over)), SC.make_params)
    return m, SC.case_inputs(name)[0].cuda()


PRIORS = {"gpt": _gpt, "rq": _rq}


def _mode(monkeypatch, mode) -> dict:
    if mode == "exact":
        return dict(use_fp16=False)
    monkeypatch.setenv("ENH_PRECISION", mode)
    return dict(use_fp16=True)


def _both(m, conds, captured=True, **kw):
    """(logits, codes) of graph=True after checking them against graph=False; captured: the call must have captured one graph per chunk"""
    le, ce = m.sample(conds, graph=False, **kw)
    m._sample_keep = None
    lg, cg = m.sample(conds, graph=True, **kw)
    assert cg.dtype == torch.int64 and cg.shape == ce.shape and torch.equal(ce, cg), "codes differ"
    assert (le is None) == (lg is None)
    if le is not None:
        assert lg.shape == le.shape and torch.equal(le.view(torch.int32), lg.view(torch.int32)), "logits differ"
    if captured:
        chunks = (conds.shape[0] + 63) // 64
        assert m._sample_keep is not None and len(m._sample_keep[0]) == chunks, "graph=True did not capture one graph per chunk"
    else:
        assert m._sample_keep is None or not m._sample_keep[0]
    return lg, cg


# ---- the cases of the goldens, every mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,over", [("tiny", {}), ("hs384", {}), ("tiny", dict(img_num_tokens=70))], ids=["tiny", "hs384", "tiny_t70"])
def test_gpt_graph_equals_the_loop(name, over, mode, monkeypatch):
    """tiny_t70 crosses the 64-slot boundary of the decode attention's plan: nsplit goes 1 -> 2 inside the replays"""
    m, conds = _gpt(name, **over)
    logits, codes = _both(m, conds, seed=4, **_mode(monkeypatch, mode))
    T, V = m.img_num_tokens, m.vocab_img_size
    assert tuple(codes.shape) == (conds.shape[0], T) and tuple(logits.shape) == (conds.shape[0], T * V)
    assert int(codes.min()) >= 0 and int(codes.max()) < V and bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_rq_graph_equals_the_loop(name, mode, monkeypatch):
    m, conds = _rq(name)
    logits, codes = _both(m, conds, seed=4, **_mode(monkeypatch, mode))
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    assert tuple(codes.shape) == (B, T, D) and tuple(logits.shape) == (B * T, D, V)
    assert int(codes.min()) >= 0 and int(codes.max()) < V and bool(torch.isfinite(logits).all())


@pytest.mark.parametrize("mode", MODES)
def test_rq_graph_with_the_reference_s_second_ln_depth(mode, monkeypatch):
    m, conds = _rq("rq_tiny")
    twice, _ = _both(m, conds, seed=4, slot0_ln="twice", **_mode(monkeypatch, mode))
    once, _ = m.sample(conds, seed=4, graph=True, **_mode(monkeypatch, mode))
    assert not torch.equal(once, twice)


@pytest.mark.parametrize("mode", MODES)
def test_rq_graph_under_the_depth_decode_switch(mode, monkeypatch):
    """ENH_RQ_DEPTH_DECODE=cache: enh_decode_attention at its constant slot d inside the captured position"""
    from enhancing import _C
    monkeypatch.setenv("ENH_RQ_DEPTH_DECODE", "cache")
    calls = []
    monkeypatch.setattr(_C, "short_decode_attention", lambda *a, **k: calls.append(1))
    m, conds = _rq("rq_d3")
    _both(m, conds, seed=4, **_mode(monkeypatch, mode))
    assert not calls


# ---- once per prior -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", list(PRIORS))
def test_filters_forced_codes_and_no_logits(prior):
    m, conds = PRIORS[prior]()
    kw = dict(top_k=50, top_p=0.9, softmax_temperature=0.8)
    logits, codes = _both(m, conds, seed=7, **kw)
    assert bool((torch.isfinite(logits.view(-1, m.vocab_img_size)).sum(-1) == 50).all()), "the logits are after the top-k mask"
    forced = torch.randint(0, m.vocab_img_size, codes.shape, device="cuda")
    lf, cf = _both(m, conds, seed=7, forced_codes=forced, **kw)
    assert not torch.equal(lf, logits)
    none, cn = _both(m, conds, seed=7, return_logits=False, **kw)
    assert none is None and torch.equal(cn, codes)


@pytest.mark.parametrize("prior", list(PRIORS))
def test_two_chunks_with_a_row_offset(prior):
    """66 rows of a T = 3 model: a chunk of 64 and one of 2, each with its own graph; the rows number from row_offset"""
    m, _ = PRIORS[prior](img_num_tokens=3)
    conds = (torch.arange(66) % 10).view(66, 1).cuda()
    logits, codes = _both(m, conds, seed=5, top_k=40, row_offset=9)
    _, shifted = m.sample(conds, seed=5, top_k=40, row_offset=10, graph=True)
    assert not torch.equal(codes, shifted)
    tail_l, tail_c = m.sample(conds[64:], seed=5, top_k=40, row_offset=9 + 64, graph=True)
    assert torch.equal(tail_c, codes[64:]) and torch.equal(tail_l.view(2, -1).view(torch.int32), logits.view(66, -1)[64:].view(torch.int32))


@pytest.mark.parametrize("prior", list(PRIORS))
def test_seeds(prior):
    m, conds = PRIORS[prior]()
    l1, c1 = _both(m, conds, seed=5)
    l2, c2 = m.sample(conds, seed=5, graph=True)
    assert torch.equal(c1, c2) and torch.equal(l1.view(torch.int32), l2.view(torch.int32)), "two calls with one seed"
    _, c3 = _both(m, conds, seed=6)
    assert not torch.equal(c1, c3)


@pytest.mark.parametrize("prior", list(PRIORS))
def test_load_state_dict_between_two_graph_calls(prior):
    m, conds = PRIORS[prior]()
    la, ca = m.sample(conds, seed=3, graph=True)
    make = GC.make_params if prior == "gpt" else SC.make_params
    P2 = make({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=GC.PARAM_SEED + 1)
    m.load_state_dict(P2)
    lb, cb = _both(m, conds, seed=3)
    assert not torch.equal(la, lb), "the second call still ran the old weights"


@pytest.mark.parametrize("prior", list(PRIORS))
def test_an_optimizer_step_between_two_graph_calls(prior, monkeypatch):
    """under a GPTAdam the operands are views into its arena, which the step kernel rewrites in place: nothing captured may outlive a call"""
    from enhancing.engine.optim import GPTAdam
    monkeypatch.setenv("ENH_PRECISION", "bf16")
    m, conds = PRIORS[prior]()
    opt = GPTAdam(m, lr=1e-2)
    la, ca = _both(m, conds, seed=3)
    m.forward_backward(ca, conds)
    opt.step()
    lb, cb = _both(m, conds, seed=3)
    assert not torch.equal(la, lb), "the second call still ran the weights from before the step"


@pytest.mark.parametrize("prior", list(PRIORS))
def test_a_model_of_one_position(prior):
    """T == 1: position 0 only, nothing is captured"""
    m, conds = PRIORS[prior](img_num_tokens=1)
    _, codes = _both(m, conds, captured=False, seed=2)
    assert codes.shape[1] == 1


@pytest.mark.parametrize("prior", list(PRIORS))
def test_per_kernel_timing_runs_the_loop(prior, monkeypatch):
    from enhancing import _C
    m, conds = PRIORS[prior]()
    want = m.sample(conds, seed=2, graph=False)
    monkeypatch.setattr(_C, "TIMER", _C.KernelTimer())
    _both(m, conds, captured=False, seed=2)
    assert any("gpt_skinny_gemm_kernel" in k for k in _C.TIMER.records), "the timed call launched nothing the timer saw"
    monkeypatch.setattr(_C, "TIMER", None)
    got = m.sample(conds, seed=2, graph=True)
    assert torch.equal(got[1], want[1])


# ---- the replay is a replay -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior", list(PRIORS))
def test_host_launches_do_not_grow_with_the_positions(prior, monkeypatch):
    """Python-level calls of _C.skinny_gemm: with graph=True position 0 plus ONE captured position whatever T is; the loop's grow with T"""
    from enhancing import _C
    monkeypatch.setenv("ENH_PRECISION", "fp16")
    real, calls = _C.skinny_gemm, []
    monkeypatch.setattr(_C, "skinny_gemm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    counts = {}
    for T in (20, 70):
        m, conds = PRIORS[prior](img_num_tokens=T)
        for graph in (True, False):
            del calls[:]
            m.sample(conds, seed=1, graph=graph)
            counts[(T, graph)] = len(calls)
    per_position = counts[(20, False)] // 20
    assert counts[(20, False)] == 20 * per_position and counts[(70, False)] == 70 * per_position
    assert counts[(20, True)] == counts[(70, True)] == 2 * per_position, counts
