"""The yardstick of GPT.forward_backward, checked on the CPU: tests/gpt_backward_cases.py's restatement against gpt_forward_cases.forward_logits,
against torch autograd of its own forward, and against the reference's golden gradients (tests/golden/gpt_bwd_<case>.npz: the reference's GPT in
fp64 with F.cross_entropy(...).backward()); the exported symbols; the refusals that need no device."""
import os

import numpy as np
import pytest
import torch

import gpt_backward_cases as BC
import gpt_forward_cases as FC

_RUNS = {}


def _shapes(name):
    from enhancing.modules.stage2.layers import GPT
    return {k: tuple(v.shape) for k, v in GPT(**BC.case_kwargs(name)).state_dict().items()}


def _run(name):
    """(P, conds, codes, loss, grads, logits) of the fp64 restatement, once per case"""
    if name not in _RUNS:
        P = BC.make_params(_shapes(name))
        conds, codes = BC.case_inputs(name)
        _RUNS[name] = (P, conds, codes) + BC.loss_and_grads(P, BC.case_dims(name), conds, codes)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(FC.CASES))
def test_forward_is_gpt_forward_cases(name):
    P, conds, codes, loss, G, logits = _run(name)
    c2, k2 = FC.case_inputs(name)
    assert torch.equal(c2, conds) and torch.equal(k2, codes)      # the shared cases get the same inputs from both tables
    ref = FC.forward_logits({k: v.double() for k, v in P.items()}, name, conds, codes, rnd=None, prod=torch.float64, work=torch.float64)
    assert (logits - ref).abs().max().item() <= 1e-11 * ref.abs().max().item()


@pytest.mark.parametrize("name", list(BC.CASES))
def test_hand_written_backward_is_autograd_of_the_forward(name):
    P, conds, codes, loss, G, _ = _run(name)
    W = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    _, l2, _ = BC.forward(W, BC.case_dims(name), conds, codes)
    l2.backward()
    assert abs(l2.item() - loss.item()) <= 1e-13 * abs(loss.item())
    qb = G["blocks.0.attn.query.bias"].norm().item()
    for k in sorted(W):
        if k.endswith("attn.key.bias"):      # analytically zero (softmax is shift-invariant): bounded absolutely
            assert G[k].norm().item() <= 1e-10 * qb and W[k].grad.norm().item() <= 1e-10 * qb, k
            continue
        assert (G[k] - W[k].grad).norm().item() <= 1e-10 * W[k].grad.norm().item(), k


@pytest.mark.parametrize("name", list(BC.CASES))
def test_against_the_reference_golden(golden_dir, name):
    P, conds, codes, loss, G, _ = _run(name)
    g = np.load(os.path.join(golden_dir, f"gpt_bwd_{name}.npz"))
    assert np.array_equal(g["conds"], conds.numpy()) and np.array_equal(g["codes"], codes.numpy())
    assert abs(loss.item() - float(g["loss64"])) <= 1e-12 * float(g["loss64"])
    names = [str(k) for k in g["state_names"]]
    assert names == sorted(G)
    qb = np.linalg.norm(g["g.blocks.0.attn.query.bias"])
    for i, k in enumerate(names):
        if k.endswith("attn.key.bias"):
            assert np.linalg.norm(g["g." + k]) <= 1e-12 * qb, k      # the golden's own: zero up to the rounding of fp64 autograd
            assert G[k].norm().item() <= 1e-9 * qb, k
            continue
        if "g." + k in g:
            ref = torch.from_numpy(g["g." + k])
            assert G[k].numel() <= BC.FULL_LIMIT and (G[k] - ref).norm().item() <= 1e-9 * ref.norm().item(), k
            continue
        n, gr, lg = BC.projections(G[k], int(g["proj_seed"]) + i)
        nref = float(g["n." + k])
        assert abs(n.item() - nref) <= 1e-9 * nref, k
        # E ||G r||^2 = ||G||_F^2 for a standard normal r: a projection's error is measured against the gradient's norm, as the norm's is
        assert (gr - torch.from_numpy(g["r." + k])).norm().item() <= 1e-9 * nref, k
        assert (lg - torch.from_numpy(g["l." + k])).norm().item() <= 1e-9 * nref, k


def test_token_rows_that_do_not_occur_are_zero_and_the_last_code_is_not_fed():
    P, conds, codes, loss, G, _ = _run("tiny")
    V, T = BC.CASES["tiny"][3], BC.CASES["tiny"][4]
    fed = torch.zeros(V, dtype=torch.bool)
    fed[codes[:, :T - 1].reshape(-1)] = True
    assert bool((G["tok_emb_code.weight"][~fed] == 0).all()) and bool((G["tok_emb_code.weight"][fed].abs().sum(1) > 0).all())
    assert bool((G["pos_emb_code"][0, T - 1] == 0).all())


def test_library_exports_the_backward_symbols():
    from enhancing import _C
    L = _C.lib()
    for name in ("enh_causal_attention_backward", "enh_cross_entropy_backward", "enh_relu_sq_backward", "enh_ln_timeshift_backward",
                 "enh_gpt_embed_seq_backward"):
        assert name in _C.SIGNATURES and hasattr(L, name), name
    assert hasattr(L, "enh_causal_attention_backward_workspace_bytes") and hasattr(L, "enh_ln_timeshift_backward_workspace_bytes")


def test_forward_backward_refusals_without_a_device():
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**BC.case_kwargs("tiny"))
    conds, codes = BC.case_inputs("tiny")
    with pytest.raises(NotImplementedError, match="device"):
        m.forward_backward(codes, conds)
    with pytest.raises(NotImplementedError, match="exact-f32 backward is not built"):
        m.forward_backward(codes, conds, use_fp16=False)
    assert m.saved_bytes_per_token() == 2 * (28 * 128 + 4 * 2) and m.backward_saved_cap == 16 << 30
