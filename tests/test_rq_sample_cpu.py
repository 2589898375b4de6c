"""Stage-2 RQTransformer sampling, host side: the plain-torch restatement of the cached spatial / depth loop that the GPU tests use as their
yardstick (tests/rq_sample_cases.py step_logits) reproduces both goldens of tests/golden/rq_sample_<case>.npz in fp64, the slot-0 quirk and the
two contracts (sampler vs teacher-forced forward) are real differences, and what sampling refuses says so."""
import os

import numpy as np
import pytest
import torch

import rq_cases as RC
import rq_sample_cases as SC
from enhancing.modules.stage2.layers import RQTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"rq_sample_{name}.npz"))
    m = RQTransformer(**SC.case_kwargs(name))
    P = SC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    conds, forced = SC.case_inputs(name)
    assert np.array_equal(conds.numpy(), g["conds"]) and np.array_equal(forced.numpy(), g["forced_codes"])
    return g, m, P, conds, forced


@pytest.mark.parametrize("name", list(SC.CASES))
def test_state_dict_names_and_shapes_equal_the_reference(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"rq_sample_{name}.npz"))
    sd = RQTransformer(**SC.case_kwargs(name)).state_dict()
    assert sorted(sd) == list(g["state_names"])
    for k, shp in zip(g["state_names"], g["state_shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(v) for v in shp if v), k


@pytest.mark.parametrize("name", list(SC.CASES))
def test_fp64_restatement_reproduces_both_goldens(golden_dir, name):
    """the yardstick's own check: the one-row-per-step restatement in fp64 is the reference's cached loop (slot0_ln="twice": its sample_depth_step
    line for line; "once": its submodules with one ln_depth at slot 0) to 1e-9, and the two differ"""
    g, m, P, conds, forced = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    P64 = {k: v.double() for k, v in P.items()}
    got = {}
    for mode in ("once", "twice"):
        got[mode] = SC.step_logits(P64, name, conds, forced, mode, prod=torch.float64, work=torch.float64)
        gold = torch.from_numpy(g[f"logits64_{mode}"])
        assert tuple(got[mode].shape) == tuple(gold.shape) == (B * T, D, V)
        err = (got[mode] - gold).abs().max().item()
        assert err <= 1e-9, (name, mode, err)
        assert float(g[f"ref32_err_{mode}"]) < 1e-4 and tuple(g[f"ref32_err_{mode}_step"].shape) == (T, D)
    diff = (got["once"] - got["twice"]).abs()
    assert diff[:, 0].max().item() > 0.05, "the second ln_depth at slot 0 changes nothing"
    assert diff[:, 1:].max().item() <= 1e-12, "slots d >= 1 do not depend on slot 0's LayerNorm count (forced codes)"


@pytest.mark.parametrize("name", ["rq_tiny", "rq_d3"])
def test_the_sampler_and_the_teacher_forced_forward_are_two_contracts(golden_dir, name):
    """under the cache every Block sees one row (time_shift is zero); the teacher-forced forward on the same codes mixes in the previous row's ln1:
    other logits everywhere except where there is no previous row (position 0's depth slot 0: spatial row 0 and depth row 0 are first rows)"""
    g, m, P, conds, forced = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    P64 = {k: v.double() for k, v in P.items()}
    smp = SC.step_logits(P64, name, conds, forced, "once", prod=torch.float64, work=torch.float64).view(B, T, D, V)
    fwd = RC_forward(P64, name, conds, forced).view(B, T, D, V)
    assert ((smp - fwd).norm() / fwd.norm()).item() > 0.05
    assert (smp[:, 0, 0] - fwd[:, 0, 0]).abs().max().item() <= 1e-9


def RC_forward(P64, name, conds, forced):
    """rq_cases.forward_logits on a case both files share (it reads the shapes from rq_cases.CASES)"""
    assert RC.CASES[name] == SC.CASES[name]
    return RC.forward_logits(P64, name, conds, forced, "depth", prod=torch.float64, work=torch.float64)


def test_refusals_say_why():
    m = RQTransformer(**SC.case_kwargs("rq_tiny"))
    with pytest.raises(NotImplementedError, match="sampling runs on a ROCm device only"):
        m.sample(torch.zeros(1, 1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="sampling runs on a ROCm device only"):
        m.sample(torch.zeros(1, 1, dtype=torch.long), slot0_ln="thrice")      # the device comes first
    from enhancing.modules.stage2.transformer import CondTransformer
    ct = CondTransformer.__new__(CondTransformer)
    torch.nn.Module.__init__(ct)
    ct.transformer, ct.code_shape = m, None
    with pytest.raises(NotImplementedError, match="sampling runs on a ROCm device only"):
        ct.sample(torch.tensor([0, 2]))


def test_library_and_header_carry_the_decode_entries():
    from enhancing import _C
    hdr = open(os.path.join(ROOT, "include", "enh_hip.h")).read()
    L = _C.lib()
    for name in ("enh_rq_embed_step", "enh_short_decode_attention"):
        assert name in _C.SIGNATURES and hasattr(L, name) and f"int {name}(" in hdr, name
    src = open(os.path.join(ROOT, "enhancing-transformers_amd", "csrc", "rq_decode.hip")).read()
    assert src.count("enh_note_kernel_plain(") >= 3 and src.count("return enh_check_launch(") == 2
