"""The contract of the stage-2 GPT's teacher-forced forward on the CPU: tests/golden/gpt_fwd_<case>.npz (the reference's GPT.forward in fp64,
tools/make_golden_gpt_forward.py) against the plain-torch restatement of tests/gpt_forward_cases.py that the device tests use as their yardstick."""
import os

import numpy as np
import pytest
import torch

import gpt_cases as GC
import gpt_forward_cases as FC

torch.set_num_threads(4)


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"gpt_fwd_{name}.npz"))
    shapes = {str(k): tuple(int(d) for d in s if d) for k, s in zip(g["state_names"], g["state_shapes"])}
    return g, FC.make_params(shapes), torch.from_numpy(g["conds"]), torch.from_numpy(g["codes"]).long()


def test_case_tables_and_inputs_extend_the_sampling_cases():
    for name in GC.CASES:
        assert FC.CASES[name] == GC.CASES[name]
        a, b = GC.make_inputs(name), FC.case_inputs(name)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert FC.CASES["long"] == (128, 2, 1, 64, 200, 2) and FC.CASES["long3"] == (192, 3, 2, 48, 131, 1)


@pytest.mark.parametrize("name", list(FC.CASES))
def test_fp32_restatement_within_the_reference_modules_own_error(golden_dir, name):
    """the restatement builds S = T rows (no row for the last code) and is another summation order of the same fp32 arithmetic: 4 x the fp32
    reference module's own max error + 1e-6, the margin of test_gpt_sample_cpu.py"""
    g, P, conds, codes = _load(golden_dir, name)
    C, H, L, V, T, B = FC.CASES[name]
    gold = torch.from_numpy(g["logits64"])
    assert tuple(gold.shape) == (B, T, V)
    got = FC.forward_logits(P, name, conds, codes, rnd=None, prod=torch.float32, work=torch.float32)
    err, ref_err = (got.double() - gold).abs().max().item(), float(g["ref32_err"])
    print(f"{name}: restatement fp32 max err {err:.3e}, fp32 reference {ref_err:.3e}, ratio {err / ref_err:.2f}")
    assert err <= 4 * ref_err + 1e-6
    got64 = FC.forward_logits(P, name, conds, codes, rnd=None, prod=torch.float64, work=torch.float64)
    assert (got64 - gold).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", list(FC.CASES))
def test_cross_entropy_of_the_golden_logits_is_the_golden_nll(golden_dir, name):
    g, P, conds, codes = _load(golden_dir, name)
    gold = torch.from_numpy(g["logits64"])
    nll = torch.nn.functional.cross_entropy(gold.reshape(-1, gold.shape[-1]), codes.reshape(-1), reduction="none").view(codes.shape)
    assert (nll - torch.from_numpy(g["nll64"])).abs().max().item() <= 1e-12
    assert float(g["nll64"].mean()) > 0.5 * np.log(gold.shape[-1])      # seeded weights predict nothing: about log V


def test_sampling_and_forward_goldens_are_different_contracts(golden_dir):
    """under the cache time_shift(x) is zero, teacher-forced it is the previous token's ln1 row: same weights, same codes, other logits"""
    f = np.load(os.path.join(golden_dir, "gpt_fwd_tiny.npz"))
    s = np.load(os.path.join(golden_dir, "gpt_tiny.npz"))
    assert np.array_equal(f["codes"], s["forced_codes"]) and np.array_equal(f["conds"], s["conds"])
    a, b = torch.from_numpy(f["logits64"]), torch.from_numpy(s["logits64"])
    assert ((a - b).norm() / b.norm()).item() > 0.1
    assert (a[:, 0] - b[:, 0]).abs().max().item() < 1e-9      # the first position has no previous token in either


def test_forward_refuses_cpu_tensors():
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**FC.case_kwargs("tiny"))
    conds, codes = FC.case_inputs("tiny")
    with pytest.raises(NotImplementedError, match="forward"):
        m(codes, conds)


def test_new_symbols_are_bound():
    from enhancing import _C
    for name in ("enh_causal_attention_forward", "enh_causal_attention_forward_f32", "enh_ln_timeshift", "enh_gpt_embed_seq", "enh_relu_sq_h16",
                 "enh_cross_entropy_rows", "enh_mean_f32"):
        assert name in _C.SIGNATURES


PREFILL_LABELS = ["gpt_prefill_causal_kernel<64, F16>", "gpt_prefill_causal_kernel<192, BF16>", "gpt_prefill_causal_kernel<384, F16>", "gpt_prefill_causal_kernel<384, BF16>",
                  "gpt_prefill_ln_kernel<F16>", "gpt_prefill_ln_kernel<BF16>", "gpt_prefill_relu_sq_kernel<F16, true, false>",
                  "gpt_prefill_relu_sq_kernel<BF16, false, false>", "gpt_prefill_relu_sq_kernel<BF16, true, true>", "gpt_prefill_ce_kernel",
                  "gpt_prefill_mean_kernel", "gpt_prefill_embed_kernel", "gpt_prefill_causal_f32_kernel"]
# what the decode entry points report (tests/test_gpt_kernels_gpu.py reads them back after each call)
DECODE_LABELS = [f"gpt_skinny_gemm_kernel<{ot}, {mt}>" for ot in ("F16", "BF16") for mt in (1, 2, 4)] + [
    "gpt_skinny_gemm_f32_kernel", "gpt_decode_attn_kernel<F16, false>", "gpt_decode_attn_kernel<BF16, false>", "gpt_decode_attn_kernel<BF16, true>",
    "gpt_row_ln_kernel<F16>", "gpt_row_ln_kernel<BF16>", "gpt_embed_kernel", "gpt_sample_kernel"]


def test_prefill_labels_are_kernel_symbols_without_scratch():
    """every label the launches of the stage-2 forward and of sampling report (enh_last_kernel) is exactly one kernel symbol of the shipped library, and none of the
    new kernels uses scratch (the D = 384 causal kernel holds 96 accumulator and 96 Q-fragment registers per lane)"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import isa_lint
    if not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"):
        pytest.skip("needs the built library and the ROCm llvm tools")
    stats = isa_lint.kernel_stats()
    for label in PREFILL_LABELS + DECODE_LABELS:
        hits = [n for n in stats if n.startswith(label + "(") or n.startswith("void " + label + "(")]
        assert len(hits) == 1, (label, hits)
    mine = [n for n in stats if "gpt_prefill_" in n]
    assert len(mine) >= 12 + 2 + 5 + 4
    for n in mine:
        s = stats[n]
        assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0, (n, s)
        if "gpt_prefill_causal_kernel" in n:      # the hot path is an MFMA kernel
            assert s.get("mfma", 0) >= 8, (n, s.get("mfma"))
