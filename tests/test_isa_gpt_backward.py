"""Resources of the causal attention backward kernels (csrc/gpt_attn_bwd.hip) in the built library: every instantiation exists for both operand
types, runs without scratch or spills inside the one-wave-per-SIMD register budget, and its register counts are the ones DESIGN.md §3.7 records
(TABLE below is that table: total registers per lane = .vgpr_count, of which accumulation registers = .agpr_count, LDS bytes per workgroup).  The
labels the new launches report are kernel symbols of the library.  Resource figures only; results: tests/test_gpt_backward_kernels_gpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"),
                                reason="needs the built library and the ROCm llvm tools")

#        kernel                        D: (registers, of which AGPRs, LDS bytes)
TABLE = {"gpt_causal_bwd_dq_kernel": {64: (192, 64, 32768), 128: (280, 96, 65536), 192: (304, 80, 98304), 256: (352, 96, 131072), 320: (386, 130, 81920),
                                      384: (452, 196, 98304)},
         "gpt_causal_bwd_dkv_kernel": {64: (264, 96, 33792), 128: (425, 169, 66560), 192: (393, 137, 99328), 256: (360, 104, 132096), 320: (410, 154, 82432),
                                       384: (483, 227, 98816)}}
ROW_KERNELS = ["gpt_ce_bwd_kernel<F16>", "gpt_ce_bwd_kernel<BF16>", "gpt_relu_sq_bwd_kernel<F16>", "gpt_relu_sq_bwd_kernel<BF16>",
               "gpt_ln_timeshift_bwd_kernel<F16>", "gpt_ln_timeshift_bwd_kernel<BF16>", "gpt_ln_bwd_reduce_kernel", "gpt_embed_seq_bwd_kernel"]


@pytest.fixture(scope="module")
def stats():
    return isa_lint.kernel_stats()


def _find(stats, symbol):
    return [n for n in stats if n.replace("void ", "").split("(")[0] == symbol]


def test_the_family_is_two_kernels_by_six_widths_by_two_types(stats):
    got = sorted(n.split("(")[0].replace("void ", "") for n in stats if "gpt_causal_bwd_" in n)
    assert got == sorted(f"{k}<{D}, {ot}>" for k in TABLE for D in TABLE[k] for ot in ("BF16", "F16"))


@pytest.mark.parametrize("ot", ["BF16", "F16"])
@pytest.mark.parametrize("D", [64, 128, 192, 256, 320, 384])
@pytest.mark.parametrize("kernel", sorted(TABLE))
def test_attention_backward_resources(stats, kernel, D, ot):
    hits = _find(stats, f"{kernel}<{D}, {ot}>")
    assert len(hits) == 1, (kernel, D, ot, hits)
    s = stats[hits[0]]
    print(f"{kernel}<{D}, {ot}>: registers {s.get('vgpr')} (agpr {s.get('agpr')}), lds {s.get('lds')}, mfma {s.get('mfma')}")
    assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0, (hits[0], s)
    assert (s.get("vgpr", 0), s.get("agpr", 0), s.get("lds", 0)) == TABLE[kernel][D], (hits[0], s.get("vgpr"), s.get("agpr"), s.get("lds"), TABLE[kernel][D])
    assert s["vgpr"] <= 512 and s["lds"] <= 160 * 1024


@pytest.mark.parametrize("symbol", ROW_KERNELS)
def test_row_kernels_exist_without_scratch(stats, symbol):
    hits = _find(stats, symbol)
    assert len(hits) == 1, (symbol, hits)
    s = stats[hits[0]]
    assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0 and s.get("atomics", 0) == 0, (symbol, s)
