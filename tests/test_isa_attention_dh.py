"""Resources of the attn_dh_* kernels (head widths 32 / 96 / 128, csrc/attention_dh.h) in the built library: every kernel exists for both operand
types, runs without scratch or spills inside the one-wave-per-SIMD register budget, and its listing holds at least one tile's MFMAs:
    forward  2 D/16 (S)           + 4 D/32 (P V)
    dQ       2 * 2 D/16 (S, dP)   + 4 D/32 (dS K)
    dK/dV    2 * 2 D/16 (S, dP)   + 2 * 4 D/32 (dV, dK)
This file checks resources only; results are checked in tests/test_attention_dim_head_gpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"),
                                reason="needs the built library and the ROCm llvm tools")

MFMA_PER_TILE = {"attn_dh_fwd_kernel": lambda D: 2 * D // 16 + 4 * D // 32,
                 "attn_dh_bwd_dq_kernel": lambda D: 4 * D // 16 + 4 * D // 32,
                 "attn_dh_bwd_dkv_kernel": lambda D: 4 * D // 16 + 8 * D // 32}


@pytest.fixture(scope="module")
def stats():
    return isa_lint.kernel_stats()


def test_the_family_is_exactly_three_kernels_by_three_widths_by_two_types(stats):
    got = sorted(n.split("(")[0].replace("void ", "") for n in stats if "attn_dh_" in n)
    want = sorted(f"{k}<{D}, {ot}>" for k in MFMA_PER_TILE for D in (32, 96, 128) for ot in ("BF16", "F16"))
    assert got == want


@pytest.mark.parametrize("ot", ["BF16", "F16"])
@pytest.mark.parametrize("D", [32, 96, 128])
@pytest.mark.parametrize("kernel", sorted(MFMA_PER_TILE))
def test_kernel_resources(stats, kernel, D, ot):
    hits = [n for n in stats if n.startswith(f"void {kernel}<{D}, {ot}>(")]
    assert len(hits) == 1, (kernel, D, ot, hits)
    s = stats[hits[0]]
    print(f"{kernel}<{D}, {ot}>: vgpr {s.get('vgpr')} (agpr {s.get('agpr')}), lds {s.get('lds')}, mfma {s.get('mfma')}")
    assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0, (hits[0], s)
    assert 0 < s.get("vgpr", 0) <= 512, (hits[0], s)
    assert s.get("mfma", 0) >= MFMA_PER_TILE[kernel](D), (hits[0], s.get("mfma"), MFMA_PER_TILE[kernel](D))
    assert s.get("lds", 0) <= 160 * 1024, (hits[0], s)
