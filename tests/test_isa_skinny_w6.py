"""Resources of the MXFP6 weight-streaming product (csrc/gpt_decode_w6.hip) in the built library: every instantiation of gpt_skinny_gemm_w6_kernel
(two operand types by three row-tile counts) exists, runs without scratch or spills and multiplies on the matrix cores; the quantizer and the slab
pass run without scratch too.  Resource figures only; results: tests/test_mxfp6_kernels_gpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"),
                                reason="needs the built library and the ROCm llvm tools")

PRODUCTS = [f"gpt_skinny_gemm_w6_kernel<{ot}, {mt}>" for ot in ("BF16", "F16") for mt in (1, 2, 4)]
HELPERS = ["gpt_mxfp6_quantize_kernel", "gpt_skinny_w6_reduce_kernel<BF16>", "gpt_skinny_w6_reduce_kernel<F16>"]


@pytest.fixture(scope="module")
def stats():
    return isa_lint.kernel_stats()


def _find(stats, symbol):
    return [n for n in stats if n.replace("void ", "").split("(")[0] == symbol]


def test_the_family_is_two_types_by_three_row_tiles(stats):
    got = sorted(n.split("(")[0].replace("void ", "") for n in stats if "gpt_skinny_gemm_w6" in n)
    assert got == sorted(PRODUCTS)


@pytest.mark.parametrize("symbol", PRODUCTS)
def test_product_has_no_scratch_and_uses_the_matrix_cores(stats, symbol):
    hits = _find(stats, symbol)
    assert len(hits) == 1, (symbol, hits)
    s = stats[hits[0]]
    print(f"{symbol}: registers {s.get('vgpr')} (agpr {s.get('agpr')}), lds {s.get('lds')}, mfma {s.get('mfma')}")
    assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0 and s.get("atomics", 0) == 0, (symbol, s)
    assert s.get("mfma", 0) >= 1, (symbol, s)


@pytest.mark.parametrize("symbol", HELPERS)
def test_helpers_exist_without_scratch(stats, symbol):
    hits = _find(stats, symbol)
    assert len(hits) == 1, (symbol, hits)
    s = stats[hits[0]]
    assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0 and s.get("atomics", 0) == 0, (symbol, s)
