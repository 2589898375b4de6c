"""CPU-side tie between the timing labels tests/test_kernel_labels_gpu.py expects and the shipped library: every EXPECTED entry is exactly one kernel
symbol of the code object (the name with its template arguments, as a profiler prints it), so a committed label cannot name a kernel that does not exist."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402
from test_kernel_labels_gpu import EXPECTED  # noqa: E402

needs_lib = pytest.mark.skipif(not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"),
                               reason="needs the built library and the ROCm llvm tools")


@pytest.fixture(scope="module")
def stats():
    return isa_lint.kernel_stats()


def _find(names, kernel):
    hits = [n for n in names if n.startswith(kernel + "(") or n.startswith("void " + kernel + "(")]
    assert len(hits) == 1, (kernel, hits)
    return hits[0]


@needs_lib
@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_expected_label_is_one_kernel_symbol(stats, case):
    print(f"{case}: {_find(stats, EXPECTED[case])}")
