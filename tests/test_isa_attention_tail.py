"""CPU-side lint of the attention TAIL kernels in the shipped library (token counts that are no multiple of 64: csrc/attention_tail.hip, x3_tail.hip):
every tail kernel exists for both operand types, without scratch or spills, and the tile loop of the LDS-DMA ones is the aligned kernels' loop as far
as the counted fragment reads go — nothing names a fragment's registers between request and wait, no read is carried over a branch, no scalar load
shares the counter.  The masked instance of the tile body stands BEHIND the loop, so tools/isa_lint.py attention_pipeline (which looks at the span of
the backward branches) sees the loop alone.  Register counts are printed, not asserted: the tail forms are not tuned to the aligned kernels'
occupancy classes."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

needs_lib = pytest.mark.skipif(not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"),
                               reason="needs the built library and the ROCm llvm tools")

OTS = ("BF16", "F16")
DMA_TAIL = ["attn_fwd_tail_pre_kernel<{ot}>", "attn_bwd_tail_dq_kernel<1, {ot}>", "attn_bwd_tail_dq_kernel<2, {ot}>",
            "attn_bwd_tail_dkv_kernel<true, false, {ot}>", "attn_bwd_tail_dkv_kernel<true, true, {ot}>"]
MFMA_PER_TILE = {"attn_fwd_tail_pre_kernel": 16, "attn_bwd_tail_dq_kernel": 24, "attn_bwd_tail_dkv_kernel": 32}      # as the aligned kernels
ALL_TAIL = [k.format(ot=ot) for k in DMA_TAIL + ["attn_fwd_tail_kernel<{ot}>"] for ot in OTS] + ["attn_fwd_tail_x3_kernel"]      # (x3 is bf16 by construction)


@pytest.fixture(scope="module")
def stats():
    return isa_lint.kernel_stats()


@pytest.fixture(scope="module")
def listings():
    return isa_lint.kernel_listings()


def _find(names, kernel):
    hits = [n for n in names if n.startswith(kernel + "(") or n.startswith("void " + kernel + "(")]
    assert len(hits) == 1, (kernel, hits)
    return hits[0]


@needs_lib
@pytest.mark.parametrize("kernel", ALL_TAIL)
def test_tail_kernel_exists_without_scratch_or_spills(stats, kernel):
    s = stats[_find(stats, kernel)]
    print(f"{kernel}: {s.get('vgpr')} VGPRs, {s.get('agpr', 0)} AGPRs, {s.get('sgpr')} SGPRs, {s.get('lds', 0)} B LDS")
    assert s.get("scratch_bytes", 0) == 0 and s.get("scratch_ops", 0) == 0 and s.get("spills", 0) == 0, (kernel, s)


@needs_lib
@pytest.mark.parametrize("ot", OTS)
@pytest.mark.parametrize("kernel", DMA_TAIL)
def test_tail_tile_loop_keeps_the_counted_reads_intact(stats, listings, kernel, ot):
    name = kernel.format(ot=ot)
    r = isa_lint.attention_pipeline(listings[_find(listings, name)])
    print(f"{name}: {stats[_find(stats, name)].get('vgpr')} VGPRs; tile loop: {r['mfma']} MFMAs, {len(r['vm_waits'])} vmcnt wait(s), {r['exposed']} exposed reads")
    assert r["touched"] == [] and r["carried"] == 0 and r["scalar_loads"] == 0, (name, r["touched"][:3], r["carried"], r["scalar_loads"])
    assert r["mfma"] == MFMA_PER_TILE[kernel.split("<")[0]], (name, r["mfma"])      # one tile body in the loop: the masked instance is not inside it


@needs_lib
def test_tail_kernels_do_not_take_the_aligned_kernels_names(listings):
    """the aligned kernels are looked up by name elsewhere (tests/test_isa_attention_pipeline.py counts 14 instances, tests/test_isa_lint.py takes exact
    signatures): a tail form under one of those prefixes would be mistaken for them"""
    tails = [n for n in listings if "_tail_" in n]
    assert len(tails) == 13, tails
    assert not [n for n in tails if n.startswith(("void attn_fwd_pre_kernel<", "void attn_bwd_dq_kernel<", "void attn_bwd_dkv_kernel<"))]
    assert all("attn_fwd" in n or "attn_bwd" in n for n in tails)
