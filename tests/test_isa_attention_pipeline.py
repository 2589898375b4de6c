"""CPU-side lint of the attention kernels' TILE LOOPS in the shipped library (tools/isa_lint.py attention_pipeline, on the disassembly of
enhancing-transformers_amd/lib/libenh_hip.so): the next tile's LDS-DMA prefetch is not drained inside a tile, fragment reads run ahead of the MFMAs that
consume them, and nothing touches the registers of a fragment read the kernel counts itself before that read has been waited for.

Before the kernels took their fragments through the counted reads of attention_common.h (att_req_* / att_take_*) the same analysis gave, for both
operand types: forward 2 waits that name vmcnt per tile loop and 15 of its 16 MFMAs behind a read awaited at once, dQ 2 and 20 of 24, dK/dV 2 and 28 of
32 — the compiler's wait-count pass put s_waitcnt vmcnt(0) in front of the first read of the tile ring and chained ds_read / lgkmcnt(0) / v_mfma."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

needs_lib = pytest.mark.skipif(not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"),
                               reason="needs the built library and the ROCm llvm tools")

OTS = ("BF16", "F16")
# the three default kernels of the training path (pre-scaled q).  Phase starts per tile loop body, from the source (attention.hip): a phase is a group of
# MFMAs that share an accumulator set, and the first fragment of a phase may be requested where the phase begins.
#   forward: S products (8) | O products (8)                                               -> 2
#   dQ     : per key block (2): S / dP products (8) | dQ products (4)                      -> 4
#   dK/dV  : per query block (2): S / dP products (8, behind the statistics) | dV / dK (8) -> 4
PHASE_STARTS = {"attn_fwd_pre_kernel<{ot}>": 2, "attn_bwd_dq_kernel<2, {ot}>": 4, "attn_bwd_dkv_kernel<true, true, {ot}>": 4}
# (all three take the read-ahead inside their occupancy classes: no kernel ships with the undrained prefetch alone)


@pytest.fixture(scope="module")
def listings():
    return isa_lint.kernel_listings()


def _find(listings, pattern, ot):
    names = [n for n in listings if n.startswith("void " + pattern.format(ot=ot) + "(")]
    assert len(names) == 1, (pattern, ot, names)
    return names[0]


@needs_lib
@pytest.mark.parametrize("ot", OTS)
@pytest.mark.parametrize("kernel", sorted(PHASE_STARTS))
def test_the_prefetch_is_awaited_once_per_tile_in_front_of_the_barrier(listings, kernel, ot):
    """inside the tile loop exactly one s_waitcnt names vmcnt, and an s_barrier follows it before any MFMA: the tile that was requested at the top of
    the loop body is awaited where the body ends, not in front of the body's own fragment reads"""
    r = isa_lint.attention_pipeline(listings[_find(listings, kernel, ot)])
    assert r["mfma"] in (16, 24, 32), r
    assert len(r["vm_waits"]) == 1, (kernel, ot, r["vm_waits"])
    assert r["closing_ok"], (kernel, ot)


@needs_lib
@pytest.mark.parametrize("ot", OTS)
@pytest.mark.parametrize("kernel", sorted(PHASE_STARTS))
def test_fragment_reads_run_ahead_of_the_mfmas(listings, kernel, ot):
    """MFMAs whose operand read was issued after the previous MFMA and awaited with lgkmcnt(0) before anything else was done: at most one per phase start"""
    r = isa_lint.attention_pipeline(listings[_find(listings, kernel, ot)])
    assert r["exposed"] <= PHASE_STARTS[kernel], (kernel, ot, r["exposed"], PHASE_STARTS[kernel])


@needs_lib
def test_counted_fragment_reads_keep_their_registers_until_the_wait(listings):
    """every LDS-DMA attention kernel (all template instances): no instruction names a register an LDS read is still writing, no such read is carried over a
    branch inside the tile loop, and no scalar load shares the counter the kernels count by hand"""
    seen = 0
    for name, listing in listings.items():
        if not name.startswith(("void attn_fwd_pre_kernel<", "void attn_bwd_dq_kernel<", "void attn_bwd_dkv_kernel<")):
            continue
        seen += 1
        r = isa_lint.attention_pipeline(listing)
        assert r["touched"] == [] and r["carried"] == 0 and r["scalar_loads"] == 0, (name, r["touched"][:3], r["carried"], r["scalar_loads"])
    assert seen == 14, seen      # forward 2, dQ 3 x 2, dK/dV 3 x 2


def _listing(instructions):
    """hand-written instructions -> a listing; `@N` at the end of a branch is its target index"""
    out = []
    for i, ins in enumerate(instructions):
        tgt = None
        if "@" in ins:
            ins, t = ins.split("@")
            tgt = 4 * int(t)
        out.append((4 * i, ins.strip(), tgt))
    return out


def test_pipeline_analysis_on_hand_written_loops():
    serial = _listing(["s_nop 0",
                       "ds_read_b128 v[0:3], v40",                      # 1: loop start
                       "s_waitcnt vmcnt(0)",
                       "s_waitcnt lgkmcnt(0)",
                       "v_mfma_f32_32x32x16_f16 v[16:31], v[0:3], v[4:7], v[16:31]",
                       "ds_read_b128 v[0:3], v40 offset:64",
                       "s_waitcnt lgkmcnt(0)",
                       "v_mfma_f32_32x32x16_f16 v[16:31], v[0:3], v[4:7], v[16:31]",
                       "s_waitcnt vmcnt(0) lgkmcnt(0)",
                       "v_mfma_f32_32x32x16_f16 v[16:31], v[0:3], v[4:7], v[16:31]",
                       "s_barrier",
                       "s_cbranch_scc0 @1"])
    r = isa_lint.attention_pipeline(serial)
    assert (r["mfma"], r["exposed"], len(r["vm_waits"]), r["closing_ok"], r["touched"]) == (3, 2, 2, False, [])
    ahead = _listing(["ds_read_b128 v[0:3], v40",                       # 0: loop start
                      "ds_read_b128 v[8:11], v40 offset:64",
                      "s_waitcnt lgkmcnt(1)",
                      "v_mfma_f32_32x32x16_f16 v[16:31], v[0:3], v[4:7], v[16:31]",
                      "ds_read_b64_tr_b16 v[0:1], v40 offset:128",
                      "ds_read_b64_tr_b16 v[2:3], v40 offset:192",
                      "s_waitcnt lgkmcnt(2)",
                      "v_mfma_f32_32x32x16_f16 v[16:31], v[8:11], v[4:7], v[16:31]",
                      "s_waitcnt lgkmcnt(0)",
                      "v_mfma_f32_32x32x16_f16 v[16:31], v[0:3], v[4:7], v[16:31]",
                      "s_waitcnt vmcnt(0)",
                      "s_barrier",
                      "s_cbranch_scc0 @0"])
    r = isa_lint.attention_pipeline(ahead)
    assert (r["mfma"], r["exposed"], len(r["vm_waits"]), r["closing_ok"], r["touched"], r["carried"]) == (3, 0, 1, True, [], 0)
    # a copy of a fragment register between request and wait, and an MFMA issued one wait too early
    early = _listing(["ds_read_b128 v[0:3], v40",
                      "ds_read_b128 v[8:11], v40 offset:64",
                      "v_mov_b32_e32 v12, v8",
                      "s_waitcnt lgkmcnt(1)",
                      "v_mfma_f32_32x32x16_f16 v[16:31], v[8:11], v[4:7], v[16:31]",
                      "s_waitcnt vmcnt(0) lgkmcnt(0)",
                      "s_barrier",
                      "s_branch @0"])
    r = isa_lint.attention_pipeline(early)
    assert [i for i, _ in r["touched"]] == [2, 4], r["touched"]
