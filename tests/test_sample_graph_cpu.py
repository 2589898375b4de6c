"""The host side of graphed stage-2 sampling, without a device: the cursor entries are declared in include/enh_hip.h, exported by
the built library and bound in _C; every label they report is exactly one kernel symbol of the code object, without scratch or spills; the
`graph` keyword is accepted by both priors, refuses what the loop refuses, and reads ENH_GRAPHS only when it is None."""
import os
import re
import sys

import pytest
import torch

import gpt_cases as GC
import rq_sample_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURSOR_ENTRIES = ("enh_cursor_advance", "enh_decode_attention_at", "enh_embed_step_at", "enh_sample_logits_at")
# what the entries pass to enh_note_kernel_plain (csrc/gpt_decode.hip), and the merge kernel that follows the attention
CURSOR_LABELS = ["gpt_cursor_advance_kernel", "gpt_decode_attn_at_kernel<F16, false>", "gpt_decode_attn_at_kernel<BF16, false>",
                 "gpt_decode_attn_at_kernel<BF16, true>", "gpt_embed_at_kernel", "gpt_sample_at_kernel"]
MERGE_KERNELS = ["gpt_decode_attn_merge_at_kernel<F16, false>", "gpt_decode_attn_merge_at_kernel<BF16, false>", "gpt_decode_attn_merge_at_kernel<BF16, true>"]


def test_cursor_entries_are_declared_exported_and_bound():
    from enhancing import _C
    hdr = open(os.path.join(ROOT, "include", "enh_hip.h")).read()
    L = _C.lib()
    for name in CURSOR_ENTRIES:
        assert re.search(r"\bint %s\(" % name, hdr), f"{name} is not declared in include/enh_hip.h"
        assert name in _C.SIGNATURES and getattr(L, name).argtypes == _C.SIGNATURES[name][1]
    for wrapper in ("cursor_advance", "decode_attention_at", "embed_step_at", "sample_logits_at"):
        assert callable(getattr(_C, wrapper))
    assert L.enh_abi_version() == _C.ABI_VERSION >= 30


def test_reported_labels_are_the_labels_of_the_sources():
    """the list above is what the sources pass to enh_note_kernel_plain in the cursor entries"""
    src = "".join(open(os.path.join(ROOT, "enhancing-transformers_amd", "csrc", f)).read() for f in ("gpt_decode.hip",))
    noted = set(re.findall(r'"((?:gpt|rq)_[a-z_]*_at_kernel(?:<[A-Z0-9]+, (?:true|false)>)?|gpt_cursor_advance_kernel)"', src))
    assert noted == set(CURSOR_LABELS), noted ^ set(CURSOR_LABELS)


def test_cursor_labels_are_kernel_symbols_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not os.path.exists(isa_lint.LLVM + "/llvm-objdump"):
        pytest.skip("needs the ROCm llvm tools")
    stats = isa_lint.kernel_stats()
    for label in CURSOR_LABELS + MERGE_KERNELS:
        hits = [n for n in stats if n.startswith(label + "(") or n.startswith("void " + label + "(")]
        assert len(hits) == 1, (label, hits)
        st = stats[hits[0]]
        print(f"{label}: vgpr {st['vgpr']} scratch {st['scratch_bytes']} spills {st['spills']} lds {st['lds']}")
        assert st["scratch_bytes"] == 0 and st.get("scratch_ops", 0) == 0 and st["spills"] == 0, (label, dict(st))


def _priors():
    from enhancing.modules.stage2.layers import GPT, RQTransformer
    return [(GPT(**GC.case_kwargs("tiny")), GC.make_inputs("tiny")[0]), (RQTransformer(**SC.case_kwargs("rq_tiny")), SC.case_inputs("rq_tiny")[0])]


def test_graph_with_host_conds_raises_what_the_loop_raises():
    for m, conds in _priors():
        raised = []
        for graph in (False, True):
            with pytest.raises((RuntimeError, NotImplementedError)) as ei:
                m.sample(conds, graph=graph)
            raised.append((type(ei.value), str(ei.value)))
        assert raised[0] == raised[1] and "device tensor" in raised[0][1]


def test_enh_graphs_is_read_only_when_graph_is_none(monkeypatch):
    from enhancing import _C
    from enhancing.modules.stage2.prior import Prior
    reads = []

    class Env(dict):      # the environment prior.py sees, with its reads recorded
        def get(self, key, default=None):
            reads.append(key)
            return super().get(key, default)

    import types
    import enhancing.modules.stage2.prior as prior
    env = Env(ENH_GRAPHS="1")
    monkeypatch.setattr(prior, "os", types.SimpleNamespace(environ=env))
    monkeypatch.setattr(_C, "TIMER", None)
    assert Prior._use_graph(False) is False and Prior._use_graph(True) is True and "ENH_GRAPHS" not in reads
    assert Prior._use_graph(None) is True and reads.count("ENH_GRAPHS") == 1
    env["ENH_GRAPHS"] = "0"
    assert Prior._use_graph(None) is False and Prior._use_graph(True) is True
    del env["ENH_GRAPHS"]
    assert Prior._use_graph(None) is False
    # per-kernel timing on: the loop, whatever the caller asked for
    monkeypatch.setattr(_C, "TIMER", _C.KernelTimer())
    assert Prior._use_graph(True) is False
