"""Timing labels of the stage-2 backward's launches (the pattern of tests/test_kernel_labels_gpu.py): under a KernelTimer every new entry point
records exactly one label, the symbol of the kernel it launched (tests/test_isa_gpt_backward.py holds the symbols to the built library)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _label(C, call):
    timer = C.KernelTimer()
    C.TIMER = timer
    try:
        call()
    finally:
        C.TIMER = None
    torch.cuda.synchronize()
    got = list(timer.records)
    assert len(got) == 1, got
    return got[0], timer.units[got[0]]


@pytest.mark.parametrize("dt,tag", [(F16, "F16"), (BF16, "BF16")])
def test_labels(C, dt, tag):
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")
    B, N, H, D = 1, 8, 1, 192
    qkv, out, lse = z(B, N, 3 * H * D, dtype=dt), z(B, N, H * D, dtype=dt), z(B, H, N)
    C.causal_attention(qkv, B, N, H, D, out, lse)
    assert _label(C, lambda: C.causal_attention_backward(qkv, out, out, lse, B, N, H, D, torch.empty_like(qkv))) == (f"gpt_causal_bwd_dkv_kernel<192, {tag}>", "flop")
    tgt = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert _label(C, lambda: C.cross_entropy_backward(z(4, 64), tgt, z(4), z(4, 64, dtype=dt), 1.0)) == (f"gpt_ce_bwd_kernel<{tag}>", "byte")
    assert _label(C, lambda: C.relu_sq_backward(z(4, 64), z(4, 64, dtype=dt), z(4, 64, dtype=dt))) == (f"gpt_relu_sq_bwd_kernel<{tag}>", "byte")
    w = torch.ones(64, device="cuda")
    assert _label(C, lambda: C.ln_timeshift_backward(z(4, 64), torch.randn(4, 64, device="cuda"), w, 2, z(4, 64), z(64), z(64), b=w, colscale=w, dcolscale=z(64),
                                                     dx16=z(4, 64, dtype=dt))) == (f"gpt_ln_timeshift_bwd_kernel<{tag}>", "byte")
    codes = torch.zeros(2, 3, dtype=torch.int64, device="cuda")
    assert _label(C, lambda: C.gpt_embed_seq_backward(z(2, 3, 64), tgt[:2], codes, z(5, 64), z(64), z(7, 64), z(3, 64))) == ("gpt_embed_seq_bwd_kernel", "byte")
