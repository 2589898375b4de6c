"""tests/attn_dh_util.py at D = 64 is tests/util.py: every helper returns the same tensors / numbers (torch.equal) on the same seeded inputs."""
import pytest
import torch

import attn_dh_util as A
import util as U

BF16, F16 = torch.bfloat16, torch.float16


def _inputs(B, N, H, dt):
    g = torch.Generator().manual_seed(B * 100 + N + H)
    qkv = U.h16r(torch.randn(B, N, 3 * H * 64, generator=g) * 1.5, dt)
    do = U.h16r(torch.randn(B, N, H * 64, generator=g), dt)
    return qkv, do


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,N,H", [(2, 40, 2), (1, 129, 3)])
def test_helpers_at_64_are_the_helpers_of_util(B, N, H, dt):
    qkv, do = _inputs(B, N, H, dt)
    r_old, r_new = U.attn_ref64(qkv, do, B, N, H, 0.125), A.attn_ref64(qkv, do, B, N, H, 64, 0.125)
    for a, b in zip(r_old[:3], r_new[:3]):
        assert torch.equal(a, b)
    for a, b in zip(r_old[3], r_new[3]):
        assert torch.equal(a, b)
    assert torch.equal(U.attn_out_bound(r_old[0], r_old[2], dt), A.attn_out_bound(r_new[0], r_new[2], dt, 64))
    m_old, m_new = U.attn_model(qkv.double(), do, B, N, H, 0.125, dt), A.attn_model(qkv.double(), do, B, N, H, 64, 0.125, dt)
    for a, b in zip(m_old, m_new):
        assert torch.equal(a, b)
    # the model fed a stored out / lse (what the GPU tests do)
    out16, lse32 = m_old[0].to(dt), m_old[1].float()
    for a, b in zip(U.attn_model(qkv.double(), do, B, N, H, 0.125, dt, out=out16, lse=lse32), A.attn_model(qkv.double(), do, B, N, H, 64, 0.125, dt, out=out16, lse=lse32)):
        assert torch.equal(a, b)
    for got, ref in zip(m_old[2:], r_old[3]):
        w = U.worst_rows(got, ref, H)
        assert w == A.worst_rows(got, ref, H, 64) and w > 0
        assert U.assert_rows_within(got, ref, H, 2 * w, "old") == A.assert_rows_within(got, ref, H, 64, 2 * w, "new")


def test_non_finite_rows_are_reported_the_same_way():
    qkv, do = _inputs(1, 8, 2, BF16)
    ref = U.attn_ref64(qkv, do, 1, 8, 2, 0.125)[3][0]
    got = ref.clone()
    got[0, 3, 70] = float("nan")
    assert U.worst_rows(got, ref, 2) != U.worst_rows(got, ref, 2) and A.worst_rows(got, ref, 2, 64) != A.worst_rows(got, ref, 2, 64)
    with pytest.raises(AssertionError, match="batch 0, token 3, head 1"):
        A.assert_rows_within(got, ref, 2, 64, 1.0, "x")


def test_out_bound_term_grows_with_the_head_width():
    ref, pav = torch.ones(2, 2), torch.ones(2, 2)
    for D in (32, 96, 128):
        b = A.attn_out_bound(ref, pav, BF16, D)
        assert torch.equal(b, U.U16[BF16] * ref + (U.U16[BF16] + 2.0 ** -20 * D / 64) * pav)
