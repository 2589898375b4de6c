"""The yardsticks of tests/attn_dh_util.py for CAUSAL attention (csrc/gpt_prefill.hip): the fp64 reference and the rounding model with keys > query
masked, checked with attn_dh_util's own bound and row metric (attn_out_bound, worst_rows, assert_rows_within; unchanged)."""
import torch

from attn_dh_util import assert_rows_within, attn_out_bound, worst_rows
from util import assert_elementwise

ATT_MARGIN = 2.0          # tests/test_elementwise_gpu.py, tests/test_attention_dim_head_gpu.py


def _heads(qkv, B, N, H, D, compute):
    return qkv.to(compute).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)


def causal_ref64(qkv, B: int, N: int, H: int, D: int, scale: float):
    """plain fp64 causal attention of the packed qkv [B, N, 3 H D]: out [B,N,H*D], lse [B,H,N], P |V| [B,N,H*D]"""
    q, k, v = _heads(qkv, B, N, H, D, torch.float64)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~torch.ones(N, N, dtype=torch.bool).tril(), float("-inf"))
    p = torch.softmax(s, dim=-1)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, H * D)
    return back(p @ v), torch.logsumexp(s, dim=-1), back(p @ v.abs())


def causal_model(qkv, B: int, N: int, H: int, D: int, scale: float, dt):
    """attn_dh_util.attn_model's forward with the causal mask: fp64 arithmetic except the roundings the kernel makes (exp(s - max) before P V, one
    rounding of out)"""
    r = lambda t: t.to(dt).to(torch.float64)
    q, k, v = _heads(qkv, B, N, H, D, torch.float64)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~torch.ones(N, N, dtype=torch.bool).tril(), float("-inf"))
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    return r((r(e) @ v) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B, N, H * D)


def check_causal_out(out, qkv, B: int, N: int, H: int, D: int, scale: float, dt, what: str, ref=None):
    """every element within ATT_MARGIN x attn_out_bound of the fp64 reference, every D-wide row within ATT_MARGIN x the worst row of the rounding
    model.  Returns (worst element / bound, worst row / model's worst row, the reference triple)."""
    ref = causal_ref64(qkv, B, N, H, D, scale) if ref is None else ref
    w = assert_elementwise(out, ref[0], ATT_MARGIN * attn_out_bound(ref[0], ref[2], dt, D), what + " out", tile=(64, D))
    m = worst_rows(causal_model(qkv, B, N, H, D, scale, dt), ref[0], H, D)
    assert m == m, (what, m)
    k = assert_rows_within(out, ref[0], H, D, ATT_MARGIN * m, what + " out rows")      # (m == 0: one key per row, out is v itself — and must be, bit for bit)
    return w, (k / m if m > 0 else 0.0), ref
