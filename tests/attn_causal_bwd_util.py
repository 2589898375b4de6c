"""The backward yardsticks of tests/attn_dh_util.py (attn_model, attn_ref64) for CAUSAL attention at head width D (csrc/gpt_attn_bwd.hip): the same
formulas with keys > query masked.  Rows are measured with attn_dh_util.worst_rows / assert_rows_within, unchanged."""
import torch


def _mask(N):
    return ~torch.ones(N, N, dtype=torch.bool).tril()


def causal_bwd_ref64(qkv, do, B: int, N: int, H: int, D: int, scale: float):
    """fp64 causal attention of the packed qkv [B, N, 3 H D] and its autograd: (dq, dk, dv), each [B, N, H D]"""
    qt = qkv.double().clone().requires_grad_(True)
    q, k, v = qt.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(_mask(N), float("-inf"))
    out = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, N, H * D)
    out.backward(do.double())
    return tuple(t.contiguous() for t in qt.grad.view(B, N, 3, H * D).unbind(2))


def causal_bwd_model(qkv, do, out, lse, B: int, N: int, H: int, D: int, scale: float, dt):
    """attn_dh_util.attn_model's backward with the causal mask, GIVEN the kernel's own stored out [B,N,H*D] and lse [B,H,N]: fp64 arithmetic except
    the roundings to `dt` that the kernels make (P = exp(s - lse) before P^T dO, P o (dP - delta) before the dQ / dK products, delta on the stored out,
    one rounding of each gradient).  Returns (dq, dk, dv)."""
    f64 = torch.float64
    r = lambda t: t.to(dt).to(f64)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, H * D)
    heads = lambda t: t.detach().cpu().to(f64).view(B, N, H, D).permute(0, 2, 1, 3)
    q, k, v = qkv.detach().cpu().to(f64).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    g, o = heads(do), heads(out)
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(_mask(N), float("-inf"))
    p = torch.exp(s - lse.detach().cpu().to(f64).unsqueeze(-1))
    dv = r(r(p).transpose(-1, -2) @ g)
    ds = r(p * (g @ v.transpose(-1, -2) - (g * o).sum(-1, keepdim=True)))
    return back(r((ds @ k) * scale)), back(r((ds.transpose(-1, -2) @ q) * scale)), back(dv)
