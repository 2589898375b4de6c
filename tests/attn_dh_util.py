"""attn_ref64, attn_model, attn_out_bound, worst_rows and assert_rows_within of tests/util.py with the head width D as an argument (util.py fixes 64).
Same formulas; at D = 64 every helper returns exactly what util.py returns (tests/test_attn_dh_util_cpu.py), so the yardstick of the new head widths
is the yardstick of the old one."""
import torch

from util import U16, row_err


def attn_model(qkv, do, B: int, N: int, H: int, D: int, scale: float, dt, compute=torch.float64, out=None, lse=None):
    """util.attn_model for qkv packed [B, N, 3 H D]: fp64 arithmetic except the roundings to `dt` that the kernels make (exp(s - max) before P V, one
    rounding of out; P and P o (dP - delta) before the backward's products, delta on the STORED out, one rounding of each gradient).
    Returns out [B,N,H*D], lse [B,H,N], dq, dk, dv [B,N,H*D]."""
    def r(t):
        return t.to(dt).to(compute)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, H * D)
    heads = lambda t: t.to(compute).view(B, N, H, D).permute(0, 2, 1, 3)
    q, k, v = qkv.to(compute).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    g = heads(do)
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    out_m, lse_m = r((r(e) @ v) / l), (m + torch.log(l)).squeeze(-1)
    o_in = out_m if out is None else heads(out.detach().cpu())
    lse_in = lse_m if lse is None else lse.detach().cpu().to(compute)
    p = torch.exp(s - lse_in.unsqueeze(-1))
    dv = r(r(p).transpose(-1, -2) @ g)
    delta = (g * o_in).sum(-1, keepdim=True)
    ds = r(p * (g @ v.transpose(-1, -2) - delta))
    dq = r((ds @ k) * scale)
    dk = r((ds.transpose(-1, -2) @ q) * scale)
    return back(out_m), lse_m, back(dq), back(dk), back(dv)


def attn_ref64(qkv, do, B: int, N: int, H: int, D: int, scale: float):
    """plain fp64 attention of the packed qkv [B, N, 3 H D] and its autograd: out [B,N,H*D], lse [B,H,N], P |V|, (dq, dk, dv)"""
    qt = qkv.double().clone().requires_grad_(True)
    q, k, v = qt.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    out = (p @ v).permute(0, 2, 1, 3).reshape(B, N, H * D)
    out.backward(do.double())
    pav = (p.detach() @ v.detach().abs()).permute(0, 2, 1, 3).reshape(B, N, H * D)
    return out.detach(), torch.logsumexp(s.detach(), dim=-1), pav, qt.grad.view(B, N, 3, H * D).unbind(2)


def attn_out_bound(ref, pav, dt, D: int):
    """util.attn_out_bound with the softmax / score term scaled by D / 64: u |ref| + (u + 2^-20 D / 64) P |V|.  The 2^-20 of util.py stands for the f32
    error of the scores (sums of D products), exp2 and the row sum at D = 64; the score sums grow with D, so the term does (a derivation, not a measurement)."""
    return U16[dt] * ref.abs() + (U16[dt] + 2.0 ** -20 * (D / 64)) * pav


def worst_rows(got, ref, H: int, D: int) -> float:
    """util.worst_rows over D-wide rows (nan when any element is non-finite)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return torch.stack([row_err(got[..., h * D:(h + 1) * D], ref[..., h * D:(h + 1) * D], D).max() for h in range(H)]).max().item()


def assert_rows_within(got, ref, H: int, D: int, limit: float, what: str) -> float:
    """util.assert_rows_within over D-wide rows"""
    g = got.detach().double().cpu()
    bad = ~torch.isfinite(g.reshape(*g.shape[:-1], H, D)).all(-1)
    if bool(bad.any()):
        b, n, h = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} rows hold non-finite values, the first at batch {b}, token {n}, head {h}")
    w = worst_rows(got, ref, H, D)
    assert w <= limit, f"{what}: worst row {w:.3e} beyond {limit:.3e}"
    return w
