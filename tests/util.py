import torch


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    """relative Frobenius error ||a-b|| / ||b|| in float64 (the parity metric of SURVEY.md §8d)."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def bf16r(x: torch.Tensor) -> torch.Tensor:
    """round to bf16 and back: test inputs are made bf16-representable so that the fp32 oracle and the bf16
    MFMA path consume IDENTICAL operand values."""
    return x.to(torch.bfloat16).to(torch.float32)


def bf16_floor(ref: torch.Tensor) -> float:
    """relative Frobenius error of merely ROUNDING the exact result to bfloat16 — the best any bf16-stored output can do
    (1.66e-3 for Gaussian-like data).  bf16-output kernels are required to stay within 15 % of it."""
    return rel(bf16r(ref.float()), ref)


def h16r(x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """round to the 16-bit format `dt` (torch.bfloat16 | torch.float16) and back to f32: bf16r for either operand format"""
    return x.to(dt).to(torch.float32)


def floor16(ref: torch.Tensor, dt: torch.dtype) -> float:
    """relative Frobenius error of merely ROUNDING the exact result to `dt`: bf16_floor for either format.  torch's CPU cast rounds to nearest even and
    keeps fp16 subnormals (and overflows to inf), so the floor stays the right yardstick for outputs in fp16's subnormal range."""
    return rel(h16r(ref.float(), dt), ref)


def disc_case(golden_npz):
    """the discriminator golden case of oracle/make_golden_disc.py: module (CPU parameters regenerated from the seed), real, fake"""
    from enhancing.losses.layers import StyleDiscriminator
    size, B = int(golden_npz["size"]), int(golden_npz["B"])
    torch.manual_seed(int(golden_npz["param_seed"]))
    D = StyleDiscriminator(size=size)
    with torch.no_grad():
        for n, p in D.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape))
    g = torch.Generator().manual_seed(int(golden_npz["data_seed"]))
    real = torch.rand(B, 3, size, size, generator=g)
    fake = (real + 0.1 * torch.randn(B, 3, size, size, generator=g)).clamp(0, 1)
    return D, real, fake


# ---------------------------------------------------------------------------------------------
# local error metrics: a bound per ELEMENT and an error per ROW (rel() above is one number for the whole tensor and cannot see an error that is
# large but local: a tile's last row or column, the last K stage, a split-K slab boundary, the last key tile of an attention row, a border pixel)
# ---------------------------------------------------------------------------------------------
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # unit roundoff of the stored format (half an ulp, relative, round to nearest)
SUB16 = {torch.float16: 2.0 ** -25}                                 # half the subnormal spacing (fp16: 2^-24); bf16 shares f32's exponent range
TANH_ABS = 4 * 2.0 ** -24


def elem_bound(ref: torch.Tensor, mag: torch.Tensor, k: int, dt=None, extra_abs: float = 0.0) -> torch.Tensor:
    """per-element limit of |out - ref| for a kernel that sums `k` products in f32 and rounds ONCE to the stored format `dt` (None / torch.float32:
    the f32 sum is stored as it is):

        u(dt) |ref| + sub(dt) + (2k + 8) 2^-24 mag + extra_abs

    `mag` is the same operation on absolute values (a GEMM: |A| |B| + |bias| + |res| + |C_old|; a convolution: conv(|x|, |w|)) with the epilogue's
    derivative factors (all <= 1) applied.  (2k + 8) 2^-24: gamma_k = k 2^-24 bounds an f32 sum of k terms in ANY order, doubled because the order
    inside an MFMA is not documented, plus a few epilogue operations; it holds for split-K slabs and atomics as well.  Nothing here is measured.
    extra_abs: TANH_ABS = 4 * 2^-24 = 2.4e-7 for the transcendental-unit tanh epilogue 1 - 2 / (exp2(c x) + 1), whose absolute error csrc/gemm_tiles.h
    states as about 1e-7.  On MI355X the worst element of the honest bias + tanh kernels uses 0.86 of the bound with this term (every family, layout
    and format of tests/test_elementwise_gpu.py), so no larger, measured figure was needed."""
    ref, mag = ref.detach().double().cpu(), mag.detach().double().cpu()
    b = (2 * k + 8) * 2.0 ** -24 * mag + extra_abs
    if dt in U16:
        b = b + U16[dt] * ref.abs() + SUB16.get(dt, 0.0)
    return b


def assert_elementwise(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str, tile=None) -> float:
    """every element of `out` within `bound` of `ref`; fails with the number of violations, the worst element's index, its coordinates inside a
    `tile` of the last two axes (e.g. (256, 256)) and err / bound.  Returns max(err / bound)."""
    out, ref, bound = out.detach().double().cpu(), ref.detach().double().cpu(), bound.detach().double().cpu()
    assert out.shape == ref.shape == bound.shape, (what, out.shape, ref.shape, bound.shape)
    err = (out - ref).abs()
    bad = ~(err <= bound)                                          # (a NaN anywhere is a violation)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = ratio.max().item()
    if bool(bad.any()):
        flat = int(ratio.argmax())
        idx = []
        for d in reversed(out.shape):
            idx.append(flat % d)
            flat //= d
        idx = tuple(reversed(idx))
        where = f"worst at {idx}"
        if tile is not None and len(idx) >= 2:
            where += f" = ({idx[-2] % tile[0]}, {idx[-1] % tile[1]}) inside its {tile[0]} x {tile[1]} tile"
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the element bound, {where}: out {out[idx].item():.9g} "
                             f"ref {ref[idx].item():.9g} err / bound = {worst:.3g}")
    return worst


def row_err(x: torch.Tensor, ref: torch.Tensor, width: int) -> torch.Tensor:
    """for each row of `width` elements: ||x_r - ref_r|| / rms_r'(||ref_r'||).  The row's error is normalised by the RMS row norm of the tensor it
    belongs to, not by its own norm: rows with a small gradient otherwise dominate (worst honest row 9e-2 against a median of 2e-3)."""
    x, ref = x.detach().double().cpu().reshape(-1, width), ref.detach().double().cpu().reshape(-1, width)
    norms = ref.norm(dim=1)
    return (x - ref).norm(dim=1) / norms.pow(2).mean().sqrt().clamp_min(1e-300)


def attn_model(qkv: torch.Tensor, do: torch.Tensor, B: int, N: int, H: int, scale: float, dt: torch.dtype, compute=torch.float64, out=None, lse=None):
    """CPU model of the fused attention (dim_head 64, qkv packed [B, N, 3 H 64] as include/enh_hip.h): arithmetic in `compute` (fp64: the model the
    kernels are compared with) except the roundings to the 16-bit format `dt` that the kernels make:
      forward : exp(s - max) to 16 bits before P V (the normaliser is the sum of the unrounded numerators); one rounding of out
      backward: P = exp(s - lse) to 16 bits before P^T dO; p o (dP - delta) to 16 bits before the dQ / dK products, delta = rowsum(dO o out) on the
                STORED out; one rounding of each gradient.
    `out` [B,N,H*64] / `lse` [B,H,N]: what the backward is GIVEN (enh_attention_backward takes the forward's stored results as inputs: a model of it
    starts from the same ones); default: the model's own forward.
    Returns out [B,N,H*64], lse [B,H,N], dq, dk, dv [B,N,H*64] (`compute` dtype, values representable in dt)."""
    def r(t):
        return t.to(dt).to(compute)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, H * 64)
    heads = lambda t: t.to(compute).view(B, N, H, 64).permute(0, 2, 1, 3)
    q, k, v = qkv.to(compute).view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
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


def attn_ref64(qkv: torch.Tensor, do: torch.Tensor, B: int, N: int, H: int, scale: float):
    """plain fp64 attention of the packed qkv and its autograd: out [B,N,H*64], lse [B,H,N], P |V| (the magnitude term of the forward's element bound),
    (dq, dk, dv)"""
    qt = qkv.double().clone().requires_grad_(True)
    q, k, v = qt.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    out = (p @ v).permute(0, 2, 1, 3).reshape(B, N, H * 64)
    out.backward(do.double())
    pav = (p.detach() @ v.detach().abs()).permute(0, 2, 1, 3).reshape(B, N, H * 64)
    return out.detach(), torch.logsumexp(s.detach(), dim=-1), pav, qt.grad.view(B, N, 3, H * 64).unbind(2)


def attn_out_bound(ref: torch.Tensor, pav: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """element bound of the fused attention's output: u |ref| (the one rounding of the store) + (u + 2^-20) P |V| (every probability rounded to 16 bits
    before P V: relative error u each, whatever the signs; 2^-20: the exp2 / f32 row-sum error of the softmax)"""
    return U16[dt] * ref.abs() + (U16[dt] + 2.0 ** -20) * pav


def worst_rows(got, ref, H: int) -> float:
    """worst row_err of a [B, N, H*64] tensor over its 64-wide rows, each head normalised by its own RMS row norm.  A non-finite element anywhere (a row
    the kernel never wrote into a NaN-filled buffer) gives nan: compare with `not (x <= limit)`, or see assert_rows_within."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return torch.stack([row_err(got[..., h * 64:(h + 1) * 64], ref[..., h * 64:(h + 1) * 64], 64).max() for h in range(H)]).max().item()     # (torch's max keeps a NaN)


def assert_rows_within(got, ref, H: int, limit: float, what: str) -> float:
    """every 64-wide row of every head finite and worst_rows(got, ref) <= limit; fails naming the first non-finite row (batch, token, head)"""
    g = got.detach().double().cpu()
    bad = ~torch.isfinite(g.reshape(*g.shape[:-1], H, 64)).all(-1)
    if bool(bad.any()):
        b, n, h = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} rows hold non-finite values, the first at batch {b}, token {n}, head {h}")
    w = worst_rows(got, ref, H)
    assert w <= limit, f"{what}: worst row {w:.3e} beyond {limit:.3e}"
    return w
