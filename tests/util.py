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
