"""The MXFP8 weight operand (include/enh_hip.h: e4m3fn codes, one E8M0 scale per 32 consecutive k of a row) in plain torch on the CPU: the
specification the device quantizer is held to bit for bit, and the exact dequantization the products are compared against."""
import torch

BLOCK = 32


def quant(w):                                   # w [N, K] f32, K % 32 == 0
    """(codes [N, K] uint8, scales [N, K / 32] uint8).  Per block: X = clamp(floor(log2 amax) - 8, -127, 127), 0 for an all-zero block; the clamp
    to +-448 followed by torch's CPU cast is round-to-nearest-even with saturation"""
    b = w.view(w.shape[0], -1, BLOCK)
    amax = b.abs().amax(-1)
    X = (torch.frexp(amax).exponent - 1 - 8).clamp(-127, 127)
    X[amax == 0] = 0
    y = torch.ldexp(b, -X[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return y.view(w.shape).view(torch.uint8), (X + 127).to(torch.uint8)


def dequant(q, s):                              # exact in f32
    """f32 [N, K]: e4m3(q) 2^(s - 127)"""
    return torch.ldexp(q.view(torch.float8_e4m3fn).float().view(q.shape[0], -1, BLOCK), (s.int() - 127)[..., None]).view(q.shape)


BLOCK_LINEARS = ("attn.query.weight", "attn.key.weight", "attn.value.weight", "attn.proj.weight", "mlp.p0.weight", "mlp.p1.weight")


def quantized_params(P: dict) -> dict:
    """P with every Linear weight of every Block replaced by dequant(quant(W)); the head, biases, LayerNorms and embeddings untouched"""
    return {k: dequant(*quant(v.float().contiguous())) if k.endswith(BLOCK_LINEARS) else v for k, v in P.items()}
