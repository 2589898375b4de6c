"""The MXFP4 weight operand (include/enh_hip.h: e2m1 codes, two to a byte, one E8M0 scale per 32 consecutive k of a row) in plain torch on the CPU:
the specification the device quantizer is held to bit for bit, and the exact dequantization the products are compared against.  Built from the
eight-value grid and the tie rule alone; no torch fp4 dtype is involved."""
import torch

BLOCK = 32
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])      # the magnitudes of codes 0 .. 7
MID = (GRID[:-1] + GRID[1:]) / 2                                   # 0.25 0.75 1.25 1.75 2.5 3.5 5: exact in f32
TIE_UP = torch.tensor([False, True, False, True, False, True, False])      # a value exactly at MID[i] goes to the even code of i, i + 1
NAN_SCALE = 0xFF


def quant(w):                                   # w [N, K] f32, K % 32 == 0
    """(codes [N, K / 2] uint8, scales [N, K / 32] uint8).  Per block: X = clamp(floor(log2 amax) - 2, -127, 127), 0 for an all-zero block;
    y = |w| 2^-X (exact: a power of two, X <= 125 for finite input); code = the number of midpoints below y, a tie going to the even code, which
    saturates everything above 5 to code 7 = 6; the sign bit of w, of -0.0 too, is bit 3.  k even sits in the low nibble.  A block that holds a
    NaN or an infinity gets the scale byte 0xff, the format's NaN, and all-zero codes."""
    N, K = w.shape
    b = w.view(N, -1, BLOCK)
    bad = ~torch.isfinite(b).all(-1)
    b = torch.where(bad[..., None], torch.zeros(()), b)
    amax = b.abs().amax(-1)
    X = (torch.frexp(amax).exponent - 1 - 2).clamp(-127, 127)
    X[amax == 0] = 0
    y = torch.ldexp(b.abs(), -X[..., None])
    mag = ((y[..., None] > MID) | ((y[..., None] == MID) & TIE_UP)).sum(-1)
    code = (mag | (torch.signbit(b).long() << 3)).view(N, K // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    scales = (X + 127).to(torch.uint8)
    scales[bad] = NAN_SCALE
    return codes, scales


def unpack(q):                                  # [N, K / 2] uint8 -> [N, K] int64 nibbles, k ascending
    return torch.stack([q & 0xF, q >> 4], -1).view(q.shape[0], -1).long()


def dequant(q, s):                              # exact in f32
    """f32 [N, K]: e2m1(nibble) 2^(s - 127); NaN throughout a block whose scale byte is 0xff"""
    c = unpack(q)
    v = GRID[c & 7] * (1.0 - 2.0 * (c >> 3).float())
    d = torch.ldexp(v.view(q.shape[0], -1, BLOCK), (s.int() - 127)[..., None])
    return torch.where((s == NAN_SCALE)[..., None], torch.full((), float("nan")), d).view(q.shape[0], -1)


BLOCK_LINEARS = ("attn.query.weight", "attn.key.weight", "attn.value.weight", "attn.proj.weight", "mlp.p0.weight", "mlp.p1.weight")


def quantized_params(P: dict) -> dict:
    """P with every Linear weight of every Block replaced by dequant(quant(W)); the head, biases, LayerNorms and embeddings untouched"""
    return {k: dequant(*quant(v.float().contiguous())) if k.endswith(BLOCK_LINEARS) else v for k, v in P.items()}
