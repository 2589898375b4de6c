"""The MXFP6 weight operand (include/enh_hip.h: e2m3 codes in 128-k chunks of 96 bytes, one E8M0 scale per 32 consecutive k of a row) in plain torch
on the CPU: the specification the device quantizer is held to bit for bit, and the exact dequantization the products are compared against.  Built
from the 32-value grid, the tie rule and the stated bit positions alone; no torch fp6 dtype is involved."""
import torch

BLOCK = 32
CHUNK_K, CHUNK_BYTES = 128, 96
# the magnitudes of codes 0 .. 31: m / 8 for e = 0, 2^(e - 1) (1 + m / 8) for e = 1 .. 3
GRID = torch.tensor([m / 8 if e == 0 else 2.0 ** (e - 1) * (1 + m / 8) for e in range(4) for m in range(8)])
MID = (GRID[:-1] + GRID[1:]) / 2                                   # exact in f32
TIE_UP = torch.arange(31) % 2 == 1                                 # a value exactly at MID[i] goes to the even code of i, i + 1
NAN_SCALE = 0xFF


def row_bytes(K):
    return CHUNK_BYTES * ((K + CHUNK_K - 1) // CHUNK_K)


def _bit_index(K):
    """[K] int64: the bit of a row at which the six bits of the code of k start.  k = 128 c + 32 i + 8 q + e is position j = 8 i + e of piece q of
    chunk c; bits [6 j, 6 j + 6) of the piece, whose bits 0 .. 127 are the chunk's bytes [16 q, 16 q + 16) and bits 128 .. 191 its bytes
    [64 + 8 q, 64 + 8 q + 8).  A code may straddle the two parts (j = 21: bits 126 .. 131)."""
    k = torch.arange(K)
    c, i, q, e = k // 128, (k // 32) % 4, (k // 8) % 4, k % 8
    return c, q, 6 * (8 * i + e)


def _piece_bit_to_row_bit(c, q, pb):
    """the bit of the row that holds bit `pb` of piece q of chunk c"""
    return torch.where(pb < 128, (96 * c + 16 * q) * 8 + pb, (96 * c + 64 + 8 * q) * 8 + pb - 128)


def pack(code):                                 # [N, K] int64 codes 0 .. 63, k ascending -> [N, 96 ceil(K / 128)] uint8
    N, K = code.shape
    c, q, b0 = _bit_index(K)
    bits = torch.zeros(N, row_bytes(K) * 8, dtype=torch.int64)
    for t in range(6):
        bits[:, _piece_bit_to_row_bit(c, q, b0 + t)] = (code >> t) & 1
    return (bits.view(N, -1, 8) << torch.arange(8)).sum(-1).to(torch.uint8)


def unpack(q8):                                 # [N, 96 ceil(K / 128)] uint8 -> [N, 128 ceil(K / 128)] int64 codes, k ascending
    N = q8.shape[0]
    K = q8.shape[1] // CHUNK_BYTES * CHUNK_K
    bits = ((q8.long()[..., None] >> torch.arange(8)) & 1).view(N, -1)
    c, q, b0 = _bit_index(K)
    return sum(bits[:, _piece_bit_to_row_bit(c, q, b0 + t)] << t for t in range(6))


def quant(w):                                   # w [N, K] f32, K % 32 == 0
    """(codes [N, 96 ceil(K / 128)] uint8, scales [N, K / 32] uint8).  Per block: X = clamp(floor(log2 amax) - 2, -127, 127), 0 for an all-zero
    block; y = |w| 2^-X (exact: a power of two, X <= 125 for finite input); code = the number of midpoints below y, a tie going to the even code,
    which saturates everything above 7.25 to code 31 = 7.5; the sign bit of w, of -0.0 too, is bit 5.  A block that holds a NaN or an infinity gets
    the scale byte 0xff, the format's NaN, and all-zero codes.  The codes of k >= K in a partial last chunk are 0."""
    N, K = w.shape
    b = w.view(N, -1, BLOCK)
    bad = ~torch.isfinite(b).all(-1)
    b = torch.where(bad[..., None], torch.zeros(()), b)
    amax = b.abs().amax(-1)
    X = (torch.frexp(amax).exponent - 1 - 2).clamp(-127, 127)
    X[amax == 0] = 0
    y = torch.ldexp(b.abs(), -X[..., None])
    mag = ((y[..., None] > MID) | ((y[..., None] == MID) & TIE_UP)).sum(-1)
    code = (mag | (torch.signbit(b).long() << 5)).view(N, K)
    scales = (X + 127).to(torch.uint8)
    scales[bad] = NAN_SCALE
    return pack(code), scales


def dequant(q8, s):                             # exact in f32
    """f32 [N, K], K = 32 x the width of s: e2m3(code) 2^(s - 127); NaN throughout a block whose scale byte is 0xff"""
    K = s.shape[1] * BLOCK
    c = unpack(q8)[:, :K]
    v = GRID[c & 31] * (1.0 - 2.0 * (c >> 5).float())
    d = torch.ldexp(v.view(q8.shape[0], -1, BLOCK), (s.int() - 127)[..., None])
    return torch.where((s == NAN_SCALE)[..., None], torch.full((), float("nan")), d).view(q8.shape[0], -1)


BLOCK_LINEARS = ("attn.query.weight", "attn.key.weight", "attn.value.weight", "attn.proj.weight", "mlp.p0.weight", "mlp.p1.weight")


def quantized_params(P: dict) -> dict:
    """P with every Linear weight of every Block replaced by dequant(quant(W)); the head, biases, LayerNorms and embeddings untouched"""
    return {k: dequant(*quant(v.float().contiguous())) if k.endswith(BLOCK_LINEARS) else v for k, v in P.items()}
