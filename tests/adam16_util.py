"""What the bf16-moment tests share (tests/test_adam16_cpu.py, test_adam16_kernel_gpu.py, test_gpt_train_adam16_gpu.py): host restatements, in plain
torch / numpy, of what include/enh_hip.h states for enh_adam_step_segments_s16:

    stored_round    the stored rounding of an f32 bit pattern with a 16-bit word, on integer views
    philox4x32_10   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), vectorised over counters
    philox_words    the [n] word array of (seed, t): group G = e / 4 takes one call with counter (G lo, G hi, t lo, t hi); word k serves element 4G + k
    adam_step_from  one Adam step in the dtype of its operands (fp64 for the reference) starting from given moments

and the f32 allowance of tests/gpt_train_util.py's rule for one tensor (4 x torch's f32 error against fp64 + one f32 ulp)."""
import numpy as np
import torch

import gpt_train_util as TU

BF16_MAX = 0x7F7F


def f32_bits(x: torch.Tensor) -> torch.Tensor:
    """f32 tensor -> its bit patterns as non-negative int64"""
    return x.detach().cpu().float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    """bf16 tensor -> its bit patterns as int64 in [0, 65535]"""
    return x.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def bf16_from_bits(h: torch.Tensor) -> torch.Tensor:
    """int64 bit patterns in [0, 65535] -> the bf16 tensor"""
    h = h.to(torch.int64)
    return torch.where(h >= 0x8000, h - 0x10000, h).to(torch.int16).view(torch.bfloat16)


def decode16(h: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns (int64) -> fp64 values: the exact widening bf16 << 16"""
    u = (h.to(torch.int64) << 16)
    return torch.where(u >= 0x80000000, u - 0x100000000, u).to(torch.int32).view(torch.float32).double()


def stored_round(u: torch.Tensor, r) -> torch.Tensor:
    """u: f32 bit patterns (int64, 0 .. 2^32 - 1); r: a 16-bit word per element (int64 tensor or int) -> the stored bf16 bit patterns (int64).
    Finite: (u + r) >> 16, and where that carries into the all-ones exponent the largest finite bf16 of the sign.  inf: truncated.  nan: truncated with
    the quiet bit set."""
    u = u.to(torch.int64)
    r = torch.as_tensor(r, dtype=torch.int64) & 0xFFFF
    a = u & 0x7FFFFFFF
    h = (u + r) >> 16
    h = torch.where((h & 0x7FFF) >= 0x7F80, (h & 0x8000) | BF16_MAX, h)
    special = (u >> 16) | torch.where(a > 0x7F800000, 0x40, 0)
    return torch.where(a >= 0x7F800000, special, h)


_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(key, ctr: np.ndarray) -> np.ndarray:
    """key: (k0, k1); ctr: uint32 [..., 4] -> uint32 [..., 4]"""
    c = [ctr[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_words(seed: int, t: int, n: int) -> torch.Tensor:
    """the kernel's words for step count t (after the advance) as an int32 [n] tensor (n % 4 == 0): what sr_words takes"""
    assert n % 4 == 0
    G = np.arange(n // 4, dtype=np.uint64)
    ctr = np.stack([G & np.uint64(0xFFFFFFFF), G >> np.uint64(32), np.full_like(G, t & 0xFFFFFFFF), np.full_like(G, (t >> 32) & 0xFFFFFFFF)], axis=-1)
    w = philox4x32_10((seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), ctr.astype(np.uint32)).reshape(-1)
    return torch.from_numpy(w.view(np.int32).copy())


def word_halves(words: torch.Tensor):
    """int32 [n] words -> (r_m, r_v): the low halves round m, the high halves v (int64)"""
    w = words.to(torch.int64) & 0xFFFFFFFF
    return w & 0xFFFF, w >> 16


def adam_step_from(p, g, m, v, t: int, lr: float, wd, betas=TU.BETAS, eps: float = TU.EPS):
    """one step of gpt_train_util.adam_step64 from the given moments, out of place -> (p, m, v) in the operands' dtype"""
    p, m, v = p.clone(), m.clone(), v.clone()
    TU.adam_step64(p, g, m, v, t, lr, wd, betas=betas, eps=eps)
    return p, m, v


def f32_allowance(f32: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """per element: 4 x the worst element error of the f32 restatement against fp64 + that element's f32 ulp (gpt_train_util.check_limit's
    worst-element rule)"""
    ref64 = ref64.double()
    return 4.0 * (f32.double() - ref64).abs().max() + TU.ulp32(ref64)
