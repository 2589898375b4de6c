"""The MXFP8 helper (tests/mxfp8_util.py) against itself and against the formats it feeds: quantization is idempotent, its crafted edge cases give
the codes the OCP rules name, and every dequantized weight of the gpt_cases parameter sets is a 16-bit value in either operand format, which is what
lets the emulation of tests/test_gpt_sample_fp8_gpu.py reuse gpt_cases.step_logits as it stands."""
import math

import pytest
import torch

import gpt_cases as GC
from mxfp8_util import BLOCK_LINEARS, dequant, quant, quantized_params


def _case_params(name):
    from enhancing.modules.stage2.layers import GPT
    return GC.make_params({k: tuple(v.shape) for k, v in GPT(**GC.case_kwargs(name)).state_dict().items()})


def _weights():
    g = torch.Generator().manual_seed(5)
    for N, K in [(8, 32), (24, 160), (40, 1088)]:
        yield torch.randn(N, K, generator=g) / math.sqrt(K)
    # wide block exponents, wide spread inside a block; amax stays a normal f32 (a block that the X = -127 clamp flushes to all zeros re-quantizes
    # to X = 0: the one case where a second pass changes the scale byte, and no weight is an f32 denormal)
    yield torch.randn(64, 256, generator=g) * torch.exp2(torch.randint(-100, 100, (64, 8), generator=g).float()).repeat_interleave(32, 1) \
        * torch.exp2(torch.randint(-14, 1, (64, 256), generator=g).float())


def test_quantization_is_idempotent():
    for w in _weights():
        q, s = quant(w.contiguous())
        q2, s2 = quant(dequant(q, s))
        assert torch.equal(q, q2) and torch.equal(s, s2)


@pytest.mark.parametrize("name", sorted(GC.CASES))
def test_idempotent_and_16_bit_exact_on_the_case_parameters(name):
    P = _case_params(name)
    n = 0
    for k, v in P.items():
        if not k.endswith(BLOCK_LINEARS):
            continue
        q, s = quant(v)
        d = dequant(q, s)
        q2, s2 = quant(d)
        assert torch.equal(q, q2) and torch.equal(s, s2), k
        for dt in (torch.float16, torch.bfloat16):      # 4 significant bits at an exponent inside either format's normal range
            assert torch.equal(d.to(dt).float(), d), (k, dt)
        n += 1
    assert n == 6 * GC.CASES[name][2]
    Q = quantized_params(P)
    assert torch.equal(Q["head.weight"], P["head.weight"]) and not torch.equal(Q["blocks.0.mlp.p0.weight"], P["blocks.0.mlp.p0.weight"])


def test_the_rules_on_crafted_blocks():
    w = torch.zeros(8, 32)
    w[1, :] = 2.0 ** -30; w[1, 3] = 2.0 ** -10                       # an outlier 2^20 times the rest: the rest flush to zero
    w[2, 0] = 0.25                                                   # amax a power of two: X = -2 - 8, code 256 = 0x78
    w[3, 0] = (1 - 2.0 ** -20) * 4.0                                 # just under 512 of its scale: saturates to 448
    w[4, 0] = 256.0; w[4, 1] = 2.0 ** -10; w[4, 2] = 1.5 * 2.0 ** -10; w[4, 3] = 17.0; w[4, 4] = 19.0; w[4, 5] = -0.0     # X = 0: ties
    w[5, 0] = 2.0 ** -140                                            # an f32 denormal: X clamps to -127
    w[6, 0] = 1.5 * 2.0 ** 127                                       # X = 119
    q, s = quant(w)
    assert s[:, 0].tolist() == [127, 127 - 18, 127 - 10, 127 - 7, 127, 0, 246, 127]
    assert q[0].eq(0).all()
    assert q[1, 3].item() == 0x78 and q[1].ne(0).sum().item() == 1
    assert q[2, 0].item() == 0x78
    assert q[3, 0].item() == 0x7e
    # 2^-10 is half the smallest subnormal: tie to even 0; 1.5 * 2^-10 lies between 2^-10 .. 2^-9, nearest 2^-9; 17 ties between 16 and 18 -> 16 (even
    # mantissa), 19 ties between 18 and 20 -> 20
    assert q[4, :6].tolist() == [0x78, 0x00, 0x01, 0x58, 0x5a, 0x80]
    assert q[5, 0].item() == torch.tensor(2.0 ** -13).to(torch.float8_e4m3fn).view(torch.uint8).item()
    assert q[6, 0].item() == torch.tensor(384.0).to(torch.float8_e4m3fn).view(torch.uint8).item()
    assert not bool(((q & 0x7f) == 0x7f).any())                      # no NaN code from finite input
