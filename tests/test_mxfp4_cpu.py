"""The MXFP4 helper (tests/mxfp4_util.py) against the OCP rules on hand-made blocks, against itself on weights already on the grid, and against the
formats it feeds: every dequantized weight of the gpt_cases parameter sets is a 16-bit value in either operand format, which is what lets the
emulation of tests/test_gpt_sample_fp4_gpu.py reuse gpt_cases.step_logits as it stands.  The last test prints what the format costs on those random
Gaussian models (DESIGN.md §3.15 carries the table); it asserts no limit."""
import math

import pytest
import torch

import gpt_cases as GC
from mxfp4_util import BLOCK_LINEARS, GRID, dequant, quant, quantized_params, unpack


def special_blocks():
    """{name: (block [32] f32, scale byte, {k: nibble})}: the blocks the rules are stated on; tests/test_mxfp4_kernels_gpu.py embeds them in a row"""
    S = {}
    z = lambda: torch.zeros(32)
    # amax = 4 -> X = 0: the scaled values are the values; every tie of the grid, both signs
    b = z(); b[0] = 4.0
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]                       # 0, 1, 1, 2, 2, 4, 4
    for i, t in enumerate(ties):
        b[1 + i], b[8 + i] = t, -t
    b[15], b[16], b[17], b[18] = 0.2500001, 0.7499999, 4.9999995, 5.0000005      # beside a tie, not on it
    exp = {0: 6, 15: 1, 16: 1, 17: 6, 18: 7}
    exp.update({1 + i: c for i, c in enumerate(want)})
    exp.update({8 + i: c | 8 for i, c in enumerate(want)})
    S["ties"] = (b, 127, exp)
    # amax just under 8 -> X = 0, scaled values in (6, 8) saturate to 6
    b = z(); b[0] = 8.0 * (1 - 2.0 ** -20); b[1] = -7.0; b[2] = 6.5; b[3] = 6.0; b[4] = 5.5
    S["saturate"] = (b, 127, {0: 7, 1: 15, 2: 7, 3: 7, 4: 7})
    # amax exactly 4 2^e, 6 2^e, just under 8 2^e, e = -9: X = -9 for all three
    e = 2.0 ** -9
    b = z(); b[3] = -4.0 * e; b[4] = 1.0 * e
    S["amax4"] = (b, 127 - 9, {3: 14, 4: 2})
    b = z(); b[3] = 6.0 * e; b[4] = 3.0 * e
    S["amax6"] = (b, 127 - 9, {3: 7, 4: 5})
    b = z(); b[3] = 8.0 * e * (1 - 2.0 ** -22); b[4] = 0.5 * e
    S["amax8-"] = (b, 127 - 9, {3: 7, 4: 1})
    # amax = 2^e exactly: X = e - 2, amax is code 6 (4.0)
    b = z(); b[31] = 2.0 ** 20
    S["pow2"] = (b, 127 + 18, {31: 6, 0: 0})
    S["zero"] = (z(), 127, {k: 0 for k in range(32)})
    b = z(); b[0] = 1.0; b[1] = -0.0; b[2] = -0.1            # -0.0 keeps its sign; -0.1 2^2 = -0.4 -> -0.5
    S["negzero"] = (b, 127 - 2, {0: 6, 1: 8, 2: 9, 3: 0})
    # f32 denormals: X clamps to -127, y = w 2^127: 2^-128 -> 0.5, 2^-140 -> 2^-13 -> 0, 3 2^-128 -> 1.5
    b = z(); b[0] = 2.0 ** -128; b[1] = 2.0 ** -140; b[2] = -3 * 2.0 ** -128
    S["denormal"] = (b, 0, {0: 1, 1: 0, 2: 11})
    # the smallest normals clamp too: 2^-126 has floor(log2) - 2 = -128 -> X = -127, y = 2 -> code 4
    b = z(); b[0] = 2.0 ** -126; b[1] = 2.0 ** -125
    S["clamp"] = (b, 0, {0: 4, 1: 6})
    b = z(); b[0] = -1.9 * 2.0 ** 127; b[1] = 2.0 ** 126    # X = 125: y = -7.6 saturates, 2^126 2^-125 = 2
    S["huge"] = (b, 252, {0: 15, 1: 4})
    return S


def test_the_rules_on_hand_made_blocks():
    S = special_blocks()
    w = torch.stack([b for b, _, _ in S.values()])
    q, s = quant(w)
    c = unpack(q)
    for i, (name, (_, scale, exp)) in enumerate(S.items()):
        assert s[i, 0].item() == scale, (name, s[i, 0].item(), scale)
        for k, nib in exp.items():
            assert c[i, k].item() == nib, (name, k, c[i, k].item(), nib)


def test_non_finite_masters_make_a_nan_block():
    """the chosen behaviour: a block that holds an infinity or a NaN gets the scale byte 0xff, the format's NaN, and all-zero codes; it dequantizes to
    NaN throughout, and its neighbours are untouched"""
    w = torch.randn(3, 96, generator=torch.Generator().manual_seed(0))
    ref_q, ref_s = quant(w.clone())
    w[0, 40] = float("inf"); w[1, 3] = float("nan"); w[2, 95] = float("-inf")
    q, s = quant(w)
    bad = torch.zeros(3, 3, dtype=torch.bool)
    bad[0, 1] = bad[1, 0] = bad[2, 2] = True
    assert bool((s[bad] == 0xFF).all()) and torch.equal(s[~bad], ref_s[~bad])
    qb, rb = q.view(3, 3, 16), ref_q.view(3, 3, 16)
    assert bool((qb[bad] == 0).all()) and torch.equal(qb[~bad], rb[~bad])
    d = dequant(q, s).view(3, 3, 32)
    assert bool(d[bad].isnan().all()) and bool(torch.isfinite(d[~bad]).all())


def test_grid_weights_are_lossless_and_the_nibble_order():
    g = torch.Generator().manual_seed(3)
    N, K = 16, 160
    c = torch.randint(0, 16, (N, K), generator=g)
    c.view(N, -1, 32)[..., 0] = 7                                   # every block holds a 6, so X is the block's own exponent
    X = torch.randint(-120, 120, (N, K // 32), generator=g)
    w = torch.ldexp((GRID[c & 7] * (1.0 - 2.0 * (c >> 3).float())).view(N, -1, 32), X[..., None]).view(N, K)
    q, s = quant(w)
    assert torch.equal(s.long(), X + 127)
    assert torch.equal(unpack(q), c)
    d = dequant(q, s)
    assert torch.equal(d, w) and torch.equal(torch.signbit(d), torch.signbit(w))      # -0.0 too
    # k even in the low nibble, k odd in the high one
    w = torch.zeros(1, 32); w[0, 0] = 6.0; w[0, 1] = -1.0; w[0, 31] = 0.5
    q, s = quant(w)
    assert q[0, 0].item() == (0x7 | (0xA << 4)) and q[0, 15].item() == (0x1 << 4) and s[0, 0].item() == 127


def _case_params(name):
    from enhancing.modules.stage2.layers import GPT
    return GC.make_params({k: tuple(v.shape) for k, v in GPT(**GC.case_kwargs(name)).state_dict().items()})


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
        for dt in (torch.float16, torch.bfloat16):      # 2 significant bits at an exponent inside either format's normal range
            assert torch.equal(d.to(dt).float(), d), (k, dt)
        n += 1
    assert n == 6 * GC.CASES[name][2]
    Q = quantized_params(P)
    assert torch.equal(Q["head.weight"], P["head.weight"]) and not torch.equal(Q["blocks.0.mlp.p0.weight"], P["blocks.0.mlp.p0.weight"])


def test_sample_weights_takes_fp4():
    from enhancing.modules.stage2.prior import SAMPLE_WEIGHTS, Prior
    assert "fp4" in SAMPLE_WEIGHTS
    assert Prior._sample_weights("fp4", True, "T") == "fp4"
    with pytest.raises(ValueError, match=r'T: weights="fp4" streams MXFP4 weights against 16-bit activations.*use_fp16=False'):
        Prior._sample_weights("fp4", False, "T")
    with pytest.raises(ValueError, match="int4"):
        Prior._sample_weights("int4", True, "T")


@pytest.mark.parametrize("name", ["tiny", "hs384", "h3"])
def test_print_what_the_format_costs(name):
    """relative weight and logit shift and KL(p || p4) of the 4-bit model against the unquantized one, fp64, on the case's random Gaussian weights.
    A table for DESIGN.md, no limit: nobody has measured the format on trained weights."""
    P = _case_params(name)
    Q = quantized_params(P)
    conds, forced = GC.make_inputs(name)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    wshift = [rel(Q[k], P[k]) for k in P if k.endswith(BLOCK_LINEARS)]
    lp = GC.step_logits(P, name, conds, forced, work=torch.float64)
    lq = GC.step_logits(Q, name, conds, forced, work=torch.float64)
    p, p4 = torch.log_softmax(lp.double(), -1), torch.log_softmax(lq.double(), -1)
    kl = float((p.exp() * (p - p4)).sum(-1).mean())
    print(f"MXFP4 format shift, {name}: weights {min(wshift):.3f} .. {max(wshift):.3f}, logits {rel(lq, lp):.3f}, KL {kl:.2e} nats per token")
    assert math.isfinite(kl)
