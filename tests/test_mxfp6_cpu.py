"""The MXFP6 helper (tests/mxfp6_util.py) against the OCP rules on hand-made blocks, against the stated layout bit by bit, against itself on weights
already on the grid, and against the formats it feeds: every dequantized weight of the gpt_cases parameter sets is a 16-bit value in either operand
format, which is what lets the emulation of tests/test_gpt_sample_fp6_gpu.py reuse gpt_cases.step_logits as it stands.  The last test prints what the
format costs on those random Gaussian models beside MXFP8 and MXFP4 (DESIGN.md §3.16 carries the table); it asserts no limit."""
import math

import pytest
import torch

import gpt_cases as GC
import mxfp4_util
import mxfp8_util
from mxfp6_util import BLOCK_LINEARS, GRID, MID, dequant, quant, quantized_params, row_bytes, unpack

UP, DOWN = torch.tensor(9.0), torch.tensor(-9.0)


def special_blocks():
    """{name: (block [32] f32, scale byte, {k: code})}: the blocks the rules are stated on; tests/test_mxfp6_kernels_gpu.py embeds them in a row"""
    S = {}
    z = lambda: torch.zeros(32)
    # every tie of the grid: the 31 midpoints, the largest (7.25) makes amax so X = 0 and the scaled values are the values.  Midpoint i lies between
    # codes i and i + 1 and goes to the even one
    even = [i + (i % 2) for i in range(31)]
    b = z(); b[:31] = MID
    S["ties+"] = (b, 127, {i: c for i, c in enumerate(even)})
    b = z(); b[:31] = -MID
    S["ties-"] = (b, 127, {i: c | 32 for i, c in enumerate(even)})
    # beside a tie, not on it: one f32 step to either side of 0.0625, 0.9375 (the subnormal / normal seam), 1.9375, 3.875 and 7.25
    b = z(); b[0] = 4.0
    exp = {0: 24}
    for n, i in enumerate((0, 7, 15, 23, 30)):      # 7: 0.9375 between 0.875 and 1; 15: 1.9375 below 2; 23: 3.875 below 4 (where the step widens)
        b[1 + 2 * n], b[2 + 2 * n] = torch.nextafter(MID[i], DOWN), -torch.nextafter(MID[i], UP)
        exp[1 + 2 * n], exp[2 + 2 * n] = i, (i + 1) | 32
    S["beside"] = (b, 127, exp)
    # amax just under 8 -> X = 0, scaled values in (7.5, 8) saturate to 7.5, the tie 7.75 too; 7.25 is the last tie below and goes down to 7
    b = z(); b[0] = 8.0 * (1 - 2.0 ** -20); b[1] = -7.75; b[2] = 7.6; b[3] = 7.5; b[4] = 7.25; b[5] = 7.2500005; b[6] = -7.9999
    S["saturate"] = (b, 127, {0: 31, 1: 63, 2: 31, 3: 31, 4: 30, 5: 31, 6: 63})
    # amax exactly 4 2^e, 7.5 2^e, just under 8 2^e, e = -9: X = -9 for all three
    e = 2.0 ** -9
    b = z(); b[3] = -4.0 * e; b[4] = 1.0 * e
    S["amax4"] = (b, 127 - 9, {3: 24 | 32, 4: 8})
    b = z(); b[3] = 7.5 * e; b[4] = 3.0 * e
    S["amax7.5"] = (b, 127 - 9, {3: 31, 4: 20})
    b = z(); b[3] = 8.0 * e * (1 - 2.0 ** -22); b[4] = 0.125 * e
    S["amax8-"] = (b, 127 - 9, {3: 31, 4: 1})
    # amax = 2^e exactly: X = e - 2, amax is code 24 (4.0)
    b = z(); b[31] = 2.0 ** 20
    S["pow2"] = (b, 127 + 18, {31: 24, 0: 0})
    S["zero"] = (z(), 127, {k: 0 for k in range(32)})
    b = z(); b[0] = 1.0; b[1] = -0.0; b[2] = -0.1            # -0.0 keeps its sign; -0.1 2^2 = -0.4 -> -0.375
    S["negzero"] = (b, 127 - 2, {0: 24, 1: 32, 2: 3 | 32, 3: 0})
    # f32 denormals: X clamps to -127, y = w 2^127: 2^-128 -> 0.5, 2^-140 -> 2^-13 -> 0, 3 2^-128 -> 1.5, 2^-130 -> 0.125, 2^-131 -> the tie 0.0625 -> 0
    b = z(); b[0] = 2.0 ** -128; b[1] = 2.0 ** -140; b[2] = -3 * 2.0 ** -128; b[3] = 2.0 ** -130; b[4] = 2.0 ** -131
    S["denormal"] = (b, 0, {0: 4, 1: 0, 2: 12 | 32, 3: 1, 4: 0})
    # the smallest normals clamp too: 2^-126 has floor(log2) - 2 = -128 -> X = -127, y = 2 -> code 16
    b = z(); b[0] = 2.0 ** -126; b[1] = 2.0 ** -125
    S["clamp"] = (b, 0, {0: 16, 1: 24})
    b = z(); b[0] = -1.9 * 2.0 ** 127; b[1] = 2.0 ** 126    # X = 125: y = -7.6 saturates, 2^126 2^-125 = 2
    S["huge"] = (b, 252, {0: 63, 1: 16})
    return S


def test_the_grid():
    assert GRID.tolist() == [0, .125, .25, .375, .5, .625, .75, .875, 1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
                             2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4, 4.5, 5, 5.5, 6, 6.5, 7, 7.5]


def test_the_rules_on_hand_made_blocks():
    S = special_blocks()
    w = torch.stack([b for b, _, _ in S.values()])
    q, s = quant(w)
    c = unpack(q)
    for i, (name, (_, scale, exp)) in enumerate(S.items()):
        assert s[i, 0].item() == scale, (name, s[i, 0].item(), scale)
        for k, code in exp.items():
            assert c[i, k].item() == code, (name, k, c[i, k].item(), code)
    assert bool((c[:, 32:] == 0).all())        # K = 32: three quarters of the one chunk are padding


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
    cb, rb = unpack(q)[:, :96].view(3, 3, 32), unpack(ref_q)[:, :96].view(3, 3, 32)
    assert bool((cb[bad] == 0).all()) and torch.equal(cb[~bad], rb[~bad])
    d = dequant(q, s).view(3, 3, 32)
    assert bool(d[bad].isnan().all()) and bool(torch.isfinite(d[~bad]).all())


def test_grid_weights_are_lossless():
    g = torch.Generator().manual_seed(3)
    N, K = 16, 160
    c = torch.randint(0, 64, (N, K), generator=g)
    c.view(N, -1, 32)[..., 0] = 31                                  # every block holds a 7.5, so X is the block's own exponent
    X = torch.randint(-120, 120, (N, K // 32), generator=g)
    w = torch.ldexp((GRID[c & 31] * (1.0 - 2.0 * (c >> 5).float())).view(N, -1, 32), X[..., None]).view(N, K)
    q, s = quant(w)
    assert tuple(q.shape) == (N, 192) and torch.equal(s.long(), X + 127)
    assert torch.equal(unpack(q)[:, :K], c) and bool((unpack(q)[:, K:] == 0).all())
    d = dequant(q, s)
    assert torch.equal(d, w) and torch.equal(torch.signbit(d), torch.signbit(w))      # -0.0 too


def _piece(row, c, q):
    """piece q of chunk c of a row of bytes as a python integer, from the stated byte ranges"""
    lo = bytes(row[96 * c + 16 * q: 96 * c + 16 * q + 16].tolist())
    hi = bytes(row[96 * c + 64 + 8 * q: 96 * c + 64 + 8 * q + 8].tolist())
    return int.from_bytes(lo, "little") | (int.from_bytes(hi, "little") << 128)


@pytest.mark.parametrize("K, ks", [(32, (0, 7, 8, 21, 31)), (160, (0, 69, 85, 127, 128, 159)), (256, (63, 64, 77, 200, 255))])
def test_the_layout_bit_by_bit(K, ks):
    """stated without the helper's packing: one code of all six bits (-7.5 = 63) at a known k sets exactly bits [6 j, 6 j + 6) of piece (c, q),
    c = k / 128, q = k / 8 % 4, j = 8 (k / 32 % 4) + k % 8, and nothing else of the row.  k = 69 and 77 are position 21, whose code straddles the
    16-byte and the 8-byte part of the piece"""
    assert row_bytes(K) == 96 * -(-K // 128)
    for k in ks:
        w = torch.zeros(1, K)
        w[0, k] = -7.5
        q8, s = quant(w)
        assert tuple(q8.shape) == (1, row_bytes(K)) and s[0, k // 32].item() == 127
        row = q8[0]
        c, q, j = k // 128, (k // 8) % 4, 8 * ((k // 32) % 4) + k % 8
        want = torch.zeros(row_bytes(K), dtype=torch.uint8)
        for bit in range(6 * j, 6 * j + 6):
            byte = 96 * c + 16 * q + bit // 8 if bit < 128 else 96 * c + 64 + 8 * q + (bit - 128) // 8
            want[byte] |= 1 << (bit % 8)
        assert int(sum(bin(v).count("1") for v in row.tolist())) == 6 and torch.equal(row, want), (K, k, row.nonzero().flatten().tolist())
        assert _piece(row, c, q) == 63 << (6 * j)
    # a full row: every position of every piece is its k's code, and what lies past K is zero
    w = torch.randn(1, K, generator=torch.Generator().manual_seed(K))
    q8, s = quant(w)
    code = unpack(q8)[0]
    for c in range(-(-K // 128)):
        for q in range(4):
            P = _piece(q8[0], c, q)
            for j in range(32):
                k = 128 * c + 32 * (j // 8) + 8 * q + j % 8
                assert (P >> (6 * j)) & 63 == (code[k].item() if k < K else 0), (c, q, j)
    if K == 160:        # the second chunk holds one block: positions 8 .. 31 of its four pieces, three quarters of its 96 bytes, are zero
        assert all(_piece(q8[0], 1, q) >> 48 == 0 for q in range(4)) and any(_piece(q8[0], 1, q) for q in range(4))


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
        for dt in (torch.float16, torch.bfloat16):      # 4 significant bits at an exponent inside either format's normal range
            assert torch.equal(d.to(dt).float(), d), (k, dt)
        n += 1
    assert n == 6 * GC.CASES[name][2]
    Q = quantized_params(P)
    assert torch.equal(Q["head.weight"], P["head.weight"]) and not torch.equal(Q["blocks.0.mlp.p0.weight"], P["blocks.0.mlp.p0.weight"])


def test_sample_weights_takes_fp6():
    from enhancing.modules.stage2.prior import QUANT_WEIGHTS, SAMPLE_WEIGHTS, Prior
    assert "fp6" in SAMPLE_WEIGHTS and QUANT_WEIGHTS["fp6"] == "MXFP6"
    assert Prior._sample_weights("fp6", True, "T") == "fp6"
    with pytest.raises(ValueError, match=r'T: weights="fp6" streams MXFP6 weights against 16-bit activations.*use_fp16=False'):
        Prior._sample_weights("fp6", False, "T")
    with pytest.raises(ValueError, match="int6"):
        Prior._sample_weights("int6", True, "T")


@pytest.mark.parametrize("name", ["tiny", "hs384", "h3"])
def test_print_what_the_format_costs(name):
    """relative weight and logit shift and KL(p || p_q) of the quantized model against the unquantized one, fp64, on the case's random Gaussian
    weights, for MXFP6 beside MXFP8 and MXFP4 from this same function.  A table for DESIGN.md, no limit: nobody has measured the formats on trained
    weights.  Measured: fp6 weights 0.028, logits 0.036 - 0.046; fp8 weights 0.028 - 0.031, logits 0.036 - 0.049; fp4 weights 0.113 - 0.116, logits
    0.14 - 0.19."""
    P = _case_params(name)
    conds, forced = GC.make_inputs(name)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    lp = GC.step_logits(P, name, conds, forced, work=torch.float64)
    p = torch.log_softmax(lp.double(), -1)
    for fmt, util in (("MXFP8", mxfp8_util), ("MXFP6", __import__("mxfp6_util")), ("MXFP4", mxfp4_util)):
        Q = util.quantized_params(P)
        wshift = [rel(Q[k], P[k]) for k in P if k.endswith(BLOCK_LINEARS)]
        lq = GC.step_logits(Q, name, conds, forced, work=torch.float64)
        pq = torch.log_softmax(lq.double(), -1)
        kl = float((p.exp() * (p - pq)).sum(-1).mean())
        print(f"{fmt} format shift, {name}: weights {min(wshift):.3f} .. {max(wshift):.3f}, logits {rel(lq, lp):.3f}, KL {kl:.2e} nats per token")
        assert math.isfinite(kl)
