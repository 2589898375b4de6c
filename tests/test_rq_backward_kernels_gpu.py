"""The three kernels the RQ prior's backward adds (csrc/rq_backward.hip; the strided LayerNorm backward: csrc/gpt_rows.hip), each against fp64 at the
limits the GPT's backward kernels are held to (tests/test_gpt_backward_kernels_gpu.py).  Outputs are pre-filled with NaN; NaN stands behind the inputs
and a sentinel behind the outputs."""
import pytest
import torch

from attn_causal_bwd_util import causal_bwd_model, causal_bwd_ref64
from attn_causal_util import ATT_MARGIN
from attn_dh_util import assert_rows_within, worst_rows
from util import assert_elementwise, elem_bound, h16r

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
WIDTHS = [64, 128, 192, 256, 320, 384]
SHAPES = [(1, 1, 1), (7, 2, 2), (33, 3, 1), (130, 4, 2), (5, 5, 3), (19, 8, 2)]      # test_rq_kernels_gpu.SHAPES: (NSEQ, L, H)
GUARD_ROWS = 64
SENTINEL = 12345.0
NAN = float("nan")


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _guarded(t, fill):
    """`t` at the FRONT of a larger allocation whose remainder, GUARD_ROWS rows of t's last axis, holds `fill`: (view of the front, the whole)"""
    whole = torch.empty(t.numel() + GUARD_ROWS * t.shape[-1], dtype=t.dtype, device="cuda")
    whole[:t.numel()] = t.reshape(-1).cuda()
    whole[t.numel():] = fill
    return whole[:t.numel()].view(t.shape), whole


def _attn_inputs(D, NSEQ, L, H, dt):
    g = torch.Generator().manual_seed(D * 1000 + NSEQ * 100 + L + H)
    return h16r(torch.randn(NSEQ, L, 3 * H * D, generator=g) * 1.5, dt), h16r(torch.randn(NSEQ, L, H * D, generator=g), dt)


def _forward(C, qkv, NSEQ, L, H, D, dt):
    qd, _ = _guarded(qkv.to(dt), NAN)
    out, _ = _guarded(torch.full((NSEQ, L, H * D), NAN, dtype=dt), NAN)
    lse, _ = _guarded(torch.full((NSEQ, H, L), NAN), NAN)
    C.short_causal_attention(qd, NSEQ, L, H, D, out, lse)
    return qd, out, lse


def _backward(C, qd, out, dod, lse, NSEQ, L, H, D, dt):
    dqkv, whole = _guarded(torch.full(tuple(qd.shape), NAN, dtype=dt), SENTINEL)
    C.short_causal_attention_backward(qd, out, dod, lse, NSEQ, L, H, D, dqkv)
    torch.cuda.synchronize()
    assert bool((whole[dqkv.numel():] == SENTINEL).all()), "wrote past dqkv"
    return dqkv


# ---- short-sequence causal attention backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", WIDTHS)
def test_short_attention_backward_against_fp64(C, D, shape, dt):
    NSEQ, L, H = shape
    scale = D ** -0.5
    qkv, do = _attn_inputs(D, NSEQ, L, H, dt)
    qd, out, lse = _forward(C, qkv, NSEQ, L, H, D, dt)
    dod, _ = _guarded(do.to(dt), NAN)
    runs = [_backward(C, qd, out, dod, lse, NSEQ, L, H, D, dt) for _ in range(2)]
    tile = torch.full(tuple(qd.shape), NAN, dtype=dt, device="cuda")
    C.causal_attention_backward(qd, out, dod, lse, NSEQ, L, H, D, tile)
    what = f"short causal attention backward D={D} NSEQ={NSEQ} L={L} H={H} {dt}"
    assert bool(torch.isfinite(runs[0].float()).all()), what + ": an element was never written"
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), what + ": two launches differ"
    got = [t.contiguous() for t in runs[0].view(NSEQ, L, 3, H * D).unbind(2)]
    got_tile = [t.contiguous() for t in tile.view(NSEQ, L, 3, H * D).unbind(2)]
    assert bool((got[0][:, 0] == 0).all()), what + ": row 0 of dQ is not exactly zero"
    if L == 1:      # one key: P = 1, dS = 0 whatever the values, and dV is dO itself
        assert bool((got[1] == 0).all()) and torch.equal(got[2].view(torch.int16), dod.view(torch.int16))
        return
    ref = causal_bwd_ref64(qkv, do, NSEQ, L, H, D, scale)
    model = causal_bwd_model(qkv, do, out, lse, NSEQ, L, H, D, scale, dt)
    ratios = []
    for name, t, tt, r_, m_ in zip(("dq", "dk", "dv"), got, got_tile, ref, model):
        m = worst_rows(m_, r_, H, D)
        assert m == m and m > 0, (what, name, m)
        ratios.append(assert_rows_within(t, r_, H, D, ATT_MARGIN * m, f"{what} {name}") / m)
        ratios.append(assert_rows_within(tt, r_, H, D, ATT_MARGIN * m, f"{what} {name} (the tile kernel at N = L)") / m)
    print(f"{what}: worst row / the model's worst row (short, tile): dq {ratios[0]:.3f} {ratios[1]:.3f} dk {ratios[2]:.3f} {ratios[3]:.3f} "
          f"dv {ratios[4]:.3f} {ratios[5]:.3f}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_sequences_of_a_pack_do_not_see_each_other(C, dt):
    """41 sequences of 3 heads: 123 pairs in four workgroups.  Sequence 13 gets other q, k, v and dout: every other sequence keeps its bits."""
    NSEQ, L, H, D = 41, 4, 3, 128
    qkv, do = _attn_inputs(D, NSEQ, L, H, dt)
    qkv2, do2 = qkv.clone(), do.clone()
    qkv2[13], do2[13] = h16r(qkv[13] * -1.75 + 0.5, dt), h16r(do[13] * 2.5 - 0.25, dt)
    res = []
    for q_, d_ in ((qkv, do), (qkv2, do2)):
        qd, out, lse = _forward(C, q_, NSEQ, L, H, D, dt)
        res.append(_backward(C, qd, out, d_.to(dt).cuda(), lse, NSEQ, L, H, D, dt))
    keep = [i for i in range(NSEQ) if i != 13]
    assert torch.equal(res[0][keep].view(torch.int16), res[1][keep].view(torch.int16))
    assert not torch.equal(res[0][13], res[1][13])
    assert bool(torch.isfinite(res[1].float()).all())


def test_unsupported_shapes_are_shape_errors(C):
    E_SHAPE = -2      # include/enh_hip.h ENH_E_SHAPE
    L_ = C.lib()
    z = torch.zeros(9 * 3 * 96, dtype=F16, device="cuda")
    p = lambda t: t.data_ptr()
    lse = torch.zeros(64, device="cuda")
    for L, D in ((9, 64), (0, 64), (4, 96), (4, 448)):
        assert L_.enh_short_causal_attention_backward(p(z), p(z), p(z), p(lse), 1, L, 1, D, 0.125, p(z), 1, None) == E_SHAPE, (L, D)


# ---- LayerNorm backward through a strided dy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True], ids=["set", "accumulate"])
@pytest.mark.parametrize("shape", [(1, 8, 8), (21, 192, 3 * 192), (131, 1536, 4 * 1536), (9, 8192, 2 * 8192)], ids=lambda s: "x".join(map(str, s)))
def test_ln_rows_strided_backward(C, shape, accumulate):
    M, D, stride = shape
    g = torch.Generator().manual_seed(D + 10 * M)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    w = 1 + 0.1 * torch.randn(D, generator=g)
    dy = torch.randn(M, D, generator=g)
    old = [torch.randn(D, generator=g) for _ in range(2)]
    wide = torch.full((M, stride), NAN)      # the other slots of the strided dy hold NaN: a read of them poisons the row
    wide[:, :D] = dy
    wide_d = wide.reshape(-1)[:(M - 1) * stride + D].clone()      # ends with the last row: nothing behind it belongs to the call
    wide_d, _ = _guarded(wide_d.view(1, -1), NAN)
    xd, wd = x.cuda(), w.cuda()

    def outs():
        dx, dx_w = _guarded(torch.full((M, D), NAN), SENTINEL)
        dx16, dx16_w = _guarded(torch.full((M, D), NAN, dtype=F16), SENTINEL)
        dw, db = (o.clone().cuda() if accumulate else torch.full((D,), NAN, device="cuda") for o in old)
        return dx, dx16, dw, db, dx_w, dx16_w

    dx, dx16, dw, db, dx_w, dx16_w = outs()
    C.ln_rows_strided_backward(wide_d, stride, xd, wd, dx, dw, db, dx16=dx16, accumulate=accumulate)
    torch.cuda.synchronize()
    assert bool((dx_w[dx.numel():] == SENTINEL).all()) and bool((dx16_w[dx16.numel():] == SENTINEL).all()), "wrote past dx / dx16"
    rx, rx16, rw, rb, _, _ = outs()
    C.ln_timeshift_backward(dy.cuda(), xd, wd, 1, rx, rw, rb, dx16=rx16, accumulate=accumulate)
    what = f"ln_rows_strided_backward M={M} D={D} stride={stride} accumulate={accumulate}"
    for name, a, b in (("dx", dx, rx), ("dw", dw, rw), ("db", db, rb)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: {name} is not the bits of ln_timeshift_backward on the compacted dy"
    assert torch.equal(dx16.view(torch.int16), rx16.view(torch.int16)) and torch.equal(dx16, dx.to(F16)), what + ": dx16"
    # against fp64, at the limits of test_gpt_backward_kernels_gpu.test_ln_timeshift_backward (plain mode)
    xq, wq, dyq = x.double().requires_grad_(True), w.double().requires_grad_(True), dy.double()
    bq = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xq, (D,), wq, bq, 1e-5).backward(dyq)
    xdd = x.double()
    rstd = 1 / torch.sqrt(xdd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    xh = (xdd - xdd.mean(-1, keepdim=True)) * rstd
    gw = dyq.abs() * w.double().abs()
    mag_dx = (gw + gw.mean(-1, keepdim=True) + xh.abs() * (gw * xh.abs()).mean(-1, keepdim=True)) * rstd
    o = [t.double() if accumulate else torch.zeros(D, dtype=torch.float64) for t in old]
    assert_elementwise(dx, xq.grad, elem_bound(xq.grad, mag_dx, 3 * D), what + " dx")
    assert_elementwise(dw, wq.grad + o[0], elem_bound(wq.grad, (dyq.abs() * xh.abs()).sum(0) + o[0].abs(), D + M), what + " dw")
    assert_elementwise(db, bq.grad + o[1], elem_bound(bq.grad, dyq.abs().sum(0) + o[1].abs(), M), what + " db")


# ---- embedding backward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True], ids=["set", "accumulate"])
@pytest.mark.parametrize("shape", [(2, 3, 2, 8, 5), (3, 1, 4, 128, 7), (1, 70, 8, 1028, 16)], ids=lambda s: "x".join(map(str, s)))
def test_rq_embed_seq_backward(C, shape, accumulate):
    """(2, 3, 2, 8, 5): many duplicates; (3, 1, 4, 128, 7): T = 1, no spatial code rows, and the deepest code is never fed; (1, 70, 8, 1028, 16):
    560 ids (three scan rounds), a thread owns two float4 columns"""
    B, T, D, Cw, V = shape
    Vc = 4
    gen = torch.Generator().manual_seed(B * 100 + T)
    gs, gd = torch.randn(B, T, Cw, generator=gen), torch.randn(B * T, D, Cw, generator=gen)
    conds = torch.randint(0, Vc - 1, (B,), generator=gen)             # condition Vc - 1 does not occur
    codes = torch.randint(0, V - 2, (B, T, D), generator=gen)         # codes V - 2 and V - 1 are not fed ...
    codes[:, T - 1, D - 1] = V - 1                                    # ... although V - 1 is the deepest code of every last position: never fed
    shapes = ((Vc, Cw), (Cw,), (V, Cw), (T + 1, Cw), (D - 1, Cw))     # tok_cond, pos_cond, tok_code, pos_code (rows T - 1 and T get nothing), pos_depth
    old = [torch.randn(s, generator=gen) for s in shapes]
    gd_dev = gd.clone()
    gd_dev[:, 0] = NAN                                                # slot 0 belongs to ln_spatial: never read here
    gsd, _ = _guarded(gs, NAN)
    gdd, _ = _guarded(gd_dev, NAN)
    runs = []
    for _ in range(2):
        pairs = [_guarded(o.clone() if accumulate else torch.full(o.shape, NAN), SENTINEL) for o in old]
        out = [p[0] for p in pairs]
        C.rq_embed_seq_backward(gsd, gdd, conds.cuda(), codes.cuda(), *out, accumulate=accumulate)
        torch.cuda.synchronize()
        assert all(bool((w[o.numel():] == SENTINEL).all()) for o, w in pairs), "wrote past a table"
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two launches differ"
    # fp64: what every fed occurrence (b, t, j) of a code sends to its row, then index_add_
    gs64, gd64 = gs.double(), gd.double().view(B, T, D, Cw)
    fed = torch.ones(B, T, D, dtype=torch.bool)
    fed[:, T - 1, D - 1] = False

    def tables(gs_, gd_):
        u = gd_.flip(2).cumsum(2).flip(2) - gd_                                        # sum_{d > j} gd[(b, t), d]
        u[:, :T - 1] += gs_[:, 1:].unsqueeze(2)
        u = u * fed.unsqueeze(-1)
        ref = [torch.zeros(s, dtype=torch.float64) for s in shapes]
        ref[0].index_add_(0, conds, gs_[:, 0])
        ref[1] += gs_[:, 0].sum(0)
        ref[2].index_add_(0, codes.reshape(-1), u.reshape(-1, Cw))
        ref[3][:T - 1] += gs_[:, 1:].sum(0)
        ref[4] += gd_[:, :, 1:].sum((0, 1))
        return ref

    ref, mag = tables(gs64, gd64), tables(gs64.abs(), gd64.abs())
    o64 = [o.double() if accumulate else torch.zeros_like(o, dtype=torch.float64) for o in old]
    for name, got, r_, m_, o_ in zip(("tok_cond", "pos_cond", "tok_code", "pos_code", "pos_depth"), runs[0], ref, mag, o64):
        assert_elementwise(got, r_ + o_, elem_bound(r_ + o_, m_ + o_.abs(), B * T * D + 1), f"rq_embed_seq_backward {shape} {name}")
    unfed = [(0, [Vc - 1]), (2, [V - 2, V - 1]), (3, [T - 1, T])]
    for i, rows in unfed:
        if accumulate:
            assert torch.equal(runs[0][i][rows].cpu().view(torch.int32), old[i][rows].view(torch.int32)), f"table {i}: an unmatched row was touched"
        else:
            assert bool((runs[0][i][rows] == 0).all()), f"table {i}: an unmatched row is not exactly zero"
