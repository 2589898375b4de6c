"""The kernels of the stage-2 RQTransformer's forward (csrc/rq_prefill.hip), each against fp64 on the values it is given.

Short-sequence causal attention, shapes (NSEQ, L, H) for every head width and both formats, and what each one catches:
    (1, 1, 1)     a single token: one live group of eight lanes in the workgroup
    (7, 2, 2)     14 (sequence, head) pairs: a partly filled workgroup
    (33, 3, 1)    an odd L; 33 pairs: a second workgroup with one live group
    (130, 4, 2)   the shipped depth; 260 pairs: nine workgroups, the last one ragged
    (5, 5, 3)     H = 3: a sequence's heads straddle a wave
    (19, 8, 2)    the longest sequence
Limits: tests/attn_causal_util.py with B = NSEQ and N = L (attn_dh_util's element bound and row metric x ATT_MARGIN = 2), the lse tolerance of
tests/test_gpt_prefill_kernels_gpu.py."""
import pytest
import torch

from attn_causal_util import check_causal_out
from util import h16r

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
WIDTHS = [64, 128, 192, 256, 320, 384]
SHAPES = [(1, 1, 1), (7, 2, 2), (33, 3, 1), (130, 4, 2), (5, 5, 3), (19, 8, 2)]
GUARD_ROWS = 64
SENTINEL = 12345.0
E_SHAPE = -2      # include/enh_hip.h ENH_E_SHAPE


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _qkv(D, NSEQ, L, H, dt):
    g = torch.Generator().manual_seed(D * 1000 + NSEQ * 100 + L + H)
    return h16r(torch.randn(NSEQ, L, 3 * H * D, generator=g) * 1.5, dt)


def _run(C, qkv, NSEQ, L, H, D, dt, with_lse=True):
    out = torch.full((NSEQ, L, H * D), float("nan"), dtype=dt, device="cuda")
    lse = torch.full((NSEQ, H, L), float("nan"), device="cuda") if with_lse else None
    C.short_causal_attention(qkv.to(dt).cuda(), NSEQ, L, H, D, out, lse)
    torch.cuda.synchronize()
    return out, lse


def _bits(t):
    return t.view(torch.int16)


# ---- short-sequence causal attention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", WIDTHS)
def test_short_attention_against_fp64(C, D, shape, dt):
    NSEQ, L, H = shape
    qkv = _qkv(D, NSEQ, L, H, dt)
    out, lse = _run(C, qkv, NSEQ, L, H, D, dt)
    what = f"short causal attention D={D} NSEQ={NSEQ} L={L} H={H} {dt}"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()), what + ": an element was never written"
    w, k, ref = check_causal_out(out, qkv, NSEQ, L, H, D, D ** -0.5, dt, what)
    e_lse = (lse.double().cpu() - ref[1]).abs().max().item()
    print(f"{what}: worst element / bound {w:.3f}, worst row / model {k:.3f}, lse abs err {e_lse:.2e}")
    assert e_lse <= 1e-4 + 1e-5 * ref[1].abs().max().item()


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_one_token_is_v_bit_for_bit(C, dt):
    NSEQ, H, D = 37, 3, 192
    qkv = _qkv(D, NSEQ, 1, H, dt)
    out, lse = _run(C, qkv, NSEQ, 1, H, D, dt)
    assert torch.equal(_bits(out), _bits(qkv[..., 2 * H * D:].to(dt).cuda()))


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_sequences_of_a_pack_do_not_see_each_other(C, dt):
    """41 sequences of 3 heads: 123 pairs in four workgroups.  Sequence 13 gets other q, k and v: every other sequence keeps its bits."""
    NSEQ, L, H, D = 41, 4, 3, 128
    base = _qkv(D, NSEQ, L, H, dt)
    other = base.clone()
    other[13] = h16r(base[13] * -1.75 + 0.5, dt)
    (ob, lb), (oo, lo) = _run(C, base, NSEQ, L, H, D, dt), _run(C, other, NSEQ, L, H, D, dt)
    keep = [i for i in range(NSEQ) if i != 13]
    assert torch.equal(_bits(ob[keep]), _bits(oo[keep])) and torch.equal(lb[keep].view(torch.int32), lo[keep].view(torch.int32))
    assert not torch.equal(ob[13], oo[13])
    check_causal_out(oo, other, NSEQ, L, H, D, D ** -0.5, dt, f"changed sequence {dt}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
def test_later_keys_do_not_move_earlier_rows(C, dt):
    """key and value 5 of sequence 2, head 1, get a key that carries every later row: rows 0 .. 4 keep their bits, so does head 0"""
    NSEQ, L, H, D = 4, 8, 2, 64
    base = _qkv(D, NSEQ, L, H, dt)
    spiked = base.clone()
    spiked[2, 5, H * D + D:H * D + 2 * D] = h16r(base[2, 6, D:2 * D] * (50.0 / (2.25 * D ** 0.5)), dt)      # k of head 1
    spiked[2, 5, 2 * H * D + D:] = 3.0                                                                     # v of head 1
    (ob, _), (os_, _) = _run(C, base, NSEQ, L, H, D, dt), _run(C, spiked, NSEQ, L, H, D, dt)
    assert torch.equal(_bits(ob[2, :5]), _bits(os_[2, :5])), "a key above the diagonal moved a row in front of it"
    assert torch.equal(_bits(ob[..., :D]), _bits(os_[..., :D])), "head 0 moved"
    assert not torch.equal(ob[2, 5:, D:], os_[2, 5:, D:])      # (the rows from the key on do see it)
    check_causal_out(os_, spiked, NSEQ, L, H, D, D ** -0.5, dt, f"spiked short attention {dt}")


def _guarded(t, fill):
    """`t` at the FRONT of a larger allocation whose remainder, GUARD_ROWS rows of t's last axis, holds `fill`: (view of the front, the whole)"""
    whole = torch.empty(t.numel() + GUARD_ROWS * t.shape[-1], dtype=t.dtype, device="cuda")
    whole[:t.numel()] = t.reshape(-1).cuda()
    whole[t.numel():] = fill
    return whole[:t.numel()].view(t.shape), whole


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D,shape", [(384, (33, 3, 1)), (64, (5, 5, 3)), (320, (19, 8, 2))])
def test_short_attention_writes_nothing_outside_its_tensors(C, D, shape, dt):
    """NaN behind qkv (an over-read that reaches arithmetic poisons the result), a finite sentinel behind out and lse (an over-write changes it)"""
    NSEQ, L, H = shape
    qkv = _qkv(D, NSEQ, L, H, dt)
    nan = float("nan")
    qd, _ = _guarded(qkv.to(dt), nan)
    out, out_w = _guarded(torch.full((NSEQ, L, H * D), nan, dtype=dt), SENTINEL)
    lse, lse_w = _guarded(torch.full((NSEQ, H, L), nan), SENTINEL)
    C.short_causal_attention(qd, NSEQ, L, H, D, out, lse)
    torch.cuda.synchronize()
    assert bool((out_w[out.numel():] == SENTINEL).all()) and bool((lse_w[lse.numel():] == SENTINEL).all()), "wrote past out / lse"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    check_causal_out(out, qkv, NSEQ, L, H, D, D ** -0.5, dt, f"guarded short attention D={D} {shape} {dt}")


def test_short_attention_same_bits_over_two_launches_and_without_lse(C):
    for D, (NSEQ, L, H), dt in ((384, (19, 8, 2), F16), (128, (130, 4, 2), BF16)):
        qkv = _qkv(D, NSEQ, L, H, dt)
        (o1, l1), (o2, l2) = _run(C, qkv, NSEQ, L, H, D, dt), _run(C, qkv, NSEQ, L, H, D, dt)
        assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
        o3, _ = _run(C, qkv, NSEQ, L, H, D, dt, with_lse=False)
        assert torch.equal(_bits(o1), _bits(o3))


def test_unsupported_shapes_are_shape_errors(C):
    for L, D in ((9, 64), (0, 64), (4, 96)):
        qkv = torch.zeros(2, max(L, 1), 3 * D, dtype=F16, device="cuda")
        out = torch.zeros(2, max(L, 1), D, dtype=F16, device="cuda")
        rc = C.lib().enh_short_causal_attention_forward(qkv.data_ptr(), 2, L, 1, D, 1.0, out.data_ptr(), None, C.DT_F16, None)
        assert rc == E_SHAPE, (L, D, rc)
    with pytest.raises(RuntimeError):
        C.short_causal_attention(torch.zeros(2, 9, 3 * 64, dtype=F16, device="cuda"), 2, 9, 1, 64, torch.zeros(2, 9, 64, dtype=F16, device="cuda"))


def test_launches_are_labelled_with_their_kernel(C):
    last = lambda: C.lib().enh_last_kernel().decode()
    _run(C, _qkv(192, 5, 3, 2, BF16), 5, 3, 2, 192, BF16)
    assert last() == "rq_short_causal_kernel<3, BF16>"
    _run(C, _qkv(64, 2, 8, 1, F16), 2, 8, 1, 64, F16)
    assert last() == "rq_short_causal_kernel<8, F16>"
    x, w = torch.randn(4, 64, device="cuda"), torch.ones(64, device="cuda")
    C.ln_rows_strided(x, w, w, torch.empty(4, 2, 64, device="cuda"), 128)
    assert last() == "rq_ln_strided_kernel"
    ids = torch.zeros(1, 1, 2, dtype=torch.int64, device="cuda")
    t = torch.randn(3, 64, device="cuda")
    C.rq_embed_seq(ids[0, 0, :1], ids, t, t[0], t, t, t[:1], torch.empty(1, 1, 64, device="cuda"), torch.empty(1, 2, 64, device="cuda"))
    assert last() == "rq_embed_seq_kernel"


# ---- the embedding stage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cw", [128, 8192])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 7)], ids=["1x1", "3x7"])
@pytest.mark.parametrize("D", [2, 8])
def test_rq_embed_seq(C, D, B, T, Cw):
    Vc, V = 5, 19
    g = torch.Generator().manual_seed(D * 10 + T)
    tc, pc = torch.randn(Vc, Cw, generator=g).cuda(), torch.randn(Cw, generator=g).cuda()
    tk, pk, pd = torch.randn(V, Cw, generator=g).cuda(), torch.randn(T, Cw, generator=g).cuda(), torch.randn(D - 1, Cw, generator=g).cuda()
    conds = torch.randint(0, Vc, (B,), generator=g).cuda()
    codes = torch.randint(0, V - 1, (B, T, D), generator=g)      # id V - 1 does not occur ...
    codes[codes == 7] = 8                                        # ... nor does id 7
    codes[0, 0, 0], codes[-1, -1, -1] = 0, V - 2
    codes = codes.cuda()
    spatial = torch.full((B, T, Cw), float("nan"), device="cuda")
    depth = torch.full((B * T, D, Cw), SENTINEL, device="cuda")
    C.rq_embed_seq(conds, codes, tc, pc, tk, pk, pd, spatial, depth)
    torch.cuda.synchronize()
    assert bool((depth[:, 0] == SENTINEL).all()), "slot 0 of the depth stream belongs to the strided LayerNorm"
    emb = tk[codes]                                                                    # [B, T, D, Cw]
    # the same f32 sums in ascending depth, one rounding per addition: the same bits
    run, slots = emb[:, :, 0], []
    for d in range(1, D):
        slots.append(run + pd[d - 1])
        run = run + emb[:, :, d]
    want_sp = torch.cat([(tc[conds] + pc)[:, None], run[:, :T - 1] + pk[:T - 1]], 1)
    assert torch.equal(spatial, want_sp)
    assert torch.equal(depth[:, 1:], torch.stack(slots, 2).view(B * T, D - 1, Cw))
    # and against an fp64 gather-and-cumsum: D roundings of at most 2^-24 of the sum of the magnitudes
    cs = emb.double().cumsum(2)
    mag = emb.double().abs().cumsum(2)
    ref_d = (cs[:, :, :D - 1] + pd.double()).view(B * T, D - 1, Cw)
    lim_d = (D * 2.0 ** -24 * (mag[:, :, :D - 1] + pd.double().abs())).view(B * T, D - 1, Cw)
    assert bool(((depth[:, 1:].double() - ref_d).abs() <= lim_d).all())
    ref_s = cs[:, :T - 1, D - 1] + pk[:T - 1].double()
    assert bool(((spatial[:, 1:].double() - ref_s).abs() <= (D + 1) * 2.0 ** -24 * (mag[:, :T - 1, D - 1] + pk[:T - 1].double().abs())).all())


# ---- LayerNorm with an output row stride -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 21])
@pytest.mark.parametrize("Cw", [128, 1536, 8192])
def test_ln_rows_strided(C, Cw, M):
    slots = 3
    g = torch.Generator().manual_seed(Cw + M)
    x = (torch.randn(M, Cw, generator=g) * 2 + 0.3).cuda()
    w, b = (1 + 0.1 * torch.randn(Cw, generator=g)).cuda(), (0.1 * torch.randn(Cw, generator=g)).cuda()
    out = torch.full((M, slots, Cw), SENTINEL, device="cuda")
    C.ln_rows_strided(x, w, b, out, slots * Cw)
    torch.cuda.synchronize()
    assert bool((out[:, 1:] == SENTINEL).all()), "the other slots were written"
    ref = torch.nn.functional.layer_norm(x.double(), (Cw,), w.double(), b.double(), 1e-5)
    err = (out[:, 0].double() - ref).abs()
    assert bool((err <= 1e-5 * ref.abs() + 1e-6).all()), err.max().item()
    out2 = torch.full((M, slots, Cw), SENTINEL, device="cuda")
    C.ln_rows_strided(x, w, b, out2, slots * Cw)
    assert torch.equal(out, out2)
    with pytest.raises(RuntimeError):
        C.ln_rows_strided(x, w, b, out, Cw - 4)      # rows that would overlap
