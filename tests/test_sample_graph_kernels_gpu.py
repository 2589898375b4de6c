"""The cursor forms of the sampling loop's launches (csrc/gpt_decode.hip) against their by-value siblings at
the same position: enh_decode_attention_at, enh_embed_step_at and enh_sample_logits_at read the position from a device int32 and must give the
bits of enh_decode_attention, enh_gpt_embed / enh_rq_embed_step and enh_sample_logits.  Every comparison is torch.equal on integer views of the
WHOLE allocation, guard regions included, so a write outside the result shows; a position outside an entry's range must write nothing at all."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 256           # sentinel elements in front of and behind every output
SENTINEL = 777.0      # exact in bf16, fp16 and f32
INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _guarded(shape, dt, content=None):
    """(whole allocation, the view of `shape` in its middle): sentinels around `content` (default: sentinels everywhere)"""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dt, device="cuda")
    view = whole[GUARD:GUARD + n].view(shape)
    if content is not None:
        view.copy_(content)
    return whole, view


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(INT_OF.get(a.dtype, a.dtype)), b.view(INT_OF.get(b.dtype, b.dtype)))


def _guards_intact(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def _cursor(t):
    return torch.tensor([t], dtype=torch.int32, device="cuda")


# ---- decode attention ---------------------------------------------------------------------------------------------------------------------
def _attention_pair(B, H, hs, Tmax, dt, positions, t_offset=0):
    from enhancing import _C
    torch.manual_seed(B * 1000 + hs + Tmax)
    C = H * hs
    k0 = torch.randn(B, H, Tmax, hs, device="cuda").to(dt)
    v0 = torch.randn(B, H, Tmax, hs, device="cuda").to(dt)
    for t in positions:
        qkv = torch.randn(B, 3 * C, device="cuda").to(dt)
        res = []
        for form in ("value", "cursor"):
            kw, k = _guarded((B, H, Tmax, hs), dt, k0)
            vw, v = _guarded((B, H, Tmax, hs), dt, v0)
            ow, o = _guarded((B, C), dt)
            if form == "value":
                _C.decode_attention(qkv, k, v, t, o)
            else:
                _C.decode_attention_at(qkv, k, v, _cursor(t - t_offset), o, t_offset=t_offset)
            res.append((ow, kw, vw))
        for name, a, b in zip(("out", "k_cache", "v_cache"), *res):
            assert _same_bits(a, b), (name, (B, H, hs, Tmax), dt, t)
            assert _guards_intact(b), (name, t)
        assert not bool((res[1][0][GUARD:-GUARD] == SENTINEL).any()), "out was not written"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", [(2, 2, 64, 200), (1, 1, 384, 200)])
def test_attention_at_few_heads_every_64_slot_boundary(shape, dt):
    """B H < 8: the plan cuts 64-slot pieces, nsplit changes at every boundary"""
    _attention_pair(*shape, dt, (0, 1, 63, 64, 65, 127, 128, 199))


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_at_many_heads_256_slot_pieces(dt):
    """B H >= 512: pieces of 256 slots, nsplit goes 1 -> 2 at t = 256"""
    _attention_pair(64, 16, 64, 300, dt, (255, 256, 299))


@pytest.mark.parametrize("t_offset", [3, -2])
def test_attention_at_with_an_offset(t_offset):
    _attention_pair(2, 2, 64, 200, torch.float16, (64, 130), t_offset=t_offset)


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_at_outside_the_cache_touches_nothing(dt):
    """the cursor at -1 and at Tmax (a replay too many): out, both caches and the workspace keep their sentinels"""
    from enhancing import _C
    B, H, hs, Tmax = 2, 2, 64, 200
    qkv = torch.randn(B, 3 * H * hs, device="cuda").to(dt)
    ws = _C._workspace(_C.lib().enh_decode_attention_workspace_bytes(B, H, hs, Tmax), qkv.device)
    for t, off in ((-1, 0), (Tmax, 0), (Tmax - 1, 1), (0, -1), (2 ** 31 - 1, 5)):
        kw, k = _guarded((B, H, Tmax, hs), dt)
        vw, v = _guarded((B, H, Tmax, hs), dt)
        ow, o = _guarded((B, H * hs), dt)
        ws.fill_(0x5A)
        _C.decode_attention_at(qkv, k, v, _cursor(t), o, t_offset=off)
        torch.cuda.synchronize()
        for w in (kw, vw, ow):
            assert bool((w == SENTINEL).all()), (t, off)
        assert bool((ws == 0x5A).all()), (t, off)


# ---- the step's input row -----------------------------------------------------------------------------------------------------------------
V_EMB = 50


def _tables(C, T, D):
    torch.manual_seed(C + T + D)
    table = torch.randn(V_EMB, C, device="cuda")
    pos_code = torch.randn(T, C, device="cuda")
    pos_depth = torch.randn(max(D - 1, 1), C, device="cuda")
    return table, pos_code, pos_depth


def _ids(*shape):
    ids = torch.randint(0, V_EMB, shape, device="cuda")
    ids.view(-1)[::7] = -3           # clamped to 0
    ids.view(-1)[3::11] = V_EMB + 9  # clamped to V - 1
    return ids


@pytest.mark.parametrize("C", [128, 4104])
def test_embed_at_is_gpt_embed(C):
    """GPT: ids feed[:, t - 1], n = 1, position row pos_emb_code[t - 1] (negative offsets), at the first and the last position"""
    from enhancing import _C
    B, T = 3, 9
    table, pos_code, _ = _tables(C, T, 1)
    feed = _ids(B, T)
    for t in (1, T - 1):
        aw, a = _guarded((B, C), torch.float32)
        bw, b = _guarded((B, C), torch.float32)
        _C.gpt_embed(table, feed[:, t - 1], pos_code[t - 1], a)
        _C.embed_step_at(table, feed, 1, 1, -1, pos_code, C, -C, _cursor(t), 1, T, b)
        assert _same_bits(aw, bw) and _guards_intact(bw), (C, t)
        assert bool((b == table[feed[:, t - 1].clamp(0, V_EMB - 1)] + pos_code[t - 1]).all())


@pytest.mark.parametrize("C", [128, 4104])
@pytest.mark.parametrize("D", [4, 8])
def test_embed_at_is_rq_embed_step(C, D):
    """RQ: the spatial row (ids feed[:, t - 1, :], n = D, pos_emb_code[t - 1]) and the depth slots (ids feed[:, t, :d], n = d, the fixed row
    pos_emb_depth[d - 1]), on a chunk of the rows of a larger tensor"""
    from enhancing import _C
    B, T = 3, 6
    table, pos_code, pos_depth = _tables(C, T, D)
    feed = _ids(B + 2, T, D)[1:B + 1]
    for t in (1, T - 1):
        aw, a = _guarded((B, C), torch.float32)
        bw, b = _guarded((B, C), torch.float32)
        _C.rq_embed_step(table, feed[:, t - 1, :], pos_code[t - 1], a)
        _C.embed_step_at(table, feed, D, D, -D, pos_code, C, -C, _cursor(t), 1, T, b)
        assert _same_bits(aw, bw) and _guards_intact(bw), ("spatial", C, D, t)
    for t in (0, 1, T - 1):
        for d in sorted({1, min(4, D - 1), D - 1}):
            aw, a = _guarded((B, C), torch.float32)
            bw, b = _guarded((B, C), torch.float32)
            _C.rq_embed_step(table, feed[:, t, :d], pos_depth[d - 1], a)
            _C.embed_step_at(table, feed, d, D, 0, pos_depth[d - 1], 0, 0, _cursor(t), 0, T, b)
            assert _same_bits(aw, bw) and _guards_intact(bw), ("depth", C, D, t, d)


def test_embed_at_outside_its_positions_touches_nothing_and_bad_ranges_are_refused():
    from enhancing import _C
    B, T, C = 2, 5, 128
    table, pos_code, _ = _tables(C, T, 1)
    feed = _ids(B, T)
    for t in (0, T, -1, 2 ** 31 - 1):
        ow, o = _guarded((B, C), torch.float32)
        _C.embed_step_at(table, feed, 1, 1, -1, pos_code, C, -C, _cursor(t), 1, T, o)
        torch.cuda.synchronize()
        assert bool((ow == SENTINEL).all()), t
    ow, o = _guarded((B, C), torch.float32)
    with pytest.raises(RuntimeError, match="reads ids outside"):
        _C.embed_step_at(table, feed, 1, 1, -1, pos_code, C, -C, _cursor(1), 0, T, o)
    with pytest.raises(RuntimeError, match="reads ids outside"):
        _C.embed_step_at(table, feed, 1, 1, 0, pos_code, C, 0, _cursor(1), 0, T + 1, o)
    with pytest.raises(RuntimeError, match="position values"):
        _C.embed_step_at(table, feed, 1, 1, -1, pos_code, C, 0, _cursor(1), 1, T + 1, o)


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k,top_p", [(None, None), (50, None), (None, 0.9), (50, 0.9)])
@pytest.mark.parametrize("V", [512, 16384])
def test_sample_at_is_sample_logits(V, top_k, top_p):
    """step = cursor * 4 + {0, 3}: the code and the logits row land in the slice of that step and nowhere else"""
    from enhancing import _C
    B, T, D = 3, 5, 4
    torch.manual_seed(V)
    logits = 3.0 * torch.randn(B, V, device="cuda")
    kw = dict(temperature=0.8, top_k=top_k, top_p=top_p, seed=11, call=2, row0=5)
    for t in (0, 2, T - 1):
        for d in (0, 3):
            pair = []
            for form in ("value", "cursor"):
                codes = torch.full((B + 2, T, D), -1, dtype=torch.int64, device="cuda")
                lw, lo = _guarded((B + 2, T, D, V), torch.float32)
                if form == "value":
                    _C.sample_logits(logits, codes[1:B + 1, t, d], step=t * D + d, logits_out=lo[1:B + 1, t, d, :], **kw)
                else:
                    _C.sample_logits_at(logits, codes[1:B + 1], _cursor(t), step_mul=D, step_add=d, logits_out=lo[1:B + 1], **kw)
                pair.append((codes, lw))
            (c1, l1), (c2, l2) = pair
            assert torch.equal(c1, c2) and _same_bits(l1, l2) and _guards_intact(l2), (V, top_k, top_p, t, d)
            assert int((c2 >= 0).sum()) == B and bool((c2[1:B + 1, t, d] >= 0).all())
            # without logits_out: the same codes
            c3 = torch.full((B + 2, T, D), -1, dtype=torch.int64, device="cuda")
            _C.sample_logits_at(logits, c3[1:B + 1], _cursor(t), step_mul=D, step_add=d, **kw)
            assert torch.equal(c3, c2)


def test_sample_at_outside_its_steps_touches_nothing():
    from enhancing import _C
    B, T, D, V = 2, 3, 4, 512
    logits = torch.randn(B, V, device="cuda")
    for t in (T, -1, 2 ** 31 - 1):
        codes = torch.full((B, T, D), -1, dtype=torch.int64, device="cuda")
        lw, lo = _guarded((B, T, D, V), torch.float32)
        _C.sample_logits_at(logits, codes, _cursor(t), step_mul=D, step_add=3, seed=1, logits_out=lo)
        torch.cuda.synchronize()
        assert bool((codes == -1).all()) and bool((lw == SENTINEL).all()), t


# ---- the cursor ---------------------------------------------------------------------------------------------------------------------------
def test_three_advances_add_three():
    from enhancing import _C
    whole = torch.full((9,), 40, dtype=torch.int32, device="cuda")
    cur = whole[4:5]
    for _ in range(3):
        _C.cursor_advance(cur)
    assert whole.tolist() == [40, 40, 40, 40, 43, 40, 40, 40, 40]
    with pytest.raises(RuntimeError, match="cursor must be"):
        _C.cursor_advance(torch.zeros(1, dtype=torch.int64, device="cuda"))
