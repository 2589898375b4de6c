"""The sequence-shaped kernels of the stage-2 forward (csrc/gpt_prefill.hip), each against fp64 on the values it is given.

Causal attention, shapes (B, N, H) for every head width and both formats, and what each one catches:
    (2, 64, 2)    one aligned tile: the diagonal mask alone; second batch element / head offsets
    (1, 1, 1)     a single token; (2, 2, 2) two
    (2, 63, 2)    one ragged tile, idle waves, leakage from the next batch element
    (1, 65, 3)    H = 3; a second tile holding ONE key, seen by one query
    (1, 129, 2)   a second query block with one live query, three tiles, waves that skip tiles above their diagonal
    (2, 200, 2)   both ring stages, a ragged last tile on the diagonal
    (1, 257, 2)   three query blocks (the reversed dispatch order), five tiles
Limits: tests/attn_causal_util.py (attn_dh_util's element bound and row metric x ATT_MARGIN = 2, causal reference and rounding model)."""
import pytest
import torch

from attn_causal_util import causal_ref64, check_causal_out
from util import U16, h16r, rel

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
WIDTHS = [64, 128, 192, 256, 320, 384]
SHAPES = [(2, 64, 2), (1, 1, 1), (2, 2, 2), (2, 63, 2), (1, 65, 3), (1, 129, 2), (2, 200, 2), (1, 257, 2)]
GUARD_ROWS = 64
SENTINEL = 12345.0
E_SHAPE = -2      # include/enh_hip.h ENH_E_SHAPE


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _qkv(D, B, N, H, dt):
    g = torch.Generator().manual_seed(D * 1000 + B * 100 + N + H)
    return h16r(torch.randn(B, N, 3 * H * D, generator=g) * 1.5, dt)


def _run(C, qkv, B, N, H, D, dt):
    out = torch.full((B, N, H * D), float("nan"), dtype=dt, device="cuda")
    lse = torch.full((B, H, N), float("nan"), device="cuda")
    C.causal_attention(qkv.to(dt).cuda(), B, N, H, D, out, lse)
    torch.cuda.synchronize()
    return out, lse


# ---- causal attention ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", WIDTHS)
def test_causal_attention_against_fp64(C, D, shape, dt):
    B, N, H = shape
    qkv = _qkv(D, B, N, H, dt)
    out, lse = _run(C, qkv, B, N, H, D, dt)
    what = f"causal attention D={D} B={B} N={N} H={H} {dt}"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()), what + ": an element was never written"
    w, k, ref = check_causal_out(out, qkv, B, N, H, D, D ** -0.5, dt, what)
    e_lse = (lse.double().cpu() - ref[1]).abs().max().item()
    print(f"{what}: worst element / bound {w:.3f}, worst row / model {k:.3f}, lse abs err {e_lse:.2e}")
    assert e_lse <= 1e-4 + 1e-5 * ref[1].abs().max().item()


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 384])
def test_future_keys_do_not_move_the_output(C, D, dt):
    """query 70 of head 0 gets a key 30+ above every other score at key 100 (its own diagonal tile, key > query) and at key 150 (a tile above its
    diagonal): every row that may not see those keys has the bits it has without them, and stays within the limits"""
    B, N, H = 1, 200, 2
    base = _qkv(D, B, N, H, dt)
    spiked = base.clone()
    gain = 50.0 / (2.25 * D ** 0.5)       # |q|^2 ~ 2.25 D, so the score is ~50; the others are ~N(0, 2.25^2)
    for key in (100, 150):
        spiked[0, key, H * D:H * D + D] = h16r(base[0, 70, :D] * gain, dt)
    s = (spiked[0, 70, :D].double() * spiked[0, :, H * D:H * D + D].double()).sum(-1) * D ** -0.5
    assert s[100] > s[:71].max() + 30 and s[150] > s[:71].max() + 30
    out_b, _ = _run(C, base, B, N, H, D, dt)
    out_s, _ = _run(C, spiked, B, N, H, D, dt)
    assert torch.equal(out_b[0, :100, :D].view(torch.int16), out_s[0, :100, :D].view(torch.int16)), "a masked key moved rows in front of it"
    assert torch.equal(out_b[..., D:].view(torch.int16), out_s[..., D:].view(torch.int16)), "head 1 moved"
    assert not torch.equal(out_b[0, 150:, :D], out_s[0, 150:, :D])      # (the rows behind the keys do see them)
    check_causal_out(out_s, spiked, B, N, H, D, D ** -0.5, dt, f"spiked causal attention D={D} {dt}")


def _guarded(t, fill):
    """`t` at the FRONT of a larger allocation whose remainder, GUARD_ROWS rows of t's last axis, holds `fill`: (view of the front, the whole)"""
    whole = torch.empty(t.numel() + GUARD_ROWS * t.shape[-1], dtype=t.dtype, device="cuda")
    whole[:t.numel()] = t.reshape(-1).cuda()
    whole[t.numel():] = fill
    return whole[:t.numel()].view(t.shape), whole


@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("D,shape", [(384, (2, 63, 2)), (192, (1, 129, 2)), (320, (1, 65, 3))])
def test_causal_attention_reads_and_writes_nothing_outside_its_tensors(C, D, shape, dt):
    """NaN rows behind qkv (the K / V rows >= N of the last batch element: an over-read that reaches arithmetic poisons the result), a finite
    sentinel behind out and lse (an over-write changes its bits).  Nothing here faults: every allocation covers a 64-row over-run."""
    B, N, H = shape
    qkv = _qkv(D, B, N, H, dt)
    nan = float("nan")
    qd, _ = _guarded(qkv.to(dt), nan)
    out, out_w = _guarded(torch.full((B, N, H * D), nan, dtype=dt), SENTINEL)
    lse, lse_w = _guarded(torch.full((B, H, N), nan), SENTINEL)
    C.causal_attention(qd, B, N, H, D, out, lse)
    torch.cuda.synchronize()
    assert bool((out_w[out.numel():] == SENTINEL).all()) and bool((lse_w[lse.numel():] == SENTINEL).all()), "wrote past out / lse"
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    check_causal_out(out, qkv, B, N, H, D, D ** -0.5, dt, f"guarded causal attention D={D} {shape} {dt}")


def test_causal_attention_same_bits_over_two_launches_and_without_lse(C):
    for D, (B, N, H), dt in ((384, (1, 257, 2), F16), (128, (2, 200, 2), BF16)):
        qkv = _qkv(D, B, N, H, dt)
        (o1, l1), (o2, l2) = _run(C, qkv, B, N, H, D, dt), _run(C, qkv, B, N, H, D, dt)
        assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
        o3 = torch.empty_like(o1)
        C.causal_attention(qkv.to(dt).cuda(), B, N, H, D, o3, None)
        assert torch.equal(o1.view(torch.int16), o3.view(torch.int16))


def test_unsupported_head_widths_are_shape_errors(C):
    for D in (80, 448, 32):
        qkv = torch.zeros(1, 4, 3 * D, dtype=F16, device="cuda")
        out = torch.zeros(1, 4, D, dtype=F16, device="cuda")
        rc = C.lib().enh_causal_attention_forward(qkv.data_ptr(), 1, 4, 1, D, 1.0, out.data_ptr(), None, C.DT_F16, None)
        assert rc == E_SHAPE, (D, rc)
        q32, o32 = qkv.float(), out.float()
        assert C.lib().enh_causal_attention_forward_f32(q32.data_ptr(), 1, 4, 1, D, 1.0, o32.data_ptr(), None, None) == E_SHAPE
        with pytest.raises(RuntimeError):
            C.causal_attention(qkv, 1, 4, 1, D, out)


@pytest.mark.parametrize("D,shape", [(64, (2, 63, 2)), (192, (1, 129, 2)), (384, (2, 70, 1))])
def test_exact_mode_causal_attention(C, D, shape):
    """the f32 instrument: sums of f32 products in ascending order against fp64: (2 k + 8) 2^-24 per sum of k terms (util.elem_bound's constant),
    k = D for a score and N for a row of P V, on P |V| and on |out|"""
    B, N, H = shape
    qkv = _qkv(D, B, N, H, F16).float()
    out = torch.full((B, N, H * D), float("nan"), device="cuda")
    lse = torch.full((B, H, N), float("nan"), device="cuda")
    C.causal_attention(qkv.cuda(), B, N, H, D, out, lse)
    ref, lse_ref, pav = causal_ref64(qkv, B, N, H, D, D ** -0.5)
    # a score error ds moves p by p ds: |ds| <= (2 D + 8) 2^-24 sum|q||k| scale, here <= (2 D + 8) 2^-24 x 2.25 D x D^-0.5 x ~3
    ds = (2 * D + 8) * 2.0 ** -24 * 2.25 * D ** 0.5 * 3
    bound = ((2 * N + 8) * 2.0 ** -24 + 2 * ds) * pav + 2.0 ** -23 * ref.abs()
    err = (out.double().cpu() - ref).abs()
    assert bool((err <= bound).all()), (err / bound).max().item()
    assert (lse.double().cpu() - lse_ref).abs().max().item() <= 1e-5 + ds


# ---- LayerNorm + time shift ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1, 128), (2, 5, 192), (1, 70, 768)], ids=lambda s: "x".join(map(str, s)))
def test_ln_timeshift(C, shape):
    B, S, D = shape
    g = torch.Generator().manual_seed(B * 100 + S)
    x = (torch.randn(B * S, D, generator=g) * 2 + 0.3).cuda()
    w, b = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    tm = (torch.arange(D) / (D - 1) + 0.05 * torch.randn(D, generator=g)).float().cuda()
    ln64 = torch.nn.functional.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5).view(B, S, D)
    prev = torch.cat([torch.zeros_like(ln64[:, :1]), ln64[:, :-1]], 1)
    ref_mix = (ln64 * tm.double() + prev * (1 - tm.double())).view(B * S, D)
    plain = torch.empty(B * S, D, device="cuda")
    C.ln_timeshift(x, w, b, plain, S)
    mix = torch.empty(B * S, D, device="cuda")
    C.ln_timeshift(x, w, b, mix, S, colscale=tm)
    for got, ref, what in ((plain, ln64.view(B * S, D), "plain"), (mix, ref_mix, "mix")):
        err = (got.double() - ref).abs()
        assert bool((err <= 1e-5 * ref.abs() + 1e-6).all()) and rel(got, ref) <= 1e-5, (what, err.max().item())
    # the shifted term of the first row of every batch element is ZERO: a shift that runs across batch elements adds ln(previous element's last row)
    assert torch.equal(mix.view(B, S, D)[:, 0], (plain * tm).view(B, S, D)[:, 0]), "the first row of a batch element is not ln * time_mix"
    for dt in (F16, BF16):
        o16, o32 = torch.empty(B * S, D, dtype=dt, device="cuda"), torch.empty(B * S, D, device="cuda")
        C.ln_timeshift(x, w, b, o16, S, colscale=tm, out_f32=o32)
        assert torch.equal(o32, mix) and torch.equal(o16, mix.to(dt))
        err = (o16.double() - ref_mix).abs()
        assert bool((err <= U16[dt] * ref_mix.abs() + 1e-6).all()), (dt, err.max().item())
    with pytest.raises(RuntimeError):
        C.ln_timeshift(x, w, b, plain, B * S + 1, colscale=tm)      # rows that are no whole sequences


# ---- embedding, relu^2, cross-entropy --------------------------------------------------------------------------------------------------------------
def test_embed_seq(C):
    B, T, Cw, Vc, V = 3, 7, 136, 5, 19
    g = torch.Generator().manual_seed(1)
    tc, pc = torch.randn(Vc, Cw, generator=g).cuda(), torch.randn(Cw, generator=g).cuda()
    tk, pk = torch.randn(V, Cw, generator=g).cuda(), torch.randn(T, Cw, generator=g).cuda()
    conds = torch.randint(0, Vc, (B,), generator=g).cuda()
    codes = torch.randint(0, V, (B, T), generator=g).cuda()
    codes[0, 0], codes[1, 1] = 0, V - 1
    for S in (T, 1):
        out = torch.full((B, S, Cw), float("nan"), device="cuda")
        C.gpt_embed_seq(conds, codes, tc, pc, tk, pk, out)
        ref = torch.cat([(tc[conds] + pc)[:, None], tk[codes[:, :S - 1]] + pk[:S - 1]], 1)
        assert torch.equal(out, ref)      # one f32 addition per element: the same bits


def test_relu_sq(C):
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(5, 1000, generator=g) * 3).cuda()
    ref = torch.square(torch.relu(x.double()))
    for dt in (F16, BF16):
        y = torch.empty(5, 1000, dtype=dt, device="cuda")
        C.relu_sq(y, x)
        assert bool(((y.double() - ref).abs() <= (U16[dt] + 2.0 ** -23) * ref + 2.0 ** -24).all())      # the f32 square, then one rounding
        z = x.to(dt)
        refz = torch.square(torch.relu(z.double()))
        C.relu_sq(z)      # in place on the 16-bit values
        assert bool(((z.double() - refz).abs() <= (U16[dt] + 2.0 ** -23) * refz + 2.0 ** -24).all())
    y32 = torch.empty_like(x)
    C.relu_sq(y32, x)
    assert torch.equal(y32, torch.square(torch.relu(x)))
    C.relu_sq(x)
    assert torch.equal(x, y32)


@pytest.mark.parametrize("V", [8, 1000, 16384])
def test_cross_entropy_rows(C, V):
    M = 37
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(M, V, generator=g) * 2
    target = torch.randint(0, V, (M,), generator=g)
    target[0], target[1] = 0, V - 1
    logits[2, V // 2] += 80.0       # one row with a logit 80 above the rest (its target is elsewhere: nll ~ 80)
    target[2] = 0 if V // 2 != 0 else 1
    ref = torch.nn.functional.cross_entropy(logits.double(), target, reduction="none")
    nll, mean = torch.empty(M, device="cuda"), torch.empty(1, device="cuda")
    C.cross_entropy_rows(logits.cuda(), target.cuda(), nll, mean)
    err = ((nll.double().cpu() - ref).abs() / ref.abs()).max().item()
    print(f"cross-entropy V={V}: worst relative error {err:.2e}")
    assert err <= 1e-6
    assert abs(mean.item() - ref.mean().item()) <= 1e-6 * ref.mean().item()
    nll2, mean2 = torch.empty(M, device="cuda"), torch.empty(1, device="cuda")
    C.cross_entropy_rows(logits.cuda(), target.cuda(), nll2, mean2)
    assert torch.equal(nll.view(torch.int32), nll2.view(torch.int32)) and torch.equal(mean.view(torch.int32), mean2.view(torch.int32))
    mean3 = torch.empty(1, device="cuda")
    C.mean_f32(nll, mean3)
    assert torch.equal(mean3.view(torch.int32), mean.view(torch.int32))


def test_launches_are_labelled_with_their_kernel(C):
    """the label path of the library (enh_last_kernel): the symbol of the kernel the call launched, as a profiler prints it"""
    last = lambda: C.lib().enh_last_kernel().decode()
    qkv = _qkv(192, 1, 65, 3, BF16)
    _run(C, qkv, 1, 65, 3, 192, BF16)
    assert last() == "gpt_prefill_causal_kernel<192, BF16>"
    x, w = torch.randn(4, 64, device="cuda"), torch.ones(64, device="cuda")
    C.ln_timeshift(x, w, w, torch.empty(4, 64, dtype=F16, device="cuda"), 2, colscale=w)
    assert last() == "gpt_prefill_ln_kernel<F16>"
    C.relu_sq(torch.empty(4, 64, dtype=F16, device="cuda"), x)
    assert last() == "gpt_prefill_relu_sq_kernel<F16, true, false>"
    C.cross_entropy_rows(x, torch.zeros(4, dtype=torch.int64, device="cuda"), torch.empty(4, device="cuda"))
    assert last() == "gpt_prefill_ce_kernel"
