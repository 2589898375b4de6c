"""The kernels of the stage-2 backward (csrc/gpt_attn_bwd.hip, the backward half of csrc/gpt_rows.hip), each against fp64 on the values it is given.

Causal attention backward, every head width x N in {1, 63, 64, 65, 129, 200} (one token; a ragged tile; an aligned tile; a second tile holding one
key; a second query / key block with one row, three tiles; both ring stages and a ragged tile on the diagonal), B = H = 2 at N = 65, both formats.
Limits: ATT_MARGIN x the worst D-wide row of the rounding model (tests/attn_causal_bwd_util.py) given the kernel's own out and lse; util.elem_bound
for the row kernels."""
import pytest
import torch

from attn_causal_bwd_util import causal_bwd_model, causal_bwd_ref64
from attn_causal_util import ATT_MARGIN
from attn_dh_util import assert_rows_within, worst_rows
from util import U16, assert_elementwise, elem_bound, h16r

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
WIDTHS = [64, 128, 192, 256, 320, 384]
TOKENS = [1, 63, 64, 65, 129, 200]
GUARD_ROWS = 64
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


# ---- causal attention backward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("N", TOKENS)
@pytest.mark.parametrize("D", WIDTHS)
def test_causal_attention_backward_against_fp64(C, D, N, dt):
    B = H = 2 if N == 65 else 1
    scale = D ** -0.5
    g = torch.Generator().manual_seed(D * 1000 + N)
    qkv = h16r(torch.randn(B, N, 3 * H * D, generator=g) * 1.5, dt)
    do = h16r(torch.randn(B, N, H * D, generator=g), dt)
    qd, dod = qkv.to(dt).cuda(), do.to(dt).cuda()
    out = torch.full((B, N, H * D), float("nan"), dtype=dt, device="cuda")
    lse = torch.full((B, H, N), float("nan"), device="cuda")
    C.causal_attention(qd, B, N, H, D, out, lse)
    runs = []
    for _ in range(2):
        whole = torch.empty(qd.numel() + GUARD_ROWS * 3 * H * D, dtype=dt, device="cuda")
        whole[:qd.numel()] = float("nan")
        whole[qd.numel():] = SENTINEL
        dqkv = whole[:qd.numel()].view(B, N, 3 * H * D)
        C.causal_attention_backward(qd, out, dod, lse, B, N, H, D, dqkv)
        torch.cuda.synchronize()
        assert bool((whole[qd.numel():] == SENTINEL).all()), "wrote past dqkv"
        runs.append(dqkv)
    what = f"causal attention backward D={D} B={B} N={N} H={H} {dt}"
    assert bool(torch.isfinite(runs[0].float()).all()), what + ": an element was never written"
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), what + ": two runs differ"
    got = [t.contiguous() for t in runs[0].view(B, N, 3, H * D).unbind(2)]
    if N == 1:      # one key: P = 1, dS = 0 whatever the values, and dV is dO itself
        assert bool((got[0] == 0).all()) and bool((got[1] == 0).all()) and torch.equal(got[2].view(torch.int16), dod.view(torch.int16))
        return
    ref = causal_bwd_ref64(qkv, do, B, N, H, D, scale)
    model = causal_bwd_model(qkv, do, out, lse, B, N, H, D, scale, dt)
    ratios = []
    for name, t, r_, m_ in zip(("dq", "dk", "dv"), got, ref, model):
        m = worst_rows(m_, r_, H, D)
        assert m == m and m > 0, (what, name, m)
        ratios.append(assert_rows_within(t, r_, H, D, ATT_MARGIN * m, f"{what} {name}") / m)
    print(f"{what}: worst row / the model's worst row: dq {ratios[0]:.3f} dk {ratios[1]:.3f} dv {ratios[2]:.3f}")


# ---- cross-entropy backward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("V", [8, 1000, 16384])
def test_cross_entropy_backward(C, V, dt):
    M = 9
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(M, V, generator=g) * 2)
    target = torch.randint(0, V, (M,), generator=g)
    target[0], target[1] = 0, V - 1
    logits[2, V // 2] += 30.0       # a row carried by one logit whose target is elsewhere
    target[2] = 0 if V // 2 != 0 else 1
    ld, td = logits.cuda(), target.cuda()
    nll0 = torch.empty(M, device="cuda")
    C.cross_entropy_rows(ld, td, nll0)
    p = torch.softmax(logits.double(), dim=-1)
    onehot = torch.zeros(M, V, dtype=torch.float64)
    onehot[torch.arange(M), target] = 1.0
    for gscale in (1.0 / M, 1024.0):
        nll = torch.full((M,), float("nan"), device="cuda")
        dl = torch.full((M, V), float("nan"), dtype=dt, device="cuda")
        C.cross_entropy_backward(ld, td, nll, dl, gscale)
        assert torch.equal(nll.view(torch.int32), nll0.view(torch.int32)), "nll is not enh_cross_entropy_rows' bits"
        ref = (p - onehot) * gscale
        # p = exp(x - max) / l: the f32 error of the row sum l (V terms) and of exp moves p relatively, so `mag` is p itself (+ the one-hot) and k = V
        w = assert_elementwise(dl, ref, elem_bound(ref, (p + onehot) * gscale, V, dt), f"dlogits V={V} {dt} gscale={gscale}")
        print(f"cross-entropy backward V={V} {dt} gscale={gscale:g}: worst element / bound {w:.3f}")


# ---- relu^2 backward ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [8, 8 * 1237])
def test_relu_sq_backward(C, n, dt):
    g = torch.Generator().manual_seed(n)
    h = torch.randn(n, generator=g) * 2
    h[1], h[2], h[3] = 0.0, -3.0, 1.5
    dy = torch.randn(n, generator=g)
    y = torch.empty(n, dtype=dt, device="cuda")
    C.relu_sq(y, h.cuda())      # what the forward keeps: relu(h)^2 in the operand format
    dx = torch.full((n,), float("nan"), dtype=dt, device="cuda")
    C.relu_sq_backward(dy.cuda(), y, dx)
    ref = dy.double() * 2 * torch.relu(h.double())
    # relu(h) = sqrt(y), y within u (+ the subnormal step) of h^2: half of that relative error, then the f32 sqrt / products and one rounding of dx
    bound = elem_bound(ref, ref.abs(), 1, dt) + 0.5 * U16[dt] * ref.abs()
    if dt == F16:      # y below fp16's normal range (h^2 < 2^-14) is kept to e = 2^-25 absolutely: |sqrt(y') - sqrt(y)| <= min(e / sqrt(y), sqrt(e))
        hh = torch.relu(h.double()).clamp_min(1e-300)
        bound = bound + 2 * dy.double().abs() * torch.minimum(2.0 ** -25 / hh, torch.full_like(hh, 2.0 ** -12.5))
    assert_elementwise(dx, ref, bound, f"relu_sq_backward n={n} {dt}")
    assert bool((dx.cpu()[h <= 0] == 0).all())


# ---- LayerNorm + time shift backward -------------------------------------------------------------------------------------------------------------------
def _ln_ref(x, w, b, tm, S, dy, dres):
    """fp64 autograd of the forward formula: (dx, dw, db, dtm, the magnitudes of their sums)"""
    B, D = x.shape[0] // S, x.shape[1]
    xd, wd, bd = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    tmd = None if tm is None else tm.double().clone().requires_grad_(True)
    ln = torch.nn.functional.layer_norm(xd, (D,), wd, bd, 1e-5).view(B, S, D)
    y = ln
    if tm is not None:
        prev = torch.cat([torch.zeros_like(ln[:, :1]), ln[:, :-1]], 1)
        y = ln * tmd + prev * (1 - tmd)
    y.reshape(B * S, D).backward(dy.double())
    dx = xd.grad + (0 if dres is None else dres.double())
    return dx, wd.grad, bd.grad, None if tm is None else tmd.grad


@pytest.mark.parametrize("mode", ["plain", "mix", "mix_dres_acc", "plain_dres_acc"])
@pytest.mark.parametrize("BS", [(3, 1), (2, 5), (1, 131)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", [128, 768])
def test_ln_timeshift_backward(C, D, BS, mode):
    B, S = BS
    M = B * S
    g = torch.Generator().manual_seed(D + 10 * M)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    tm = (torch.arange(D) / (D - 1) + 0.05 * torch.randn(D, generator=g)).float() if mode.startswith("mix") else None
    dy = torch.randn(M, D, generator=g)
    extra = mode.endswith("dres_acc")
    dres = torch.randn(M, D, generator=g) if extra else None
    old = [torch.randn(D, generator=g) for _ in range(3)]
    dx64, dw64, db64, dtm64 = _ln_ref(x, w, b, tm, S, dy, dres)
    dev = lambda t: None if t is None else t.cuda()
    dx = torch.full((M, D), float("nan"), device="cuda")
    dx16 = torch.full((M, D), float("nan"), dtype=F16, device="cuda")
    dw, db, dtm = (o.clone().cuda() if extra else torch.full((D,), float("nan"), device="cuda") for o in old)
    C.ln_timeshift_backward(dev(dy), dev(x), dev(w), S, dx, dw, db, b=dev(b), colscale=dev(tm), dcolscale=dtm if tm is not None else None, dres=dev(dres),
                            dx16=dx16, accumulate=extra)
    # magnitudes: the same sums on absolute values.  xhat and rstd come from f32 row statistics (two sums of D terms), so every term carries ~D more
    # roundings than its own sum: k = D + the number of summed terms
    xd = x.double()
    mean, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-5)
    xh = (xd - mean) * rstd
    dyd = dy.double().view(B, S, D)
    gl = dyd
    if tm is not None:
        nxt = torch.cat([dyd[:, 1:], torch.zeros_like(dyd[:, :1])], 1)
        gl = dyd * tm.double() + nxt * (1 - tm.double())
        # the last row of every batch element receives nothing from the next element
        assert torch.equal(gl[:, -1], dyd[:, -1] * tm.double())
    gl = gl.reshape(M, D)
    gw = gl.abs() * w.double().abs()
    mag_dx = (gw + gw.mean(-1, keepdim=True) + xh.abs() * (gw * xh.abs()).mean(-1, keepdim=True)) * rstd + (0 if dres is None else dres.double().abs())
    o = [t.double() if extra else torch.zeros(D, dtype=torch.float64) for t in old]
    what = f"ln_timeshift_backward D={D} B={B} S={S} {mode}"
    assert_elementwise(dx, dx64, elem_bound(dx64, mag_dx, 3 * D), what + " dx")
    assert torch.equal(dx16, dx.to(F16)), what + ": the 16-bit copy is not the rounded dx"
    assert_elementwise(dw, dw64 + o[0], elem_bound(dw64, (gl.abs() * xh.abs()).sum(0) + o[0].abs(), D + M), what + " dw")
    assert_elementwise(db, db64 + o[1], elem_bound(db64, gl.abs().sum(0) + o[1].abs(), M), what + " db")
    if tm is not None:
        ln = (xh * w.double() + b.double()).view(B, S, D)
        prev = torch.cat([torch.zeros_like(ln[:, :1]), ln[:, :-1]], 1)
        mag = (dyd.abs() * (ln.abs() + prev.abs())).sum((0, 1))
        assert_elementwise(dtm, dtm64 + o[2], elem_bound(dtm64, mag + o[2].abs(), D + 2 * M), what + " dcolscale")


# ---- embedding backward ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
def test_embed_seq_backward(C, accumulate):
    B, T, Cw, Vc, V = 5, 70, 1032, 4, 19      # 5 x 69 = 345 fed codes: two rounds of 256 ids; 1032 columns: two column blocks
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(B, T, Cw, generator=gen)
    conds = torch.randint(0, Vc - 1, (B,), generator=gen)      # condition Vc - 1 does not occur
    codes = torch.randint(0, V - 2, (B, T), generator=gen)     # codes V - 2 and V - 1 are not fed ...
    codes[:, T - 1] = V - 1                                    # ... although V - 1 is every sequence's LAST code: never fed, no gradient
    old = [torch.randn(s, generator=gen) for s in ((Vc, Cw), (Cw,), (V, Cw), (T, Cw))]
    out = [o.clone().cuda() if accumulate else torch.full(o.shape, float("nan"), device="cuda") for o in old]
    C.gpt_embed_seq_backward(g.cuda(), conds.cuda(), codes.cuda(), *out, accumulate=accumulate)
    # the same sums in torch, f32, ascending (b, s): start from zero, add the rows one by one, add what was there last
    ref = [torch.zeros_like(o) for o in old]
    for b_ in range(B):
        ref[0][conds[b_]] += g[b_, 0]
        ref[1] += g[b_, 0]
        for s in range(1, T):
            ref[2][codes[b_, s - 1]] += g[b_, s]
    for s in range(1, T):
        for b_ in range(B):
            ref[3][s - 1] += g[b_, s]
    if accumulate:
        ref = [r_ + o for r_, o in zip(ref, old)]
    for name, got, r_ in zip(("tok_cond", "pos_cond", "tok_code", "pos_code"), out, ref):
        assert torch.equal(got.cpu().view(torch.int32), r_.view(torch.int32)), name
    if not accumulate:
        assert bool((out[0][Vc - 1] == 0).all()) and bool((out[2][V - 2:] == 0).all()) and bool((out[3][T - 1] == 0).all())
