"""An inf or a NaN on its way through the stage-2 kernels (csrc/gpt_prefill.hip, gpt_attn_bwd.hip, gpt_rows.hip, rq_prefill.hip, rq_backward.hip):
causal attention forward / backward (the tile kernels and the RQ depth transformer's short-sequence kernels), LayerNorm + time shift, the strided
LayerNorm, cross-entropy, relu^2 and the embedding gradients — held to tests/nonfinite_util.py as tests/test_nonfinite_vit_kernels_gpu.py holds the
stage-1 kernels: no swallow inside the unit that shares data with the poisoned element, bit-identity with the clean run outside it, and fp16's range
edge exact where the kernel rounds once.

GPTAdam's loss scaler (engine/optim.py) drops a step when the flat gradient holds an inf or NaN; these are the kernels that have to carry an overflow
of the scaled backward there.  Counts of spurious non-finite elements (inside the unit, where fp64 is finite) are printed, not asserted."""
import pytest
import torch

from nonfinite_util import assert_isolated, assert_no_swallow, check_overflow, element_bound, nonfinite, pow2_scale, scrub_shared_buffers  # noqa: F401  (the last: an autouse fixture)
from test_gpt_backward_kernels_gpu import C, _ln_ref  # noqa: F401  (C: the fixture)
from util import U16, elem_bound, h16r

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
INF, NAN = float("inf"), float("nan")
POISONS = (("inf", INF), ("nan", NAN))
SENTINEL = 12345.0


def _nz(x, fill=2.0 ** -6):
    return torch.where(x == 0, torch.full_like(x, fill), x)


def _mask(shape, *index):
    m = torch.zeros(shape, dtype=torch.bool)
    m[index] = True
    return m


# ---- causal attention --------------------------------------------------------------------------------------------------------------------------------
def _causal_run(C, short, qkv, do, B, N, H, D, dt):
    qd, dod = qkv.to(dt).cuda(), do.to(dt).cuda()
    out = torch.full((B, N, H * D), NAN, dtype=dt, device="cuda")
    lse = torch.full((B, H, N), NAN, device="cuda")
    dqkv = torch.full((B, N, 3 * H * D), NAN, dtype=dt, device="cuda")
    if short:
        C.short_causal_attention(qd, B, N, H, D, out, lse)
        C.short_causal_attention_backward(qd, out, dod, lse, B, N, H, D, dqkv)
    else:
        C.causal_attention(qd, B, N, H, D, out, lse)
        C.causal_attention_backward(qd, out, dod, lse, B, N, H, D, dqkv)
    torch.cuda.synchronize()
    return out.cpu(), lse.cpu(), dqkv.cpu()


def _causal_refs(qkv, do, B, N, H, D):
    """the fp64 reference of (sequence 1, head 0): out, lse, dq, dk, dv.  attn_causal_bwd_util.causal_bwd_ref64's formula with one addition: the
    masked probabilities are exact zeros (torch.softmax fills the masked positions of a NaN row with NaN, which P^T dO then carries to keys that row
    never sees); on finite inputs the two agree bit for bit"""
    scale = D ** -0.5
    qt = qkv.double().clone().requires_grad_(True)
    q, k, v = qt.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    mask = ~torch.ones(N, N, dtype=torch.bool).tril()
    s = ((q @ k.transpose(-1, -2)) * scale).masked_fill(mask, float("-inf"))
    p = torch.where(mask, torch.zeros((), dtype=torch.float64), torch.softmax(s, dim=-1))
    out = (p @ v).permute(0, 2, 1, 3).reshape(B, N, H * D)
    out.backward(do.double())
    dq, dk, dv = qt.grad.view(B, N, 3, H * D).unbind(2)
    return dict(out=out.detach()[1, :, :D], lse=torch.logsumexp(s.detach(), dim=-1)[1, 0], dq=dq[1, :, :D], dk=dk[1, :, :D], dv=dv[1, :, :D])


def _check_causal(C, short, B, N, H, D, j, dt):
    """k, v and q of (sequence 1, head 0) poisoned at token j, one at a time.

    Under a causal mask the plain fp64 evaluation on the poisoned input is non-finite in places the poison cannot reach: torch multiplies the masked
    zeros of P and dS into V, K and Q (0 x inf).  The kernels do the same inside the tiles they
    visit and skip the others; neither is wrong.  So the reference is consulted only where the output is a FUNCTION of the poisoned element: where
    the same fp64 evaluation changes when that element moves by +-1 (finite values, exact zeros at the masked positions).  There, wherever fp64 on
    the poisoned input is non-finite, the kernel must be.  Non-finite elements anywhere else inside the unit are counted and printed.
    An infinite key is signed so that the diagonal's score is +inf (a score of -inf is a probability of exactly zero, which harms nothing)."""
    g = torch.Generator().manual_seed(D * 1000 + N + B)
    qkv = _nz(h16r(torch.randn(B, N, 3 * H * D, generator=g) * 1.5, dt))
    do = _nz(h16r(torch.randn(B, N, H * D, generator=g), dt))
    clean = _causal_run(C, short, qkv, do, B, N, H, D, dt)
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean)
    r_clean = _causal_refs(qkv, do, B, N, H, D)
    unit = _mask((B, N, H * D), 1, slice(None), slice(0, D))
    unit3 = _mask((B, N, 3, H * D), 1, slice(None), slice(None), slice(0, D)).view(B, N, 3 * H * D)
    unit_lse = _mask((B, H, N), 1, 0)
    what = f"{'short ' if short else ''}causal attention D={D} B={B} N={N} H={H} {dt}"
    for which, off in (("q", 0), ("k", H * D), ("v", 2 * H * D)):
        depends = {k: torch.zeros_like(v, dtype=torch.bool) for k, v in r_clean.items()}
        for delta in (1.0, -1.0):
            qm = qkv.clone()
            qm[1, j, off + 5] += delta
            for k, v in _causal_refs(qm, do, B, N, H, D).items():
                depends[k] |= v != r_clean[k]
        for pname, pv in POISONS:
            if which == "k" and pv == INF:
                pv = INF if qkv[1, j, 5] > 0 else -INF
            qp = qkv.clone()
            qp[1, j, off + 5] = pv
            out, lse, dqkv = _causal_run(C, short, qp, do, B, N, H, D, dt)
            dq, dk, dv = dqkv.view(B, N, 3, H * D).unbind(2)
            got = dict(out=out[1, :, :D], lse=lse[1, 0], dq=dq[1, :, :D], dk=dk[1, :, :D], dv=dv[1, :, :D])
            tag = f"{what} {pname} in {which} token {j}"
            counts = {}
            for name, r in _causal_refs(qp, do, B, N, H, D).items():
                must = nonfinite(r.to(dt) if name != "lse" else r) & depends[name]
                if name in ("out", "dq", "dk") or which != "v":          # (lse and dv are no functions of v)
                    assert bool(must.any()), f"{tag}: nothing of {name} has to be non-finite: the case checks nothing"
                spurious = assert_no_swallow(got[name], torch.where(must, torch.full_like(r, NAN), torch.zeros_like(r)), f"{tag} {name}")
                counts[name] = (int(must.sum()), spurious)
            if which == "q":       # a poisoned query row touches only that row of out
                assert_isolated(out, clean[0], _mask((B, N, H * D), 1, j, slice(0, D)), tag + " out")
                assert_isolated(lse, clean[1], _mask((B, H, N), 1, 0, j), tag + " lse")
            assert_isolated(out, clean[0], unit, tag + " out")
            assert_isolated(lse, clean[1], unit_lse, tag + " lse")
            assert_isolated(dqkv, clean[2], unit3, tag + " dqkv")
            print(f"{tag}: (elements that must be non-finite, spurious non-finite elsewhere in the unit) " + " ".join(f"{k} {v[0]},{v[1]}" for k, v in counts.items()))


@DTS
@pytest.mark.parametrize("N", [65, 129])
@pytest.mark.parametrize("D", [64, 128, 384])
def test_causal_attention_poisoned_token(C, D, N, dt):
    """key / query 70 of (image 1, head 0) at N = 129 (inside the second tile, seen by rows 70 .. 128 across two query blocks); at N = 65 there is no
    key 70: the poison sits at key 64, the one key of the second tile, seen by the last row alone"""
    _check_causal(C, False, 2, N, 2, D, 70 if N > 70 else N - 1, dt)


@DTS
@pytest.mark.parametrize("D", [64, 128, 384])
def test_short_causal_attention_poisoned_token(C, D, dt):
    """the RQ depth transformer's kernels at (NSEQ, L) = (5, 4): token 2 of sequence 1"""
    _check_causal(C, True, 5, 4, 2, D, 2, dt)


# ---- LayerNorm + time shift, strided LayerNorm ------------------------------------------------------------------------------------------------------------
def _ts_forward64(x, w, b, tm, S):
    M, D = x.shape
    ln = torch.nn.functional.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5).view(M // S, S, D)
    prev = torch.cat([torch.zeros_like(ln[:, :1]), ln[:, :-1]], 1)
    return (ln * tm.double() + prev * (1 - tm.double())).view(M, D)


@DTS
@pytest.mark.parametrize("S", [1, 5])
def test_ln_timeshift_poisoned_row(C, S, dt):
    """forward: a poisoned row of x reaches its own output row and, through the shift, the NEXT position of the same sequence — not the first row of the
    next sequence; backward: a poisoned row of dy reaches its own dx row and the PREVIOUS position's, column c0 of dw, db and dcolscale, nothing else"""
    B, D, b0, c0 = 3, 192, 1, 77
    M = B * S
    g = torch.Generator().manual_seed(S)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    w, b = _nz(1 + 0.1 * torch.randn(D, generator=g)), 0.1 * torch.randn(D, generator=g)
    tm = (0.05 + 0.9 * torch.arange(D) / (D - 1)).float()          # strictly inside (0, 1): both terms of the mix carry the poison
    dy = _nz(torch.randn(M, D, generator=g))
    dev = lambda t: t.cuda()

    def fwd(xx):
        o16, o32 = torch.full((M, D), NAN, dtype=dt, device="cuda"), torch.full((M, D), NAN, device="cuda")
        C.ln_timeshift(dev(xx), dev(w), dev(b), o16, S, colscale=dev(tm), out_f32=o32)
        return o16.cpu(), o32.cpu()

    def bwd(dd):
        dx, dx16 = torch.full((M, D), NAN, device="cuda"), torch.full((M, D), NAN, dtype=dt, device="cuda")
        dw, db, dtm = (torch.full((D,), NAN, device="cuda") for _ in range(3))
        C.ln_timeshift_backward(dev(dd), dev(x), dev(w), S, dx, dw, db, b=dev(b), colscale=dev(tm), dcolscale=dtm, dx16=dx16)
        return dx.cpu(), dx16.cpu(), dw.cpu(), db.cpu(), dtm.cpu()
    cf, cb = fwd(x), bwd(dy)
    assert all(bool(torch.isfinite(t.float()).all()) for t in cf + cb)
    for pname, pv in POISONS:
        for s0 in sorted({0, S // 2, S - 1}):
            r0 = b0 * S + s0
            what = f"ln_timeshift S={S} {dt} {pname} at position {s0}"
            xp = x.clone()
            xp[r0, c0] = pv
            ref = _ts_forward64(xp, w, b, tm, S)
            rows = _mask((M, 1), slice(r0, r0 + (2 if s0 + 1 < S else 1)))
            assert bool(nonfinite(ref[rows[:, 0]]).all()) and bool(torch.isfinite(ref[~rows[:, 0]]).all())
            for name, got, cl in zip(("out16", "out32"), fwd(xp), cf):
                assert assert_no_swallow(got, ref, f"{what} {name}") == 0
                assert_isolated(got, cl, rows, f"{what} {name}")
            dyp = dy.clone()
            dyp[r0, c0] = pv
            dx64, dw64, db64, dtm64 = _ln_ref(x, w, b, tm, S, dyp, None)
            rows = _mask((M, 1), slice(r0 - (1 if s0 > 0 else 0), r0 + 1))
            assert bool(nonfinite(dx64[rows[:, 0]]).all()) and bool(torch.isfinite(dx64[~rows[:, 0]]).all())
            got = bwd(dyp)
            for name, t, cl in zip(("dx", "dx16"), got[:2], cb[:2]):
                assert assert_no_swallow(t, dx64, f"{what} {name}") == 0
                assert_isolated(t, cl, rows, f"{what} {name}")
            colm = _mask((D,), c0)
            for name, t, cl, r in zip(("dw", "db", "dcolscale"), got[2:], cb[2:], (dw64, db64, dtm64)):
                assert bool(nonfinite(r[c0])) or (name == "dcolscale" and S == 1), (what, name)
                assert assert_no_swallow(t, r, f"{what} {name}") == 0
                assert_isolated(t, cl, colm, f"{what} {name}")


@DTS
def test_ln_rows_strided_poisoned_row(C, dt):
    M, D, stride, r0, c0 = 21, 192, 3 * 192, 13, 100
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, D, generator=g) * 2 + 0.3
    w, b = _nz(1 + 0.1 * torch.randn(D, generator=g)), 0.1 * torch.randn(D, generator=g)
    dy = _nz(torch.randn(M, D, generator=g))
    row, colm = _mask((M, 1), r0), _mask((D,), c0)

    def fwd(xx):
        out = torch.full((M, stride), SENTINEL, device="cuda")
        C.ln_rows_strided(xx.cuda(), w.cuda(), b.cuda(), out, stride)
        return out.cpu()

    def bwd(dd):
        dys = torch.full((M, stride), NAN, device="cuda")          # (what lies between the rows is never read: NaN there must change nothing)
        dys[:, :D] = dd.cuda()
        dx, dx16 = torch.full((M, D), NAN, device="cuda"), torch.full((M, D), NAN, dtype=dt, device="cuda")
        dw, db = torch.full((D,), NAN, device="cuda"), torch.full((D,), NAN, device="cuda")
        C.ln_rows_strided_backward(dys, stride, x.cuda(), w.cuda(), dx, dw, db, dx16=dx16)
        return dx.cpu(), dx16.cpu(), dw.cpu(), db.cpu()
    cf, cb = fwd(x), bwd(dy)
    assert bool(torch.isfinite(cf).all()) and all(bool(torch.isfinite(t.float()).all()) for t in cb)
    for pname, pv in POISONS:
        what = f"ln_rows_strided {dt} {pname}"
        xp = x.clone()
        xp[r0, c0] = pv
        ref = torch.nn.functional.layer_norm(xp.double(), (D,), w.double(), b.double(), 1e-5)
        got = fwd(xp)
        assert bool((got[:, D:] == SENTINEL).all()), what + ": wrote between the rows"
        assert assert_no_swallow(got[:, :D], ref, what + " out") == 0
        assert_isolated(got, cf, row, what + " out")
        dyp = dy.clone()
        dyp[r0, c0] = pv
        dx64, dw64, db64, _ = _ln_ref(x, w, b, None, 1, dyp, None)
        gb = bwd(dyp)
        for name, t, cl in zip(("dx", "dx16"), gb[:2], cb[:2]):
            assert assert_no_swallow(t, dx64, f"{what} {name}") == 0
            assert_isolated(t, cl, row, f"{what} {name}")
        for name, t, cl, r in zip(("dw", "db"), gb[2:], cb[2:], (dw64, db64)):
            assert bool(nonfinite(r[c0]))
            assert assert_no_swallow(t, r, f"{what} {name}") == 0
            assert_isolated(t, cl, colm, f"{what} {name}")


# ---- cross-entropy, relu^2, embedding gradients ----------------------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("V", [8, 1000])
def test_cross_entropy_poisoned_logit(C, V, dt):
    """a NaN logit (the target's own, or another one): that row's nll and dlogits are non-finite, the mean follows fp64, every other row keeps its
    bits.  (An infinite logit is left out: softmax in fp64 turns the whole row into NaN where exp(x - lse) gives the limit 0 — neither is wrong.)"""
    M, m0 = 9, 4
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(M, V, generator=g) * 2
    target = torch.randint(0, V, (M,), generator=g)
    target[m0] = 1
    row = _mask((M, 1), m0)

    def run(lg):
        ld, td = lg.cuda(), target.cuda()
        nll0, mean = torch.full((M,), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
        C.cross_entropy_rows(ld, td, nll0, mean)
        nll, dl = torch.full((M,), NAN, device="cuda"), torch.full((M, V), NAN, dtype=dt, device="cuda")
        C.cross_entropy_backward(ld, td, nll, dl, 1.0 / M)
        return nll0.cpu(), mean.cpu(), nll.cpu(), dl.cpu()
    clean = run(logits)
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean)
    for pname, pv in (("nan", NAN),):
        for v0 in (1, V - 1):          # the target's own logit, and another one
            lp = logits.clone()
            lp[m0, v0] = pv
            l64 = lp.double()
            nll64 = torch.logsumexp(l64, -1) - l64[torch.arange(M), target]
            p = torch.softmax(l64, -1)
            p[torch.arange(M), target] -= 1.0
            what = f"cross-entropy V={V} {dt} {pname} at logit {v0}"
            assert bool(nonfinite(nll64[m0]))
            nll0, mean, nll, dl = run(lp)
            assert assert_no_swallow(nll0, nll64, what + " nll") == 0 and assert_no_swallow(nll, nll64, what + " nll (backward)") == 0
            assert assert_no_swallow(mean, nll64.mean().reshape(1), what + " mean") == 0
            n = assert_no_swallow(dl, p / M, what + " dlogits")
            assert_isolated(nll0, clean[0], row[:, 0], what + " nll")
            assert_isolated(nll, clean[2], row[:, 0], what + " nll (backward)")
            assert_isolated(dl, clean[3], row, what + " dlogits")
            print(f"{what}: {n} spurious non-finite dlogits in the row")


@DTS
def test_relu_sq_poisoned_element(C, dt):
    n, i0 = 8 * 1237, 4321
    g = torch.Generator().manual_seed(5)
    h, dy = _nz(torch.randn(n, generator=g) * 2), _nz(torch.randn(n, generator=g))
    h[i0] = 1.5
    elem = _mask((n,), i0)

    def run(hh, dd, ypoison=None):
        y = torch.full((n,), NAN, dtype=dt, device="cuda")
        C.relu_sq(y, hh.cuda())
        yin = y.clone()
        C.relu_sq(yin)                        # the in-place form on 16-bit values: relu(y)^2 of y = relu(h)^2 >= 0
        if ypoison is not None:
            y[i0] = ypoison
        dx = torch.full((n,), NAN, dtype=dt, device="cuda")
        C.relu_sq_backward(dd.cuda(), y, dx)
        return y.cpu(), yin.cpu(), dx.cpu()
    clean = run(h, dy)
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean)
    for pname, pv in POISONS:
        what = f"relu_sq {dt} {pname}"
        hp = h.clone()
        hp[i0] = pv
        y, yin, dx = run(hp, dy)
        ref = torch.square(torch.relu(hp.double()))
        assert bool(nonfinite(ref[i0]))
        assert assert_no_swallow(y, ref, what + " forward") == 0
        assert assert_no_swallow(yin, torch.square(torch.relu(ref.to(dt).double())), what + " forward in place") == 0
        assert assert_no_swallow(dx, dy.double() * 2 * torch.sqrt(ref.to(dt).double()), what + " backward from the stored y") == 0
        for name, t, cl in zip(("forward", "forward in place", "backward"), (y, yin, dx), clean):
            assert_isolated(t, cl, elem, f"{what} {name}")
        dyp = dy.clone()
        dyp[i0] = pv
        _, _, dx = run(h, dyp)
        assert assert_no_swallow(dx, dyp.double() * 2 * torch.relu(h.double()), what + " in dy") == 0
        assert_isolated(dx, clean[2], elem, what + " in dy")


def test_embed_seq_backward_poisoned_gradient_row(C):
    """a poisoned element of g reaches exactly the table rows its ids name (column c0 of them)"""
    B, T, Cw, Vc, V, b0, c0 = 5, 70, 1032, 4, 19, 2, 1030
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(B, T, Cw, generator=gen)
    conds = torch.randint(0, Vc, (B,), generator=gen)
    codes = torch.randint(0, V, (B, T), generator=gen)
    shapes = ((Vc, Cw), (Cw,), (V, Cw), (T, Cw))

    def run(gg):
        out = [torch.full(s, NAN, device="cuda") for s in shapes]
        C.gpt_embed_seq_backward(gg.cuda(), conds.cuda(), codes.cuda(), *out)
        return [o.cpu() for o in out]

    def ref64(gg):
        r = [torch.zeros(s, dtype=torch.float64) for s in shapes]
        gd = gg.double()
        r[0].index_add_(0, conds, gd[:, 0])
        r[1] += gd[:, 0].sum(0)
        r[2].index_add_(0, codes[:, :T - 1].reshape(-1), gd[:, 1:].reshape(-1, Cw))
        r[3][:T - 1] += gd[:, 1:].sum(0)
        return r
    clean = run(g)
    for pname, pv in POISONS:
        for s0 in (0, 3, T - 1):
            gp = g.clone()
            gp[b0, s0, c0] = pv
            ref = ref64(gp)
            masks = [torch.zeros(s, dtype=torch.bool) for s in shapes]
            if s0 == 0:
                masks[0][conds[b0], c0] = True
                masks[1][c0] = True
            else:
                masks[2][codes[b0, s0 - 1], c0] = True
                masks[3][s0 - 1, c0] = True
            for name, got, cl, r, m in zip(("tok_cond", "pos_cond", "tok_code", "pos_code"), run(gp), clean, ref, masks):
                what = f"gpt_embed_seq_backward {pname} at position {s0}: {name}"
                assert torch.equal(nonfinite(r), m), what + ": the reference disagrees with the ids"
                assert assert_no_swallow(got, r, what) == 0
                if bool(m.any()):
                    assert_isolated(got, cl, m, what)
                else:
                    assert torch.equal(got.view(torch.int32), cl.view(torch.int32)), what + ": a table no id of the poisoned row names changed"


def test_rq_embed_seq_backward_poisoned_gradient_row(C):
    B, T, D, Cw, V, Vc, b0, t0, j0, c0 = 2, 6, 4, 136, 9, 4, 1, 3, 2, 133
    gen = torch.Generator().manual_seed(7)
    gs, gd = torch.randn(B, T, Cw, generator=gen), torch.randn(B * T, D, Cw, generator=gen)
    conds = torch.randint(0, Vc, (B,), generator=gen)
    codes = torch.randint(0, V, (B, T, D), generator=gen)
    shapes = ((Vc, Cw), (Cw,), (V, Cw), (T + 1, Cw), (D - 1, Cw))

    def run(gs_, gd_):
        gdd = gd_.clone()
        gdd[:, 0] = NAN                                                # slot 0 belongs to ln_spatial: never read here
        out = [torch.full(s, NAN, device="cuda") for s in shapes]
        C.rq_embed_seq_backward(gs_.cuda(), gdd.cuda(), conds.cuda(), codes.cuda(), *out)
        return [o.cpu() for o in out]

    def ref64(gs_, gd_):
        """what every fed occurrence (b, t, j) of a code receives: the depth slots behind it, and the next position's spatial row"""
        gs_, gd_ = gs_.double(), gd_.double().view(B, T, D, Cw)
        r = [torch.zeros(s, dtype=torch.float64) for s in shapes]
        r[0].index_add_(0, conds, gs_[:, 0])
        r[1] += gs_[:, 0].sum(0)
        for b_ in range(B):
            for t in range(T):
                for j in range(D):
                    if t == T - 1 and j == D - 1:
                        continue                                       # the deepest code of the last position is never fed
                    u = gd_[b_, t, j + 1:].sum(0)
                    if t < T - 1:
                        u = u + gs_[b_, t + 1]
                    r[2][codes[b_, t, j]] += u
        r[3][:T - 1] += gs_[:, 1:].sum(0)
        r[4] += gd_[:, :, 1:].sum((0, 1))
        return r
    clean = run(gs, gd)
    for pname, pv in POISONS:
        for where in ("gs", "gd"):
            gsp, gdp = gs.clone(), gd.clone()
            masks = [torch.zeros(s, dtype=torch.bool) for s in shapes]
            if where == "gs":          # the spatial row of position t0: every depth's code of position t0 - 1, and pos_code[t0 - 1]
                gsp[b0, t0, c0] = pv
                masks[2][codes[b0, t0 - 1], c0] = True
                masks[3][t0 - 1, c0] = True
            else:                      # depth slot j0 of (b0, t0): the codes in front of it, and pos_depth[j0 - 1]
                gdp[b0 * T + t0, j0, c0] = pv
                masks[2][codes[b0, t0, :j0], c0] = True
                masks[4][j0 - 1, c0] = True
            ref = ref64(gsp, gdp)
            for name, got, cl, r, m in zip(("tok_cond", "pos_cond", "tok_code", "pos_code", "pos_depth"), run(gsp, gdp), clean, ref, masks):
                what = f"rq_embed_seq_backward {pname} in {where}: {name}"
                assert torch.equal(nonfinite(r), m), what + ": the reference disagrees with the ids"
                assert assert_no_swallow(got, r, what) == 0
                if bool(m.any()):
                    assert_isolated(got, cl, m, what)
                else:
                    assert torch.equal(got.view(torch.int32), cl.view(torch.int32)), what + ": a table no id of the poisoned row names changed"


# ---- fp16's range edge ---------------------------------------------------------------------------------------------------------------------------------
def test_fp16_overflow_of_the_row_kernels_is_exact(C):
    """relu^2 with |h| > 256, its backward, cross-entropy backward under gscale = 2^24 and the 16-bit output of ln_timeshift: +-inf exactly where
    fp16(ref) is, the rest inside the bound of each kernel's own per-element test"""
    g = torch.Generator().manual_seed(11)
    n = 8 * 1237
    h = torch.randn(n, generator=g) * 300
    y = torch.full((n,), NAN, dtype=F16, device="cuda")
    C.relu_sq(y, h.cuda())
    ref = torch.square(torch.relu(h.double()))
    check_overflow(y, ref, element_bound((U16[F16] + 2.0 ** -23) * ref + 2.0 ** -24), "relu_sq", exact=True)      # tests/test_gpt_prefill_kernels_gpu.py test_relu_sq
    # backward: dx = dy * 2 relu(h) from the stored y = relu(h)^2 (finite here), dy scaled past the range of dx
    h = torch.randn(n, generator=g) * 2
    dy = torch.randn(n, generator=g)
    dy = dy * pow2_scale((dy.double() * 2 * torch.relu(h.double()))[h > 0])
    y = torch.empty(n, dtype=F16, device="cuda")
    C.relu_sq(y, h.cuda())
    dx = torch.full((n,), NAN, dtype=F16, device="cuda")
    C.relu_sq_backward(dy.cuda(), y, dx)
    # the operation is a function of what it is GIVEN, the stored y: dx = dy * 2 sqrt(y), one f32 square root and two products, rounded once
    ref = dy.double() * 2 * torch.sqrt(y.double().cpu())
    check_overflow(dx, ref, element_bound(elem_bound(ref, ref.abs(), 1, F16)), "relu_sq_backward", exact=True)
    # cross-entropy backward under a loss scale of 2^24: probabilities above 2^-8 overflow
    M, V, gscale = 9, 1000, 2.0 ** 24
    logits, target = torch.randn(M, V, generator=g) * 2, torch.randint(0, V, (M,), generator=g)
    nll, dl = torch.empty(M, device="cuda"), torch.full((M, V), NAN, dtype=F16, device="cuda")
    C.cross_entropy_backward(logits.cuda(), target.cuda(), nll, dl, gscale)
    p = torch.softmax(logits.double(), -1)
    onehot = torch.zeros(M, V, dtype=torch.float64)
    onehot[torch.arange(M), target] = 1.0
    ref = (p - onehot) * gscale
    check_overflow(dl, ref, element_bound(elem_bound(ref, (p + onehot) * gscale, V, F16)), "cross_entropy_backward gscale 2^24", exact=True)
    # ln_timeshift's 16-bit output with a large w.  tests/test_gpt_prefill_kernels_gpu.py test_ln_timeshift holds it to u |ref| + 1e-6 at unit scale;
    # w carries a power of two s here, which scales the f32 error term exactly: u |ref| + 1e-6 s
    B, S, D = 2, 5, 192
    x = torch.randn(B * S, D, generator=g) * 2 + 0.3
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    tm = (torch.arange(D) / (D - 1) + 0.05 * torch.randn(D, generator=g)).float()
    s = pow2_scale(_ts_forward64(x, w, b, tm, S))
    w, b = w * s, b * s
    ref = _ts_forward64(x, w, b, tm, S)
    o16 = torch.full((B * S, D), NAN, dtype=F16, device="cuda")
    C.ln_timeshift(x.cuda(), w.cuda(), b.cuda(), o16, S, colscale=tm.cuda())
    check_overflow(o16, ref, element_bound(U16[F16] * ref.abs() + 1e-6 * s), "ln_timeshift 16-bit output", exact=True)
