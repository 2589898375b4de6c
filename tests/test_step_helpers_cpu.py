"""The limits of tests/step_helpers_util.py have teeth: for every helper-kernel family of a stage-1 step an f32 torch restatement of the kernel's
arithmetic (the same grouping of the sums where it matters: lanes, waves, chunks and the fixed-order second pass) stays within its limit, and each
fault injected into the restatement raises.  Every test prints max(err / bound) of the honest restatement and, per fault, whether TODAY's assertion
(the whole-tensor limits of tests/test_ops_gpu.py and tests/test_fp16_gpu.py, restated: rel <= F32_TOL, rel(p) <= 1e-6, ...) lets it through.

Faults that pass today's assertions (the evidence that the suite was blind there): AdamW without weight decay, AdamW with eps inside the square
root, dpix with sign(0) = +1, unpatchify with gx_n and gy_n exchanged (today's one geometry is square).  The others are reported as they fall.
"""
import pytest
import torch

from gpt_train_util import check_limit
from step_helpers_util import (BF16, F16, F32, F64, TorchAdamW, adamw_check, bits_equal, check, colsum_exact, colsum_ref, dyadic, from_patches, gemm_f32_ref,
                               int_matrix, ln_ref, pixel_loss_ref, to_patches)
from util import h16r, rel

F32_TOL, BF16_TOL = 1e-5, 2.5e-3          # today's whole-tensor limits (tests/test_ops_gpu.py)


def _raises(fn, what: str, today=None):
    """fn() must raise an AssertionError (the new check sees the fault); prints what today's assertion says about the same fault"""
    with pytest.raises(AssertionError) as e:
        fn()
    t = "" if today is None else f"; today's assertion {'PASSES it' if today else 'fails it too'}"
    print(f"fault: {what}: flagged{t}  [{str(e.value)[:160]}]")


# ---- column sums ------------------------------------------------------------------------------------------------------------------------------------
def _seqsum(rows: torch.Tensor) -> torch.Tensor:
    a = torch.zeros(rows.shape[1:], dtype=F32)
    for r in rows:
        a = a + r
    return a


def _rowsum16(part: torch.Tensor) -> torch.Tensor:
    """common.h fixed_order_rowsum16: 16 contiguous groups of rows, ascending inside a group, the group sums added in ascending order"""
    rows = part.shape[0]
    per = (rows + 15) // 16
    t = torch.zeros(part.shape[1:], dtype=F32)
    for g in range(16):
        t = t + _seqsum(part[min(g * per, rows):min(g * per + per, rows)])
    return t


def colsum_restated(x: torch.Tensor, old=None, lost_row=None, lost_block: bool = False) -> torch.Tensor:
    """enh_colsum_h16_ws in f32 torch: chunks of rows (at most 256), four waves per chunk taking every fourth row, wave 0 adding the others' partials,
    then the fixed-order second pass.  lost_row = (chunk, column block): that chunk drops its last row in that 512-column block; lost_block: the
    ragged last 512-column block is never summed."""
    M, N = x.shape
    chunks = min(256, (M + 511) // 512)
    rpb = (M + chunks - 1) // chunks
    part = torch.zeros(chunks, N, dtype=F32)
    for y in range(chunks):
        lo, hi = y * rpb, min(M, y * rpb + rpb)
        waves = [_seqsum(x[lo + w:hi:4]) for w in range(4)]
        if lost_row is not None and lost_row[0] == y:
            c0 = lost_row[1] * 512
            w = (hi - 1 - lo) % 4
            waves[w][c0:c0 + 512] = _seqsum(x[lo + w:hi - 1:4])[c0:c0 + 512]
        part[y] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    t = _rowsum16(part)
    if lost_block:
        t[(N - 1) // 512 * 512:] = 0.0
    return t if old is None else old + t


def test_column_sums():
    M, N = 1031, 520
    xi = int_matrix(M, N, 1)
    assert bits_equal(colsum_restated(xi), colsum_exact(xi))
    g = torch.Generator().manual_seed(2)
    x = h16r(torch.randn(M, N, generator=g), BF16)
    old = torch.randn(N, generator=g)
    ref, bound = colsum_ref(x, old)
    w = check(colsum_restated(x, old), ref, bound, "column sums")
    print(f"honest column sums {M}x{N} (3 chunks, ragged second block): integer data bit-exact, Gaussian max err / bound {w:.4f}")
    assert w <= 1.0
    ref0, bound0 = colsum_ref(x)
    for what, kw in (("lost the last row of chunk 1 in column block 0", dict(lost_row=(1, 0))), ("lost the ragged last column block (N = 520)", dict(lost_block=True))):
        bad = colsum_restated(x, **kw)
        today = rel(bad, ref0) <= F32_TOL
        _raises(lambda: check(bad, ref0, bound0, what), "column sum " + what + ", Gaussian data", today)
        assert not bits_equal(colsum_restated(xi, **kw), colsum_exact(xi)), what + ": the exact check misses it"


# ---- unpatchify + pixel loss ----------------------------------------------------------------------------------------------------------------------
def unpatchify_restated(pix, target, B, C, H, W, p, w_l1, w_l2, dt, swap: bool = False, sign0: bool = False):
    """unpatchify_loss_kernel in f32 torch: the kernel's index arithmetic per element, a lane's four terms added in order, the xor butterfly of a wave,
    (s0 + s1) + (s2 + s3) per workgroup, then f64.  swap: gx_n and gy_n exchanged; sign0: sign(0) taken as +1."""
    numel = B * C * H * W
    gx_n, gy_n = (H // p, W // p) if swap else (W // p, H // p)
    r = torch.arange(numel)
    pw = r % p; r = r // p
    ph = r % p; r = r // p
    c = r % C; r = r // C
    gx, gy, b = r % gx_n, (r // gx_n) % gy_n, r // (gx_n * gy_n)
    off = ((b * C + c) * H + gy * p + ph) * W + gx * p + pw
    v = pix.reshape(-1)
    xrec = torch.full((numel,), float("nan"))
    off = off % numel          # (a faulty index may leave the image: what a restatement can do with it is wrap)
    xrec[off] = v
    d = v - target.reshape(-1)[off]
    sg = torch.where(d >= 0, 1.0, -1.0) if sign0 else torch.sign(d)
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(numel), dtype=F32)
    g = ((torch.tensor(w_l1, dtype=F32) * sg + torch.tensor(w_l2, dtype=F32) * 2.0 * d) * inv).to(dt)
    sums = torch.zeros(2, dtype=F64)
    pad = (-numel) % 1024
    for k, t in enumerate((d.abs(), d * d)):
        t = torch.cat([t, torch.zeros(pad)]).view(-1, 4, 64, 4)          # workgroup, wave, lane, element
        lane = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
        idx = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[..., idx ^ o]
        wv = lane[..., 0]
        sums[k] = ((wv[:, 0] + wv[:, 1]) + (wv[:, 2] + wv[:, 3])).double().sum()
    return xrec.view(B, C, H, W), sums, g.view(-1, C * p * p)


def _unpatchify_checks(pix, target, p, w_l1, w_l2, dt, got, what, exact_sums=False):
    B, C, H, W = target.shape
    xrec, sums, g = got
    assert bits_equal(xrec, from_patches(pix, B, C, H, W, p)), what + ": xrec is not the permutation"
    s_ref, g_ref, s_bound, g_bound = pixel_loss_ref(pix, target, p, w_l1, w_l2, 1.0, dt)
    if exact_sums:
        assert torch.equal(sums, s_ref), what + ": sums are not exact"
    return max(check(sums, s_ref, s_bound, what + " sums"), check(g, g_ref, g_bound, what + " dpix"))


def test_unpatchify_and_pixel_loss():
    gen = torch.Generator().manual_seed(3)
    B, C, H, W, p = 2, 3, 16, 32, 8
    pix, target = torch.randn(B * (H // p) * (W // p), C * p * p, generator=gen), torch.rand(B, C, H, W, generator=gen)
    for dt in (BF16, F16):
        w = _unpatchify_checks(pix, target, p, 0.3, 1.0, dt, unpatchify_restated(pix, target, B, C, H, W, p, 0.3, 1.0, dt), f"unpatchify {dt}")
        print(f"honest unpatchify + loss 2x3x16x32 p=8 {dt}: max err / bound {w:.3f}")
        assert w <= 1.0
    pd, td = dyadic(pix.shape, 4), dyadic(target.shape, 5)
    _unpatchify_checks(pd, td, p, 0.3, 1.0, BF16, unpatchify_restated(pd, td, B, C, H, W, p, 0.3, 1.0, BF16), "dyadic grid", exact_sums=True)

    # gx_n <-> gy_n: today's geometry is square (3 x 3 x 64 x 64, p = 8), where the exchange changes nothing
    S = 64
    ps, ts = torch.randn(3 * (S // p) ** 2, 3 * p * p, generator=gen), torch.rand(3, 3, S, S, generator=gen)
    a, b = unpatchify_restated(ps, ts, 3, 3, S, S, p, 0.3, 1.0, BF16), unpatchify_restated(ps, ts, 3, 3, S, S, p, 0.3, 1.0, BF16, swap=True)
    today = all(bits_equal(u, v) for u, v in zip(a, b))
    assert today, "gx_n / gy_n exchanged no longer passes today's square case: it documents nothing"
    _raises(lambda: _unpatchify_checks(pix, target, p, 0.3, 1.0, BF16, unpatchify_restated(pix, target, B, C, H, W, p, 0.3, 1.0, BF16, swap=True), "swap"),
            "unpatchify with gx_n and gy_n exchanged, 16 x 32 image", today)

    # sign(0) = +1: today's operands (randn against rand) never meet, so no element has d == 0
    a, b = unpatchify_restated(ps, ts, 3, 3, S, S, p, 0.3, 1.0, BF16), unpatchify_restated(ps, ts, 3, 3, S, S, p, 0.3, 1.0, BF16, sign0=True)
    today = bits_equal(a[2], b[2])
    assert today, "sign(0) = +1 no longer passes today's case"
    planted = pix.clone()
    tp = to_patches(target, p)
    planted[::3, ::5] = tp[::3, ::5]
    for w1, w2 in ((1.0, 0.0), (0.3, 1.0)):
        _raises(lambda: _unpatchify_checks(planted, target, p, w1, w2, BF16, unpatchify_restated(planted, target, B, C, H, W, p, w1, w2, BF16, sign0=True), "sign0"),
                f"dpix with sign(0) = +1, w_l1 = {w1}, planted pix == target", today)
    _unpatchify_checks(planted, target, p, 1.0, 0.0, BF16, unpatchify_restated(planted, target, B, C, H, W, p, 1.0, 0.0, BF16), "planted, honest")


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------------------------------
def adamw_restated(p, g, m, v, step, lr, wd, b1=0.9, b2=0.99, eps=1e-8, no_wd=False, eps_in_sqrt=False, bc2_prev=False):
    """adamw_kernel in f32 torch (in place); the host's bias corrections in double, handed over as f32"""
    f = lambda x: torch.tensor(x, dtype=F32)
    bc1, t2 = 1.0 - b1 ** step, (step - 1 if bc2_prev else step)
    bc2 = 1.0 - b2 ** t2
    inv_bc1, inv_sqrt_bc2 = f(1.0 / bc1), f(1.0 / bc2 ** 0.5 if bc2 > 0 else float("inf"))
    if not no_wd:
        p.mul_(f(1.0) - f(lr) * f(wd))
    m.copy_(m * f(b1) + g * (f(1.0) - f(b1)))
    v.copy_(v * f(b2) + g * g * (f(1.0) - f(b2)))
    denom = torch.sqrt(v * inv_sqrt_bc2 * inv_sqrt_bc2 + f(eps)) if eps_in_sqrt else torch.sqrt(v) * inv_sqrt_bc2 + f(eps)
    p.sub_((f(lr) * inv_bc1) * (m / denom))


def adamw_case(n: int, seed: int):
    """parameters and the gradients of the issue: most about 1e-2, a slice about 1e-8, a slice exactly zero, one element 1e3"""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 1e-2
    if n >= 8:
        s = max(1, n // 8)
        g[s:2 * s] = torch.randn(s, generator=gen) * 1e-8
        g[2 * s:3 * s] = 0.0
        g[n - 1] = 1e3
    return p, g


STEPS = (1, 2, 3, 1000, 100000)


def _adamw_run(n, lr, wd, **fault):
    p0, g = adamw_case(n, 7)
    f32, ref = TorchAdamW(p0, F32, lr, wd), TorchAdamW(p0, F64, lr, wd)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    worst = 0.0
    for t in STEPS:
        gt = g * (1.0 + 0.25 * (t % 3))
        adamw_restated(p, gt, m, v, t, lr, wd, **fault)
        worst = max(worst, adamw_check((p, m, v), f32.step(gt, t), ref.step(gt, t), f"AdamW n={n} lr={lr} wd={wd} step {t}"))
    return worst


def _adamw_today(**fault):
    """tests/test_ops_gpu.py test_colsum_cast_adamw restated: lr 4.5e-6, wd 1e-4, g = 0.01 randn, steps 1 - 3, rel(p) <= 1e-6, rel(m), rel(v) <= 1e-5"""
    n = 100003
    gen = torch.Generator().manual_seed(2)
    p0, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.01
    a, b = [p0.clone(), torch.zeros(n), torch.zeros(n)], [p0.clone(), torch.zeros(n), torch.zeros(n)]
    for t in (1, 2, 3):
        adamw_restated(a[0], g, a[1], a[2], t, 4.5e-6, 1e-4)
        adamw_restated(b[0], g, b[1], b[2], t, 4.5e-6, 1e-4, **fault)
    return rel(b[0], a[0]) <= 1e-6 and rel(b[1], a[1]) <= 1e-5 and rel(b[2], a[2]) <= 1e-5


def test_adamw():
    for lr, wd in ((1e-2, 0.1), (4.5e-6, 1e-4)):
        w = max(_adamw_run(n, lr, wd) for n in (5, 1023, 4101))
        print(f"honest AdamW lr={lr} wd={wd}, steps {STEPS}: max error / limit {w:.3f}")
        assert w <= 1.0
    for what, fault, must_pass_today in (("without weight decay", dict(no_wd=True), True), ("eps inside the square root", dict(eps_in_sqrt=True), True),
                                         ("bc2 of the previous step", dict(bc2_prev=True), False)):
        today = _adamw_today(**fault)
        assert today or not must_pass_today, f"AdamW {what} no longer passes today's assertion: it documents nothing"
        _raises(lambda: _adamw_run(4101, 1e-2, 0.1, **fault), f"AdamW {what} (lr 1e-2, wd 0.1)", today)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------------
def _wave_sum(lane: torch.Tensor) -> torch.Tensor:
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[..., idx ^ o]
    return lane[..., 0]


def _lanes(t: torch.Tensor) -> torch.Tensor:
    """[M, D] -> the per-lane partial of a row: chunks i = 0 .. NCH-1 of four elements at column 4 (lane + 64 i), added as (a + b) + (c + d), in order"""
    M, D = t.shape
    nch = (D + 255) // 256
    t = torch.cat([t, torch.zeros(M, nch * 256 - D)], 1).view(M, nch, 64, 4)
    s = torch.zeros(M, 64)
    for i in range(nch):
        s = s + ((t[:, i, :, 0] + t[:, i, :, 1]) + (t[:, i, :, 2] + t[:, i, :, 3]))
    return s


def ln_restated(x, w, b, dy, dres, old, dt, cus: int = 256, drop_wg=None, wrong_rstd_row=None):
    """ln_fwd_kernel and ln_bwd_kernel (+ ln_bwd_reduce_kernel) in f32 torch: lane / wave grouping of the row sums, rows dealt to (workgroup, wave),
    a wave's column partials in row order, wave 0 adding the others', the fixed-order second pass added INTO dw / db / dx_colsum."""
    M, D = x.shape
    mean = (_wave_sum(_lanes(x)) / D).unsqueeze(1)
    d = x - mean
    rstd = (1.0 / torch.sqrt(_wave_sum(_lanes(d * d)) / D + 1e-5)).unsqueeze(1)
    y32 = d * rstd * w + b
    rs = rstd.clone()
    if wrong_rstd_row is not None:
        rs[wrong_rstd_row] = rstd[wrong_rstd_row + 1]
    xh = d * rs
    g = dy * w
    c1, c2 = (_wave_sum(_lanes(g)) / D).unsqueeze(1), (_wave_sum(_lanes(g * xh)) / D).unsqueeze(1)
    dx = rs * (g - c1 - xh * c2) + dres
    grid = min((M + 3) // 4, cus)
    parts = torch.zeros(grid, 3, D)
    for wg in range(grid):
        waves = [[_seqsum(t[wg * 4 + wv::grid * 4]) for wv in range(4)] for t in (dy * xh, dy, dx)]
        parts[wg] = torch.stack([((wv[0] + wv[1]) + wv[2]) + wv[3] for wv in waves])
    if drop_wg is not None:
        parts[drop_wg, 0] = 0.0
    sums = [o + _rowsum16(parts[:, k]) for k, o in enumerate(old)]
    return dict(mean=mean.squeeze(1), rstd=rstd.squeeze(1), y32=y32, y16=y32.to(dt), dx=dx, dx16=dx.to(dt), dw=sums[0], db=sums[1], dx_colsum=sums[2])


def _ln_case(M, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy = h16r(torch.randn(M, D, generator=g), dt)
    dres = torch.randn(M, D, generator=g)
    old = [torch.randn(D, generator=g) for _ in range(3)]
    return x, w, b, dy, dres, old


def _ln_check(got, refs, what):
    worst = {k: check(got[k], *refs[k], f"{what} {k}") for k in refs}
    assert bits_equal(got["y16"], got["y32"].to(got["y16"].dtype)) and bits_equal(got["dx16"], got["dx"].to(got["dx16"].dtype))
    return worst


@pytest.mark.parametrize("M,D", [(37, 260), (1027, 768), (33, 2048)])
def test_layernorm(M, D):
    for dt in (BF16, F16):
        case = _ln_case(M, D, dt, M + D)
        refs = ln_ref(*case, dt=dt)
        worst = _ln_check(ln_restated(*case, dt), refs, f"layernorm {M}x{D} {dt}")
        print(f"honest layernorm {M}x{D} {dt}: max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0
    if M != 1027:
        return
    case = _ln_case(M, D, BF16, M + D)
    refs = ln_ref(*case, dt=BF16)
    bad = ln_restated(*case, BF16, drop_wg=100)
    today = rel(bad["dw"] - case[5][0], refs["dw"][0] - case[5][0].double()) <= F32_TOL
    _raises(lambda: _ln_check(bad, refs, "dw"), "layernorm dw missing one workgroup's partial", today)
    bad = ln_restated(*case, BF16, wrong_rstd_row=500)
    today = rel(bad["dx"], refs["dx"][0]) <= F32_TOL and rel(bad["dx16"].float(), refs["dx"][0]) <= BF16_TOL
    _raises(lambda: _ln_check(bad, refs, "dx"), "layernorm dx of one row computed with its neighbour's rstd", today)


# ---- enh_gemm_f32 -----------------------------------------------------------------------------------------------------------------------------------------
def gemm_f32_restated(A, B, bias, res, res_rows, ignore_res_rows=False):
    M, K = A.shape
    acc = torch.zeros(M, B.shape[0])
    for k in range(K):
        acc = acc + A[:, k:k + 1] * B[:, k].unsqueeze(0)
    rows = torch.arange(M) if ignore_res_rows else torch.arange(M) % res_rows
    return acc + bias + res[rows]


def test_gemm_f32_position_table():
    M, N, K = 70, 66, 19
    g = torch.Generator().manual_seed(9)
    A, B, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.3, torch.randn(N, generator=g)
    mem = torch.randn(M, N, generator=g)          # a 7-row table and what lies behind it
    ref, bound = gemm_f32_ref(A, B, bias, res=mem[:7], res_rows=7)
    w = check(gemm_f32_restated(A, B, bias, mem, 7), ref, bound, "gemm_f32 bias + position table")
    print(f"honest gemm_f32 {M}x{N}x{K} with a 7-row position table: max err / bound {w:.4f}")
    assert w <= 1.0
    # where today's callers pass res_rows = M (the in-place residual) the fault changes nothing
    ref_m, bound_m = gemm_f32_ref(A, B, bias, res=mem, res_rows=M)
    today = check(gemm_f32_restated(A, B, bias, mem, M, ignore_res_rows=True), ref_m, bound_m, "res_rows = M") <= 1.0
    _raises(lambda: check(gemm_f32_restated(A, B, bias, mem, 7, ignore_res_rows=True), ref, bound, "gemm_f32"),
            "gemm_f32 with res_rows ignored (row m instead of m % 7)", today)


def test_exact_references_are_what_torch_gives():
    """the data-movement references: to_patches / from_patches are each other's inverse and agree with unfold"""
    img = torch.arange(2 * 3 * 8 * 16, dtype=F32).view(2, 3, 8, 16)
    pat = to_patches(img, 4)
    assert torch.equal(from_patches(pat, 2, 3, 8, 16, 4), img)
    unf = torch.nn.functional.unfold(img, 4, stride=4).transpose(1, 2).reshape(-1, 3 * 16)
    assert torch.equal(pat, unf)
    assert check_limit(torch.ones(3), torch.ones(3), torch.ones(3, dtype=F64), "identity") == (0.0, 0.0)
