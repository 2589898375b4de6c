"""An inf or a NaN on its way through the stage-1 transformer's kernels: GEMM (every family, layout and fused mode, forward and weight-gradient
split-K, the fused bias gradient), LayerNorm, attention (aligned, ragged, every head width) and the step's helper kernels.

fp16 training is safe as long as an overflow anywhere in a loss-scaled step reaches the flat gradient as an inf or NaN (engine/optim.py LossScaler
drops the step).  Every case here runs clean once and then once per poison in {+inf, NaN}, in fp16 and bf16, and holds the kernel to
tests/nonfinite_util.py:

  assert_no_swallow  inside the unit that shares data with the poisoned element (a GEMM row or column, a LayerNorm row, an (image, head) of attention,
                     a column of a column sum) the output is non-finite wherever the float64 evaluation of the formula on the poisoned inputs is;
  assert_isolated    everything outside that unit equals the clean run bit for bit;
  check_overflow     fp16 results past 65520 are +-inf exactly where the correctly rounded reference is (no 65504, no NaN), the finite rest inside the
                     bound the per-element tests use; the bf16 twin of the same case is entirely finite and inside its bound.

Poisoned operands are redrawn so that no exact zero multiplies the poison.  The counts of SPURIOUS non-finite elements (kernel non-finite, reference
finite, inside the affected unit) are printed per case; they are not faults ("what a non-finite input does to each kernel").

GEMM shapes: the smallest that reach each kernel, asserted through enh_gemm_h16_variant_mode as tests/test_elementwise_gpu.py does —
(1000, 200, 328) gemm_kernel, (384, 128, 192) gemm_pipe2_kernel under family 3, (512, 256, 384) gemm_w256 / w256p / w256r under families 7 / 8 / 9."""
import os

import pytest
import torch

import attn_dh_util as DH
from nonfinite_util import (assert_all_finite_within, assert_isolated, assert_no_swallow, check_overflow, element_bound, nonfinite, pow2_scale,
                            scrub_shared_buffers)  # noqa: F401  (scrub_shared_buffers: an autouse fixture)
from step_helpers_util import bits_equal, colsum_ref, from_patches, int_matrix, ln_ref, pixel_loss_ref, to_patches
from test_elementwise_gpu import ATT_MARGIN, GEMM_MODES, LOG2E, C, _expected_kernel, _gemm_case, _gemm_modes, _mm64  # noqa: F401  (C: the fixture)
from util import SUB16, U16, assert_elementwise, elem_bound, h16r, row_err

pytestmark = pytest.mark.gpu

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
INF, NAN = float("inf"), float("nan")
POISONS = (("inf", INF), ("nan", NAN))
I0, N0 = 129, 70                  # the poisoned GEMM row / column: the second row of a 128-row tile, off every 64-column boundary


def _nz(x, fill=2.0 ** -6):
    """no exact zero (a zero times the poison is a NaN of the test's own making)"""
    return torch.where(x == 0, torch.full_like(x, fill), x)


def _mask(shape, *index):
    m = torch.zeros(shape, dtype=torch.bool)
    m[index] = True
    return m


def _same_bits(a, b) -> bool:
    """bits_equal, except that a NaN answers a NaN whatever its payload (the kernels' conversions and torch's give different quiet NaNs)"""
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(na, nb) and bits_equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


# =====================================================================================================================================================
# 2a. GEMM
# =====================================================================================================================================================
GEMM_CONFIGS = ([(fam, shape, ta, True) for fam, shape in ((0, (1000, 200, 328)), (3, (384, 128, 192)), (7, (512, 256, 384))) for ta in (False, True)]
                + [(fam, (512, 256, 384), False, tb) for fam in (8, 9) for tb in (False, True)])
_CASES = {}


def _case(M, N, K, dt):
    """test_elementwise_gpu._gemm_case with the operands that meet a poison made nonzero (B[:, K-1], A[:, 0]; h kept off +-1, where tanh' is 0)"""
    key = (M, N, K, dt)
    if key not in _CASES:
        c = dict(_gemm_case(M, N, K, dt))
        c["A"], c["B"] = c["A"].clone(), c["B"].clone()
        c["A"][:, 0], c["B"][:, K - 1] = _nz(c["A"][:, 0]), _nz(c["B"][:, K - 1])
        c["h"] = torch.where(c["h"].abs() >= 1, c["h"].sign() * 0.5, c["h"])
        c["base"], c["mag"], c["dev"] = _mm64(c["A"], c["B"].t()), _mm64(c["A"].abs(), c["B"].abs().t()), {}
        _CASES[key] = c
    return _CASES[key]


def _poisoned(c, **changed):
    """a copy of the case with some operands replaced; the fp64 product re-evaluated on them (IEEE arithmetic does the propagating)"""
    p = dict(c)
    p.update(changed)
    p["dev"] = {}
    if "A" in changed or "B" in changed:
        p["base"] = p["A"].double() @ p["B"].double().t()
    return p


def _run_modes(C, c, M, N, K, dt, ta, tb):
    return {name: (out.cpu(), ref, bound) for name, out, ref, bound in _gemm_modes(C, c, M, N, K, dt, ta, tb)}


def _forced(C, fam, ta, tb, M, N, K):
    L = C.lib()
    assert L.enh_gemm_set_kernel(fam) == 0 and L.enh_gemm_set_scheduler(1) == 0
    if not os.environ.get("ENH_GEMM_KERNEL"):
        for name, mode in GEMM_MODES:
            want = _expected_kernel(fam, ta, M, N, K, mode)
            assert L.enh_gemm_h16_variant_mode(int(ta), int(tb), M, N, K, mode).decode() == want, (name, want)


def _release(C):
    C.lib().enh_gemm_set_kernel(-1)
    C.lib().enh_gemm_set_scheduler(1)


@DTS
@pytest.mark.parametrize("fam,shape,ta,tb", GEMM_CONFIGS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gemm_poisoned_operand(C, fam, shape, ta, tb, dt):
    """A[i0, K-1] (the last K stage), B[n0, 0] (the first), and one element of aux / res: every fused mode"""
    M, N, K = shape
    c = _case(M, N, K, dt)
    what = f"gemm family {fam} {M}x{N}x{K} ta={int(ta)} tb={int(tb)} {dt}"
    row, col, elem = _mask((M, 1), I0), _mask((1, N), 0, N0), _mask((M, N), I0 + 1, N0 + 1)
    try:
        _forced(C, fam, ta, tb, M, N, K)
        clean = _run_modes(C, c, M, N, K, dt, ta, tb)
        for name, (out, ref, bound) in clean.items():
            assert_elementwise(out, ref, bound, f"{what} {name} clean")
        for pname, pv in POISONS:
            Ap, Bp, hp, rp = c["A"].clone(), c["B"].clone(), c["h"].clone(), c["res"].clone()
            Ap[I0, K - 1], Bp[N0, 0], hp[I0 + 1, N0 + 1], rp[I0 + 1, N0 + 1] = pv, pv, pv, pv
            report = []
            for where, pc, unit in (("A", _poisoned(c, A=Ap), row), ("B", _poisoned(c, B=Bp), col)):
                for name, (out, ref, _) in _run_modes(C, pc, M, N, K, dt, ta, tb).items():
                    tag = f"{what} {pname} in {where}: {name}"
                    sel = unit.expand(M, N)
                    assert bool(nonfinite(pc["base"][sel]).all()), tag + ": the reference product is finite"
                    if name == "bias_tanh" and pv == INF:
                        # tanh(+-inf) = +-1 is finite: the one place where the kernel may answer either way — exactly +-1 or non-finite
                        g, r = out[sel].float(), ref[sel].float()
                        ok = nonfinite(g) | (g == r)
                        assert bool(ok.all()), f"{tag}: {int((~ok).sum())} elements neither +-1 nor non-finite, e.g. {g[~ok][0].item()!r}"
                        report.append(f"{where} bias_tanh: {int((g == r).sum())} x +-1, {int(nonfinite(g).sum())} non-finite")
                    else:
                        spurious = assert_no_swallow(out[sel], ref[sel], tag, dt if out.dtype == dt else None)
                        assert spurious == 0, (tag, spurious)      # (every reference element of the unit is non-finite: nothing can be spurious)
                    assert_isolated(out, clean[name][0], unit, tag)
            pc = _poisoned(c, h=hp, res=rp)
            for name, (out, ref, _) in _run_modes(C, pc, M, N, K, dt, ta, tb).items():
                tag = f"{what} {pname} in aux / res: {name}"
                if name in ("dtanh", "bias_res", "accumulate"):
                    assert_no_swallow(out[elem], ref[elem], tag, dt if out.dtype == dt else None)
                    assert_isolated(out, clean[name][0], elem, tag)
                else:
                    assert bits_equal(out, clean[name][0]), tag + ": a mode that does not read aux / res changed"
            print(f"{what} {pname}: no swallow, no leak; " + "; ".join(report))
    finally:
        _release(C)


def _overflow_operands(c, dt):
    """A scaled by the power of two that takes the rms of the product to ~4e4; what A cannot carry inside fp16's range goes to B (a power of two on
    either operand is the same exact scaling of every product)"""
    s = pow2_scale(c["base"])
    sa = min(s, 2.0 ** int(torch.floor(torch.log2(60000.0 / c["A"].abs().max())).item()))
    A, B = c["A"] * sa, c["B"] * (s / sa)
    assert A.abs().max() < 65504 and B.abs().max() < 65504 and bool((h16r(A, dt) == A).all()) and bool((h16r(B, dt) == B).all())
    return A, B, c["base"] * s, c["mag"] * s


def _overflow_check(got, ref, mag, k, dt, what):
    if dt == F16:
        check_overflow(got, ref, element_bound(elem_bound(ref, mag, k, F16)), what, exact=True)
    else:
        w = assert_all_finite_within(got, ref, elem_bound(ref, mag, k, BF16), what)
        print(f"overflow twin {what}: finite, {w:.3f} of the element bound")


@DTS
@pytest.mark.parametrize("fam,shape,ta,tb", GEMM_CONFIGS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gemm_fp16_overflow_is_exact(C, fam, shape, ta, tb, dt):
    """the 16-bit pack of the plain and the tanh' epilogue: +-inf exactly where fp16(ref) is; the same case in bf16 entirely finite"""
    M, N, K = shape
    c = _case(M, N, K, dt)
    A, B, base, mag = _overflow_operands(c, dt)
    d = 1 - c["h"].double() ** 2
    a = (A.t().contiguous() if ta else A).to(dt).cuda()
    b = (B.t().contiguous() if tb else B).to(dt).cuda()
    what = f"gemm family {fam} {M}x{N}x{K} ta={int(ta)} tb={int(tb)} {dt}"
    try:
        _forced(C, fam, ta, tb, M, N, K)
        o = torch.full((M, N), 5.0, dtype=dt, device="cuda")
        C.gemm(a, b, M, N, K, out_bf16=o, trans_a=ta, trans_b=tb)
        o2 = torch.full((M, N), 5.0, dtype=dt, device="cuda")
        C.gemm(a, b, M, N, K, act=C.ACT_DTANH, aux=c["h"].to(dt).cuda(), out_bf16=o2, trans_a=ta, trans_b=tb)
    finally:
        _release(C)
    _overflow_check(o, base, mag, K, dt, what + " h16")
    _overflow_check(o2, base * d, mag * d.abs(), K, dt, what + " dtanh")


def _split_k_shape(C):
    """the smallest shape the planner splits along K in the forward layout (the existing per-element test's 1024 x 768 x 2304 as the last resort)"""
    for s in ((256, 128, 2304), (512, 256, 2304), (1024, 768, 2304)):
        if C.lib().enh_gemm_h16_workspace_bytes(0, 1, *s) > 0:
            return s
    raise AssertionError("no forward shape is split along K")


@DTS
def test_forward_split_k_poison_in_the_last_slab(C, dt):
    M, N, K = _split_k_shape(C)
    c = _case(M, N, K, dt)
    b, bias = c["B"].t().contiguous().to(dt).cuda(), c["bias"].cuda()
    row = _mask((M, 1), I0)

    def run(A):
        a = A.to(dt).cuda()
        o16 = torch.empty(M, N, dtype=dt, device="cuda"); C.gemm(a, b, M, N, K, trans_b=True, out_bf16=o16)
        x = c["res"].clone().cuda(); C.gemm(a, b, M, N, K, trans_b=True, bias=bias, res=x, res_rows=M, out_f32=x)
        return o16.cpu(), x.cpu()
    clean = run(c["A"])
    assert_elementwise(clean[0], c["base"], elem_bound(c["base"], c["mag"], K, dt), f"forward split-K {M}x{N}x{K} {dt} h16 clean")
    for pname, pv in POISONS:
        Ap = c["A"].clone()
        Ap[I0, K - 1] = pv
        ref = Ap[I0].double() @ c["B"].double().t()
        for name, out, cl, r in zip(("h16", "bias_res"), run(Ap), clean, (ref, ref + c["bias"].double() + c["res"][I0].double())):
            tag = f"forward split-K {M}x{N}x{K} {dt} {pname} in the last slab: {name}"
            assert assert_no_swallow(out[I0], r, tag, dt if name == "h16" else None) == 0
            assert_isolated(out, cl, row, tag)
    # the 16-bit pack of the second pass at fp16's range edge
    A, B, base, mag = _overflow_operands(c, dt)
    o16 = torch.empty(M, N, dtype=dt, device="cuda")
    C.gemm(A.to(dt).cuda(), B.t().contiguous().to(dt).cuda(), M, N, K, trans_b=True, out_bf16=o16)
    _overflow_check(o16, base, mag, K, dt, f"forward split-K {M}x{N}x{K} {dt} h16")


@DTS
@pytest.mark.parametrize("form,data", [("two_pass", "gaussian"), ("two_pass", "integers"), ("atomic", "integers")])
def test_wgrad_split_k_one_inf_in_the_upstream_gradient(C, form, data, dt):
    """dW += dY^T X over 8192 tokens: one inf at dY[t0, n0] makes row n0 of dW non-finite — enh_nonfinite_flag reads 1 — and touches no other row.
    The atomic form adds its slabs in whatever order they finish: on Gaussian data two CLEAN launches already differ in the last bit (26107 of 49152
    elements on MI355X), so a poisoned launch cannot be compared with a clean one there.  On integers in [-4, 4] every f32 partial sum is an integer
    below 2^24 (16 x 8192 = 2^17), exact in any order (step_helpers_util.int_matrix): both forms are then deterministic and held to bit-identity."""
    L = C.lib()
    tokens, n_out, k_in, t0 = 8192, 256, 192, 8191
    g = torch.Generator().manual_seed(9)
    if data == "integers":
        dY, X = int_matrix(tokens, n_out, 1), _nz(int_matrix(tokens, k_in, 2), 1.0)
        old = torch.randint(-50, 51, (n_out, k_in), generator=g).float()
    else:
        dY, X = h16r(torch.randn(tokens, n_out, generator=g) * 0.1, dt), _nz(h16r(torch.randn(tokens, k_in, generator=g), dt))
        old = torch.randn(n_out, k_in, generator=g)
    assert L.enh_gemm_h16_workspace_bytes(1, 1, n_out, k_in, tokens) > 0          # the shape IS split
    b = X.to(dt).cuda()

    def run(dy):
        a, dW = dy.to(dt).cuda(), old.clone().cuda()
        if form == "two_pass":
            C.gemm(a, b, n_out, k_in, tokens, trans_a=True, trans_b=True, accumulate=True, out_f32=dW)
        else:
            C._check(L.enh_gemm_h16(C._p(a), n_out, 1, C._p(b), k_in, 1, n_out, k_in, tokens, None, C.ACT_NONE, None, 0, None, 0, 0, 1, C._p(dW), None, k_in,
                                    C.DT_BF16 if dt == BF16 else C.DT_F16, C._stream()), "enh_gemm_h16")
        flag = torch.zeros(1, device="cuda")
        C.nonfinite_flag(dW.reshape(-1), flag)
        return dW.cpu(), flag.item()
    clean, flag = run(dY)
    assert flag == 0.0 and bool(torch.isfinite(clean).all())
    if data == "integers":
        assert bits_equal(clean, (dY.double().t() @ X.double() + old.double()).float()), "the integer sums are not exact"
    for pname, pv in POISONS:
        dYp = dY.clone()
        dYp[t0, N0] = pv
        got, flag = run(dYp)
        tag = f"weight-gradient split-K {form} {data} {dt} {pname}"
        ref = dYp[:, N0].double() @ X.double() + old[N0].double()
        assert assert_no_swallow(got[N0], ref, tag) == 0
        assert_isolated(got, clean, _mask((n_out, 1), N0), tag)
        assert flag == 1.0, tag + ": enh_nonfinite_flag did not see it"


@DTS
@pytest.mark.parametrize("M,N,K,fam", [(512, 256, 192, -1), (512, 256, 192, 9), (1000, 192, 256, -1)])
def test_dtanh_colsum_poisoned_column(C, M, N, K, fam, dt):
    """B[n0, 0] poisoned: column n0 of the output and of the fused bias gradient are non-finite, every other column keeps its bits"""
    L = C.lib()
    c = _case(M, N, K, dt)
    a, h, old = c["A"].to(dt).cuda(), c["h"].to(dt).cuda(), c["bias"].cuda()
    d = 1 - c["h"].double() ** 2
    col = _mask((1, N), 0, N0)

    def run(B, accumulate):
        out, cs = torch.empty(M, N, dtype=dt, device="cuda"), old.clone()
        C.gemm_dtanh_colsum(a, B.t().contiguous().to(dt).cuda(), M, N, K, h, out, cs, trans_b=True, accumulate_colsum=accumulate)
        return out.cpu(), cs.cpu()
    try:
        assert L.enh_gemm_set_kernel(fam) == 0
        if fam == 9 and not os.environ.get("ENH_GEMM_KERNEL"):
            assert L.enh_gemm_h16_variant_mode(0, 1, M, N, K, 3).decode() == "gemm_w256p_kernel"
        for accumulate in (False, True):
            clean = run(c["B"], accumulate)
            assert_elementwise(clean[0], c["base"] * d, elem_bound(c["base"] * d, c["mag"] * d.abs(), K, dt), f"dtanh_colsum {M}x{N}x{K} family {fam} {dt} clean")
            for pname, pv in POISONS:
                Bp = c["B"].clone()
                Bp[N0, 0] = pv
                out, cs = run(Bp, accumulate)
                tag = f"dtanh_colsum {M}x{N}x{K} family {fam} {dt} accumulate={accumulate} {pname}"
                ref = (c["A"].double() @ Bp[N0].double()) * d[:, N0]
                assert assert_no_swallow(out[:, N0], ref, tag + " output", dt) == 0
                assert assert_no_swallow(cs[N0:N0 + 1], ref.sum(0, keepdim=True), tag + " column sum") == 0
                assert_isolated(out, clean[0], col, tag + " output")
                assert_isolated(cs, clean[1], col[0], tag + " column sums")
    finally:
        L.enh_gemm_set_kernel(-1)


# =====================================================================================================================================================
# 2b. LayerNorm
# =====================================================================================================================================================
LN_SHAPES = [(5, 256), (130, 768), (3, 1280)]


def _ln_inputs(M, D, dt, x_std=2.0):
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * x_std + 0.5
    w = _nz(1 + 0.1 * torch.randn(D, generator=g))
    b = 0.1 * torch.randn(D, generator=g)
    dy = _nz(h16r(torch.randn(M, D, generator=g), dt))
    dres = torch.randn(M, D, generator=g)
    return x, w, b, dy, dres


def _ln_forward(C, x, w, b, dt):
    M, D = x.shape
    y16, y32 = torch.full((M, D), NAN, dtype=dt, device="cuda"), torch.full((M, D), NAN, device="cuda")
    mean, rstd = torch.full((M,), NAN, device="cuda"), torch.full((M,), NAN, device="cuda")
    C.ln_fwd(x.cuda(), w.cuda(), b.cuda(), y16, mean, rstd, y_extra_f32=y32)
    return dict(y16=y16, y32=y32, mean=mean, rstd=rstd)


def _ln_backward(C, dy, x, w, mean, rstd, dres, dt):
    M, D = x.shape
    dx, dx16 = torch.full((M, D), NAN, device="cuda"), torch.full((M, D), NAN, dtype=dt, device="cuda")
    dw, db, dxs = (torch.zeros(D, device="cuda") for _ in range(3))
    C.ln_bwd(dy.to(dt).cuda(), x.cuda(), w.cuda(), mean, rstd, None if dres is None else dres.cuda(), dx, dx16, dw, db, dx_colsum=dxs)
    return dict(dx=dx.cpu(), dx16=dx16.cpu(), dw=dw.cpu(), db=db.cpu(), dx_colsum=dxs.cpu())


@DTS
@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_poisoned_row(C, M, D, dt):
    x, w, b, dy, dres = _ln_inputs(M, D, dt)
    r0, c0 = M - 2, D - 3
    row, colm = _mask((M, 1), r0), _mask((D,), c0)
    ref = ln_ref(x, w, b, dy, dres, dt=dt)
    fwd = _ln_forward(C, x, w, b, dt)
    bwd = _ln_backward(C, dy, x, w, fwd["mean"], fwd["rstd"], dres, dt)
    for name, got in list(fwd.items()) + list(bwd.items()):
        assert_elementwise(got, ref[name][0], ref[name][1], f"layernorm {M}x{D} {dt} clean {name}")
    for pname, pv in POISONS:
        what = f"layernorm {M}x{D} {dt} {pname}"
        xp = x.clone()
        xp[r0, c0] = pv
        rp = ln_ref(xp, w, b, dt=dt)
        got = _ln_forward(C, xp, w, b, dt)
        for name in ("y16", "y32"):
            assert bool(nonfinite(rp[name][0][r0]).all())
            assert_no_swallow(got[name][r0], rp[name][0][r0], f"{what} in x: {name}")
            assert_isolated(got[name], fwd[name], row, f"{what} in x: {name}")
        for name in ("mean", "rstd"):
            assert_no_swallow(got[name][r0:r0 + 1], rp[name][0][r0:r0 + 1], f"{what} in x: {name}")
            assert_isolated(got[name], fwd[name], row[:, 0], f"{what} in x: {name}")
        dyp = dy.clone()
        dyp[r0, c0] = pv
        rb = ln_ref(x, w, b, dyp, dres, dt=dt)
        gb = _ln_backward(C, dyp, x, w, fwd["mean"], fwd["rstd"], dres, dt)
        for name in ("dx", "dx16"):
            assert bool(nonfinite(rb[name][0][r0]).all())
            assert_no_swallow(gb[name][r0], rb[name][0][r0], f"{what} in dy: {name}")
            assert_isolated(gb[name], bwd[name], row, f"{what} in dy: {name}")
        for name in ("dw", "db"):
            assert bool(nonfinite(rb[name][0][c0])) and bool(nonfinite(gb[name][c0])), f"{what} in dy: {name}[c0] is finite"
            assert_isolated(gb[name], bwd[name], colm, f"{what} in dy: {name}")
        assert bool(nonfinite(rb["dx_colsum"][0]).all())
        assert assert_no_swallow(gb["dx_colsum"], rb["dx_colsum"][0], f"{what} in dy: dx_colsum") == 0


@DTS
@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_fp16_overflow_is_exact(C, M, D, dt):
    """y with a large w, and the 16-bit dx with dy scaled up (x drawn narrow, rstd ~ 4, so that dy itself stays inside fp16's range).
    y16's bound: the 16-bit output is the rounded y32 (tests/test_step_helpers_gpu.py holds that bit for bit), so it gets y32's bound of
    step_helpers_util.ln_ref plus one rounding, u |y| + sub.  (ln_ref's own y16 entry, u |y| + 8 * 2^-24 (|w| |x^| + |b|), leaves out the error x^
    inherits from the f32 mean and rstd; under w ~ 1 that error, ~1e-7, hides below the other terms, under w ~ 2^15 it is 3e-3 where |x^| is small.)"""
    x, w, b, dy, _ = _ln_inputs(M, D, dt, x_std=0.25)
    w = w * pow2_scale(ln_ref(x, w, b, dt=dt)["y32"][0])
    ref = ln_ref(x, w, b, dt=dt)
    fwd = _ln_forward(C, x, w, b, dt)
    what = f"layernorm {M}x{D} {dt}"
    y_bound = ref["y32"][1] + U16[dt] * ref["y32"][0].abs() + SUB16.get(dt, 0.0)
    if dt == F16:
        check_overflow(fwd["y16"], ref["y16"][0], element_bound(y_bound), what + " y16", exact=True)
    else:
        assert_all_finite_within(fwd["y16"], ref["y16"][0], y_bound, what + " y16")
    x, w, b, dy, _ = _ln_inputs(M, D, dt, x_std=0.25)
    fwd = _ln_forward(C, x, w, b, dt)
    dy = dy * pow2_scale(ln_ref(x, w, b, dy, dt=dt)["dx"][0])
    assert dy.abs().max() < 65504
    ref = ln_ref(x, w, b, dy, dt=dt)
    bwd = _ln_backward(C, dy, x, w, fwd["mean"], fwd["rstd"], None, dt)
    if dt == F16:
        check_overflow(bwd["dx16"], ref["dx16"][0], element_bound(ref["dx16"][1]), what + " dx16", exact=True)
    else:
        assert_all_finite_within(bwd["dx16"], *ref["dx16"], what + " dx16")


# =====================================================================================================================================================
# 2c. attention
# =====================================================================================================================================================
ATT_CASES = ([(64, fam, shape) for fam in ((0, 0, 0), (1, 1, 1)) for shape in ((2, 64, 2), (2, 128, 2), (2, 72, 2), (2, 129, 2))]
             + [(D, (0, 0, 0), (2, 72, 2)) for D in (32, 96, 128)])


def _att_inputs(B, N, H, D, pre, dt, scale, seed=0):
    """(device-side packed qkv, dO) as f32 CPU tensors holding values of dt, no exact zeros"""
    g = torch.Generator().manual_seed(B * 100 + N + H + D + seed)
    qkv = _nz(h16r(torch.randn(B, N, 3 * H * D, generator=g) * 1.5, dt))
    do = _nz(h16r(torch.randn(B, N, H * D, generator=g), dt))
    if pre:       # the q third holds dt(q * scale * log2e)
        qkv[..., :H * D] = _nz(h16r(qkv[..., :H * D] * (scale * LOG2E), dt))
    return qkv, do


def _att_ref(qkv, do, B, N, H, D, pre, scale):
    """fp64 on the UNSCALED values the bits represent: out, lse, (dq, dk, dv)"""
    qref = qkv.double().clone()
    if pre:
        qref[..., :H * D] /= (scale * LOG2E)
    out, lse, _, grads = DH.attn_ref64(qref, do, B, N, H, D, scale)
    return out, lse, grads


def _att_run(C, fam, qkv, do, B, N, H, D, pre, dt, scale):
    qd, dod = qkv.to(dt).cuda(), do.to(dt).cuda()
    out = torch.full((B, N, H * D), NAN, dtype=dt, device="cuda")
    lse = torch.full((B, H, N), NAN, device="cuda")
    dqkv = torch.full((B, N, 3 * H * D), NAN, dtype=dt, device="cuda")
    delta = torch.empty(B, H, N, device="cuda")
    try:
        C.attention_set_kernel(*fam)
        C.attention_forward(qd, B, N, H, scale, out, lse, q_prescaled=pre, dim_head=D)
        C.attention_backward(qd, out, dod, lse, B, N, H, scale, dqkv, delta, q_prescaled=pre, dim_head=D)
        torch.cuda.synchronize()
    finally:
        C.attention_set_kernel(0, 0, 0)
    return out.cpu(), lse.cpu(), dqkv.cpu()


@DTS
@pytest.mark.parametrize("pre", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("D,fam,shape", ATT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_attention_poisoned_element(C, D, fam, shape, pre, dt):
    """one element of q, k, v or dO of (image 1, head 0) at row 0 (what a wrong clamp of image 0's tail reads) and at row N - 1 (what every clamped row
    of image 1 reads): non-finite inside that (image, head) wherever fp64 says so, every other (image, head) bit-identical"""
    B, N, H = shape
    scale = D ** -0.5
    qkv, do = _att_inputs(B, N, H, D, pre, dt, scale)
    clean = _att_run(C, fam, qkv, do, B, N, H, D, pre, dt, scale)
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean)
    unit = _mask((B, N, H * D), 1, slice(None), slice(0, D))
    unit3 = _mask((B, N, 3, H * D), 1, slice(None), slice(None), slice(0, D)).view(B, N, 3 * H * D)
    unit_lse = _mask((B, H, N), 1, 0)
    what = f"attention D={D} family {fam} B={B} N={N} H={H} {'prescaled' if pre else 'plain'} {dt}"
    col = 5
    for pname, pv in POISONS:
        spurious = {}
        for r in (0, N - 1):
            for which, off in (("q", 0), ("k", H * D), ("v", 2 * H * D), ("dO", None)):
                qp, dp = qkv.clone(), do.clone()
                if off is None:
                    dp[1, r, col] = pv
                else:
                    qp[1, r, off + col] = pv
                out, lse, dqkv = _att_run(C, fam, qp, dp, B, N, H, D, pre, dt, scale)
                r_out, r_lse, r_grads = _att_ref(qp, dp, B, N, H, D, pre, scale)
                tag = f"{what} {pname} in {which} row {r}"
                n = 0
                if which != "dO":
                    n += assert_no_swallow(out[1, :, :D], r_out[1, :, :D], tag + " out")
                    n += assert_no_swallow(lse[1, 0], r_lse[1, 0], tag + " lse")
                    if which == "q":       # a poisoned query row is that row's business alone
                        assert_isolated(out, clean[0], _mask((B, N, H * D), 1, r, slice(0, D)), tag + " out")
                        assert_isolated(lse, clean[1], _mask((B, H, N), 1, 0, r), tag + " lse")
                assert_isolated(out, clean[0], unit, tag + " out")
                assert_isolated(lse, clean[1], unit_lse, tag + " lse")
                for name, got, ref in zip(("dq", "dk", "dv"), dqkv.view(B, N, 3, H * D).unbind(2), r_grads):
                    assert bool(nonfinite(ref[1, :, :D]).any()) or name == "dv", tag + f": the reference {name} is finite"
                    n += assert_no_swallow(got[1, :, :D], ref[1, :, :D], f"{tag} {name}")
                assert_isolated(dqkv, clean[2], unit3, tag + " dqkv")
                spurious[f"{which}{r}"] = n
        print(f"{what} {pname}: spurious non-finite elements inside the unit " + " ".join(f"{k}:{v}" for k, v in spurious.items()))


def _rows_bound(model, H, D, margin):
    """bound_fn for check_overflow(exact=False) on a gradient [B, N, H D]: over the D-wide rows that are finite throughout (kernel, model and
    fp16(ref)), the worst row_err of the kernel <= margin x the worst row_err of the rounding model — the limit of the per-row tests"""
    def fn(got, ref, what, fin):
        worst_k = worst_m = 0.0
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            keep = (fin[..., sl].all(-1) & torch.isfinite(model[..., sl]).all(-1)).reshape(-1)
            assert bool(keep.any()), f"{what}: no finite row in head {h}"
            r = ref[..., sl].reshape(-1, D)
            # row_err normalises by the rms row norm of the tensor handed in: hand in the kept rows of the reference for both
            ek, em = row_err(got[..., sl].reshape(-1, D)[keep], r[keep], D), row_err(model[..., sl].reshape(-1, D)[keep], r[keep], D)
            worst_k, worst_m = max(worst_k, ek.max().item()), max(worst_m, em.max().item())
        assert worst_m > 0
        return worst_k / worst_m, margin, "x the model's worst row"
    fn.wants_mask = True
    return fn


@pytest.mark.parametrize("fam", [(0, 0, 0), (1, 1, 1)], ids=lambda f: "fam%d%d%d" % f)
@pytest.mark.parametrize("B,N,H", [(2, 128, 2), (2, 72, 2)])
def test_attention_backward_fp16_overflow(C, fam, B, N, H):
    """dO scaled so that part of dV = P^T dO passes 65520.  dS is packed to 16 bits inside the kernels, so dQ / dK may turn non-finite where fp64 is
    finite (counted); what fp16(ref) makes +-inf is non-finite, what stays finite is within ATT_MARGIN x the rounding model's worst row.  dO's rows
    share one direction (each a multiple of one vector, plus 10 % noise): P^T dO then grows with the column sums of P and passes the range although
    dO itself stays inside it.  The bf16 run of the same case is finite throughout and inside the same limit."""
    D, scale = 64, 0.125
    for dt in (F16, BF16):
        g = torch.Generator().manual_seed(N)
        qkv = h16r(torch.randn(B, N, 3 * H * D, generator=g) * 2.0, dt)          # (scores of std 4: column sums of P well above 1)
        shared = torch.randn(1, 1, H * D, generator=g)
        do = h16r(shared * (1 + 0.1 * torch.randn(B, N, H * D, generator=g)), dt)
        do = do * 2.0 ** int(torch.floor(torch.log2(65504.0 / do.abs().max())).item())
        out, lse, dqkv = _att_run(C, fam, qkv, do, B, N, H, D, False, dt, scale)
        _, _, _, grads = DH.attn_ref64(qkv, do, B, N, H, D, scale)
        model = DH.attn_model(qkv, do, B, N, H, D, scale, dt, out=out, lse=lse)[2:]
        what = f"attention backward family {fam} B={B} N={N} H={H} {dt}"
        for name, got, ref, m in zip(("dq", "dk", "dv"), dqkv.float().view(B, N, 3, H * D).unbind(2), grads, model):
            if dt == BF16:
                w = DH.assert_rows_within(got, ref, H, D, ATT_MARGIN * DH.worst_rows(m, ref, H, D), f"{what} {name}")
                print(f"overflow twin {what} {name}: finite, worst row {w:.2e}")
            else:       # (on the CPU: 1.2 - 2.4 % of the reference dq, dk and dv of these cases pass 65520)
                check_overflow(got.contiguous(), ref, _rows_bound(m, H, D, ATT_MARGIN), f"{what} {name}", exact=False)


# =====================================================================================================================================================
# 2d. the rest of the step
# =====================================================================================================================================================
@DTS
def test_pixel_loss_and_patchify_poisoned_pixel(C, dt):
    B, Cc, H, W, p = 2, 3, 16, 32, 8
    g = torch.Generator().manual_seed(3)
    M, K = B * (H // p) * (W // p), Cc * p * p
    target, pix = torch.rand(B, Cc, H, W, generator=g), torch.randn(M, K, generator=g)
    scale = torch.tensor([1024.0], device="cuda")

    def run(px, tg):
        xrec, sums = torch.full((B, Cc, H, W), NAN, device="cuda"), torch.zeros(2, dtype=F64, device="cuda")
        dpix = torch.full((M, K), NAN, dtype=dt, device="cuda")
        C.unpatchify_loss(px.cuda(), tg.cuda(), B, Cc, H, W, p, 0.3, 1.0, xrec, sums, dpix, grad_scale=scale)
        pat = torch.full((M, K), NAN, dtype=dt, device="cuda")
        C.patchify(tg.cuda(), p, pat)
        return xrec.cpu(), sums.cpu(), dpix.cpu(), pat.cpu()
    clean = run(pix, target)
    s_ref, g_ref, s_bound, g_bound = pixel_loss_ref(pix, target, p, 0.3, 1.0, 1024.0, dt)
    assert_elementwise(clean[1], s_ref, s_bound, "pixel loss clean sums")
    assert_elementwise(clean[2], g_ref, g_bound, "pixel loss clean dpix")
    m0, k0 = 5, 77
    for pname, pv in POISONS:
        for which in ("pix", "target"):
            px, tg = pix.clone(), target.clone()
            if which == "pix":
                px[m0, k0] = pv
            else:       # the same element, addressed in image layout
                tp = to_patches(tg, p).clone()
                tp[m0, k0] = pv
                tg = from_patches(tp, B, Cc, H, W, p).contiguous()
            xrec, sums, dpix, pat = run(px, tg)
            sr, gr, _, _ = pixel_loss_ref(px, tg, p, 0.3, 1.0, 1024.0, dt)
            tag = f"unpatchify_loss {dt} {pname} in {which}"
            assert bool(nonfinite(sr).all())
            assert assert_no_swallow(sums, sr, tag + " sums") == 0
            assert_no_swallow(dpix, gr, tag + " dpix")
            assert bool(nonfinite(dpix[m0, k0])), tag
            assert_isolated(dpix, clean[2], _mask((M, K), m0, k0), tag + " dpix")
            assert _same_bits(xrec, from_patches(px, B, Cc, H, W, p).contiguous()), tag + ": xrec"
            assert _same_bits(pat, to_patches(tg, p).to(dt)), tag + ": patchify is not the permutation and one rounding"


@DTS
@pytest.mark.parametrize("M,N", [(513, 136), (8701, 520)])
def test_column_sums_poisoned_column(C, M, N, dt):
    g = torch.Generator().manual_seed(M + N)
    x = h16r(torch.randn(M, N, generator=g), dt)
    old = torch.randn(N, generator=g)

    def run(xx, acc):
        out = old.clone().cuda() if acc else torch.full((N,), NAN, device="cuda")
        C.colsum(xx.to(dt).cuda(), M, N, out, accumulate=acc)
        return out.cpu()
    for acc in (False, True):
        clean = run(x, acc)
        assert_elementwise(clean, *colsum_ref(x, old if acc else None), f"colsum {M}x{N} {dt} clean")
        for pname, pv in POISONS:
            for m0 in (0, M - 1):
                xp = x.clone()
                xp[m0, N0] = pv
                got = run(xp, acc)
                tag = f"colsum {M}x{N} {dt} accumulate={acc} {pname} at row {m0}"
                assert assert_no_swallow(got, colsum_ref(xp, old if acc else None)[0], tag) == 0
                assert_isolated(got, clean, _mask((N,), N0), tag)


@DTS
def test_casts_keep_inf_nan_and_overflow_to_inf(C, dt):
    """enh_cast_f32_h16 and the head-scaled casts: torch's round-to-nearest-even cast bit for bit on +-inf, NaN, fp16's range edge (65519.99 -> 65504,
    65520 -> inf) and values past it — no saturation"""
    n, ns, alpha = 1027, 512, 0.3
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, generator=g) * 3
    x[3], x[4], x[5], x[600], x[601], x[1026] = INF, -INF, NAN, INF, NAN, -INF
    x[8:16] = torch.tensor([65504.0, 65519.996, 65520.0, -65520.0, 70000.0, -1e30, 3e38, -3e38])
    x[700:704] = torch.tensor([65519.996, 65520.0, -70000.0, 3e38])
    x[20:24] = torch.tensor([65520.0, 218400.0, 218399.0, -3e38]) / 1.0          # head region: x * 0.3 crosses 65520 at 218400
    y = torch.full((n,), 5.0, dtype=dt, device="cuda")
    C.cast_bf16(x.cuda(), y)
    assert _same_bits(y, x.to(dt)), f"cast {dt}"
    want = x.clone()
    want[:ns] = want[:ns] * torch.tensor(alpha, dtype=F32)
    y = torch.full((n,), 5.0, dtype=dt, device="cuda")
    C.cast_bf16_head_scaled(x.cuda(), y, ns, alpha)
    assert _same_bits(y, want.to(dt)), f"head-scaled cast {dt}"
    assert assert_no_swallow(y, want.double(), f"head-scaled cast {dt}") == 0
    xs = 1028
    xb = torch.randn(3, xs, generator=g)
    xb[1, :n] = x
    yb = torch.full((3, xs), 5.0, dtype=dt, device="cuda")          # (row strides are multiples of 4 elements)
    C.cast_bf16_head_scaled_strided(xb.cuda(), xs, yb, n, ns, alpha)
    wb = xb[:, :n].clone()
    wb[:, :ns] = wb[:, :ns] * torch.tensor(alpha, dtype=F32)
    assert _same_bits(yb[:, :n].contiguous(), wb.to(dt)) and bool((yb[:, n:] == 5.0).all()), f"strided head-scaled cast {dt}"


@pytest.mark.parametrize("depth", [1, 4])
def test_vq_poisoned_token(C, depth):
    """one coordinate of one token: every index stays inside the codebook, that token's z_q and the loss are non-finite, every other token keeps its
    indices and z_q bit for bit; in the backward that token's dz follows fp64 (the oracle's quantizer on the poisoned z, with the kernel's indices)"""
    import vitvq_oracle as O
    M, K, beta, t0, resid = 96, 512, 0.25, 41, depth > 1
    z, E, g_out = O.make_vq_inputs(3 + depth, M, K)
    z = _nz(z)
    zd, Ed = z.cuda(), E.cuda()
    zq, _, idx, loss = C.vq_forward(zd, Ed, beta, depth, True)
    assert bool(torch.isfinite(zq).all()) and bool(torch.isfinite(loss).all())
    dE = torch.zeros(K, E.shape[1], device="cuda")
    dz, _ = C.vq_backward(zd, Ed, idx, g_out.cuda(), 0.7, None, beta, depth, resid, True, dE)
    tok = _mask((M, 1), t0)
    for pname, pv in POISONS:
        zp = z.clone()
        zp[t0, 3] = pv
        zq_p, _, idx_p, loss_p = C.vq_forward(zp.cuda(), Ed, beta, depth, True)
        tag = f"vq depth {depth} {pname}"
        assert bool(((idx_p >= 0) & (idx_p < K)).all()), tag + ": an index outside the codebook"
        zt = zp.double().clone().requires_grad_(True)
        r_zq, r_loss, _ = O.quantizer_forward(zt, E.double(), beta, True, resid, depth if resid else None, force_idx=idx_p.cpu().view(M, -1) if resid else idx_p.cpu().view(M))
        ((r_zq * g_out.double()).sum() + 0.7 * r_loss).backward()
        # (with residual levels the oracle's loss sees z detached and dz is the straight-through g_out alone: finite — the reference decides)
        assert bool(nonfinite(r_zq[t0]).any()) and bool(nonfinite(r_loss)) and (resid or bool(nonfinite(zt.grad[t0]).any()))
        n = assert_no_swallow(zq_p[t0], r_zq.detach()[t0], tag + " z_q")
        assert assert_no_swallow(loss_p.reshape(()), r_loss.detach(), tag + " loss") == 0
        assert_isolated(zq_p, zq, tok, tag + " z_q")
        assert_isolated(idx_p, idx, tok, tag + " indices")
        dEp = torch.zeros_like(dE)
        dz_p, _ = C.vq_backward(zp.cuda(), Ed, idx_p, g_out.cuda(), 0.7, None, beta, depth, resid, True, dEp)
        n2 = assert_no_swallow(dz_p[t0], zt.grad[t0], tag + " dz")
        assert_isolated(dz_p, dz, tok, tag + " dz")
        print(f"{tag}: indices of the poisoned token {idx_p[t0].tolist()}; spurious non-finite in its z_q {n}, in its dz {n2}")
