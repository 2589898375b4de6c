"""The helper kernels of a stage-1 step — patch gather / scatter with the pixel loss, column sums, the 16-bit casts, LayerNorm forward / backward, AdamW
(csrc/elementwise.hip, csrc/layernorm.hip) and their f32 twins with enh_gemm_f32 (csrc/exact_f32.hip) — held per element to the fp64 references
and limits of tests/step_helpers_util.py (derivations there; tests/test_step_helpers_cpu.py shows that the limits catch the faults the whole-tensor
metric lets through).

Conventions of every case: output buffers are pre-filled with NaN (with old values where the entry accumulates), a sentinel region sits behind
every output and is compared afterwards, the padding behind / between input rows holds NaN (an over-read that reaches arithmetic poisons the
result), both operand formats run where the kernel is a template over them.  The atomic and the workspace (`_ws`) entries of the column sums and of
LayerNorm backward are called directly through the C ABI, whatever ENH_DETERMINISTIC says.  Rejections are checked by return code alone.

Measured on MI355X, the largest err / bound over all cases (test_zz_report prints them; exact cases are bit-equalities and have no figure):
  column sums, Gaussian data: atomic 0.071, _ws 0.071, enh_colsum_f32 0.108
  pixel-loss sums 0.0005 (f32 twin 0.0004); dpix 0.993 (one rounding to 16 bits), f32 twin 0.400
  LayerNorm: mean 0.062, rstd 0.056, y32 0.048, y16 0.998, dx 0.128, dx16 0.985, dw 0.078, db 0.137, dx_colsum 0.023
  AdamW 0.602 of 4 x torch's f32 error + one ulp (p, m, v; per tensor and worst element; steps 1, 2, 3, 1000, 100000)
  enh_gemm_f32 0.118 (every layout and epilogue)
"""
import ctypes

import pytest
import torch

from step_helpers_util import (BF16, F16, F32, F64, TorchAdamW, adamw_check, bits_equal, check, colsum_exact, colsum_ref, dyadic, from_patches,
                               gemm_f32_ref, int_matrix, ln_ref, pixel_loss_ref, to_patches)
from util import h16r

pytestmark = pytest.mark.gpu

DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
GUARD = 64          # sentinel elements behind every output
SENTINEL = 12345.0
NAN = float("nan")


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def ptr(t, off: int = 0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


class Guarded:
    """a device buffer of `n` elements (`.t`, shaped) with GUARD sentinel elements behind it; fill: a number or a CPU tensor of old values"""

    def __init__(self, shape, dtype, fill=NAN):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.n = 1
        for s in shape:
            self.n *= s
        self.whole = torch.empty(self.n + GUARD, dtype=dtype, device="cuda")
        if isinstance(fill, torch.Tensor):
            self.whole[:self.n] = fill.reshape(-1).to(dtype).cuda()
        else:
            self.whole[:self.n] = fill
        self.whole[self.n:] = SENTINEL
        self.t = self.whole[:self.n].view(shape)
        self.before = self.whole[self.n:].clone()

    def intact(self) -> bool:
        return bits_equal(self.whole[self.n:], self.before)

    def cpu(self):
        return self.t.cpu()


def all_intact(what, *bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert b is None or b.intact(), f"{what}: the sentinel behind output {i} was overwritten"


def dev_in(x: torch.Tensor, dtype=None, pad: int = 8):
    """an input on the device with `pad` NaN elements behind it"""
    dtype = x.dtype if dtype is None else dtype
    whole = torch.full((x.numel() + pad,), NAN, dtype=dtype, device="cuda")
    whole[:x.numel()] = x.reshape(-1).to(dtype).cuda()
    return whole[:x.numel()].view(x.shape)


WORST = {}


def note(key: str, value: float):
    WORST[key] = max(WORST.get(key, 0.0), value)
    assert value <= 1.0, (key, value)


# =====================================================================================================================================================
# column sums
# =====================================================================================================================================================
# (M, N, ldx, base offset in elements).  M: fewer rows than waves; one pass + remainder of the 16-row unroll; exactly one chunk; two chunks; 17 chunks
# (a ragged group in the second pass); beyond the 256-chunk cap.  N = 520: a second column block with one live lane.
COLSUM_WIDE = [(M, N, N, 0) for M in (3, 17, 512, 513, 8701) for N in (8, 520, 1024)] + [(131077, 24, 24, 0)]
COLSUM_NARROW = [(513, 130, 130, 0), (513, 136, 138, 0), (513, 136, 136, 2)]          # each dispatch condition of the narrow kernel alone
COLSUM_STRIDED = [(513, 520, 528, 0), (513, 520, 520, 8)]                              # the wide kernel off the dense layout
COLSUM_CASES = COLSUM_WIDE + COLSUM_NARROW + COLSUM_STRIDED


def _strided_input(x: torch.Tensor, ld: int, off: int, dtype):
    """x [M, N] laid out with row stride ld from element `off` of a NaN-filled allocation; returns (allocation, offset)"""
    M, N = x.shape
    whole = torch.full((off + M * ld + 16,), NAN, dtype=dtype, device="cuda")
    whole[off:off + M * ld].view(M, ld)[:, :N] = x.to(dtype).cuda()
    return whole, off


def _colsum_run(L, C, entry, xw, off, M, N, ld, old, accumulate, dti):
    """one launch of enh_colsum_h16 (entry 'atomic'), enh_colsum_h16_ws ('ws') or enh_colsum_f32 ('f32'); returns the guarded output [, workspace]"""
    out = Guarded(N, F32, old if accumulate else NAN)
    ws = None
    if entry == "ws":
        nb = L.enh_colsum_h16_workspace_bytes(M, N)
        assert nb % 4 == 0 and nb >= 4 * N
        ws = Guarded(nb // 4, F32)
        rc = L.enh_colsum_h16_ws(ptr(xw, off), M, N, ld, ptr(out.t), int(accumulate), ptr(ws.t), nb, dti, C._stream())
    elif entry == "atomic":
        rc = L.enh_colsum_h16(ptr(xw, off), M, N, ld, ptr(out.t), int(accumulate), dti, C._stream())
    else:
        rc = L.enh_colsum_f32(ptr(xw, off), M, N, ld, ptr(out.t), int(accumulate), C._stream())
    assert rc == 0, L.enh_last_error().decode()
    all_intact(f"colsum {entry} {M}x{N} ld {ld} off {off}", out, ws)
    return out.cpu()


@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("M,N,ld,off", COLSUM_CASES, ids=lambda v: str(v))
def test_column_sums(C, M, N, ld, off, dt):
    """integer data: the int64 sums bit for bit in every form and mode; Gaussian data: the element bound; the _ws form twice: the same bits"""
    L = C.lib()
    entries = ("f32",) if dt == F32 else ("atomic", "ws")
    dti = {BF16: C.DT_BF16, F16: C.DT_F16, F32: C.DT_F32}[dt]
    g = torch.Generator().manual_seed(M * 7 + N + ld + off)
    xi = int_matrix(M, N, M + N)
    xg = torch.randn(M, N, generator=g)
    xg = xg if dt == F32 else h16r(xg, dt)
    old_i = torch.randint(-50, 51, (N,), generator=g).float()
    old_g = torch.randn(N, generator=g) * 3
    xiw, _ = _strided_input(xi, ld, off, dt)
    xgw, _ = _strided_input(xg, ld, off, dt)
    what = f"colsum {M}x{N} ld {ld} off {off} {dt}"
    for entry in entries:
        for acc in (False, True):
            got = _colsum_run(L, C, entry, xiw, off, M, N, ld, old_i, acc, dti)
            assert bits_equal(got, colsum_exact(xi, old_i if acc else None)), f"{what} {entry} accumulate={acc}: integer sums are not exact"
            got = _colsum_run(L, C, entry, xgw, off, M, N, ld, old_g, acc, dti)
            ref, bound = colsum_ref(xg, old_g if acc else None)
            note(f"colsum {entry}", check(got, ref, bound, f"{what} {entry} accumulate={acc}"))
            if entry == "ws":
                assert bits_equal(got, _colsum_run(L, C, entry, xgw, off, M, N, ld, old_g, acc, dti)), f"{what}: two launches of the _ws form differ"


def test_column_sum_rejections(C):
    L = C.lib()
    x = torch.zeros(64 * 16, dtype=BF16, device="cuda")
    out = Guarded(16, F32)
    ws = torch.zeros(4096, device="cuda")
    s = C._stream()
    assert L.enh_colsum_h16(ptr(x), 8, 7, 8, ptr(out.t), 0, C.DT_BF16, s) != 0          # odd N
    assert L.enh_colsum_h16(ptr(x), 8, 8, 9, ptr(out.t), 0, C.DT_BF16, s) != 0          # odd ldx
    assert L.enh_colsum_h16_ws(ptr(x), 8, 7, 8, ptr(out.t), 0, ptr(ws), 4096 * 4, C.DT_BF16, s) != 0
    need = L.enh_colsum_h16_workspace_bytes(8, 8)
    assert need == 8 * 4
    assert L.enh_colsum_h16_ws(ptr(x), 8, 8, 8, ptr(out.t), 0, ptr(ws), need - 1, C.DT_BF16, s) != 0          # a workspace one byte short
    assert L.enh_colsum_h16_ws(ptr(x), 8, 8, 8, ptr(out.t), 0, None, need, C.DT_BF16, s) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.cpu()).all()) and out.intact(), "a rejected call wrote its output"


# =====================================================================================================================================================
# patchify, unpatchify + pixel loss, and the f32 twins
# =====================================================================================================================================================
# 12 live lanes in one wave; both non-square orientations; a quad count that is no multiple of 256 (last workgroup with idle lanes); C other than 3
GEOMS = [(1, 1, 4, 12, 4), (2, 3, 16, 32, 8), (3, 5, 32, 16, 16), (1, 3, 24, 40, 8), (2, 1, 64, 16, 4)]
GEOMS_F32 = GEOMS + [(1, 3, 6, 10, 2), (2, 2, 3, 5, 1)]          # the twins do not need p % 4
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (0.3, 1.0)]
OLD_SUMS = torch.tensor([3.5, -1.25], dtype=F64)          # what sums held before: the kernels add into it


def _pixel_case(B, Cc, H, W, p, seed):
    g = torch.Generator().manual_seed(seed)
    M, K = B * (H // p) * (W // p), Cc * p * p
    target = torch.rand(B, Cc, H, W, generator=g)
    pix = torch.randn(M, K, generator=g)
    tp = to_patches(target, p)
    pix[::2, ::3] = tp[::2, ::3]          # planted elements with pix == target: d == 0
    return pix, target, dyadic((M, K), seed + 1), dyadic((B, Cc, H, W), seed + 2)


def _expected_l1_grad(pix, target, p, w_l1, scale, numel, dt):
    """w_l2 = 0: the gradient is 0 where pix == target and +-round(w_l1 * (fl(1 / numel) * scale)) elsewhere, exactly"""
    d = pix - to_patches(target, p)
    inv = (torch.tensor(1.0, dtype=F32) / torch.tensor(float(numel), dtype=F32)) * torch.tensor(scale, dtype=F32)
    g = torch.tensor(w_l1, dtype=F32) * inv
    return (torch.sign(d) * g).to(F32 if dt is None else dt)


@DTS
@pytest.mark.parametrize("B,Cc,H,W,p", GEOMS, ids=lambda v: str(v))
def test_patchify_unpatchify_loss(C, B, Cc, H, W, p, dt):
    L = C.lib()
    dti = C.DT_BF16 if dt == BF16 else C.DT_F16
    what = f"{B}x{Cc}x{H}x{W} p={p} {dt}"
    pix, target, pix_d, target_d = _pixel_case(B, Cc, H, W, p, B + Cc + H + W + p)
    M, K, numel = pix.shape[0], pix.shape[1], B * Cc * H * W
    # patchify: the permutation and one round-to-nearest-even cast
    out = Guarded((M, K), dt)
    imgd = dev_in(target)
    assert L.enh_patchify(ptr(imgd), B, Cc, H, W, p, ptr(out.t), dti, C._stream()) == 0, L.enh_last_error().decode()
    all_intact("patchify " + what, out)
    assert bits_equal(out.cpu(), to_patches(target, p).to(dt)), "patchify " + what
    scale_dev = torch.tensor([1024.0], device="cuda")
    for px, tg, exact in ((pix, target, False), (pix_d, target_d, True)):
        pxd, tgd = dev_in(px), dev_in(tg)
        for w1, w2 in WEIGHTS:
            for mode in ("all", "all_scaled", "xrec_only", "loss_only", "no_dpix"):
                scale = 1024.0 if mode == "all_scaled" else 1.0
                xrec = None if mode == "loss_only" else Guarded((B, Cc, H, W), F32)
                sums = Guarded(2, F64, OLD_SUMS)
                dpix = Guarded((M, K), dt)
                rc = L.enh_unpatchify_loss(ptr(pxd), None if mode == "xrec_only" else ptr(tgd), B, Cc, H, W, p, w1, w2, None if xrec is None else ptr(xrec.t),
                                           ptr(sums.t), None if mode == "no_dpix" else ptr(dpix.t), ptr(scale_dev) if mode == "all_scaled" else None, dti,
                                           C._stream())
                assert rc == 0, L.enh_last_error().decode()
                tag = f"unpatchify {what} w=({w1}, {w2}) {mode}{' dyadic' if exact else ''}"
                all_intact(tag, xrec, sums, dpix)
                if xrec is not None:
                    assert bits_equal(xrec.cpu(), from_patches(px, B, Cc, H, W, p)), tag + ": xrec"
                if mode == "xrec_only":
                    assert torch.equal(sums.cpu(), OLD_SUMS) and bool(torch.isnan(dpix.cpu().float()).all()), tag + ": sums or dpix written without a target"
                    continue
                s_ref, g_ref, s_bound, g_bound = pixel_loss_ref(px, tg, p, w1, w2, scale, dt)
                if exact:
                    assert torch.equal(sums.cpu(), s_ref + OLD_SUMS), tag + ": sums are not exact"
                note("pixel-loss sums", check(sums.cpu(), s_ref + OLD_SUMS, s_bound, tag + " sums"))
                if mode == "no_dpix":
                    assert bool(torch.isnan(dpix.cpu().float()).all()), tag + ": dpix written although absent"
                    continue
                note("dpix", check(dpix.cpu(), g_ref, g_bound, tag + " dpix"))
                if w2 == 0.0:
                    assert bits_equal(dpix.cpu(), _expected_l1_grad(px, tg, p, w1, scale, numel, dt)), tag + ": the L1 gradient is not exactly 0 / +-w_l1 scale / numel"


@pytest.mark.parametrize("B,Cc,H,W,p", GEOMS_F32, ids=lambda v: str(v))
def test_patch_twins_f32(C, B, Cc, H, W, p):
    L = C.lib()
    what = f"f32 {B}x{Cc}x{H}x{W} p={p}"
    pix, target, pix_d, target_d = _pixel_case(B, Cc, H, W, p, B + Cc + H + W + p)
    M, K, numel = pix.shape[0], pix.shape[1], B * Cc * H * W
    out = Guarded((M, K), F32)
    srcs = (dev_in(target), dev_in(pix))          # (held: a temporary's memory is handed to the next allocation)
    assert L.enh_patch_perm_f32(ptr(srcs[0]), ptr(out.t), B, Cc, H, W, p, 1, C._stream()) == 0, L.enh_last_error().decode()
    img = Guarded((B, Cc, H, W), F32)
    assert L.enh_patch_perm_f32(ptr(srcs[1]), ptr(img.t), B, Cc, H, W, p, 0, C._stream()) == 0, L.enh_last_error().decode()
    all_intact("patch_perm " + what, out, img)
    assert bits_equal(out.cpu(), to_patches(target, p).contiguous()) and bits_equal(img.cpu(), from_patches(pix, B, Cc, H, W, p).contiguous()), "patch_perm " + what
    for px, tg, exact in ((pix, target, False), (pix_d, target_d, True)):
        pxd, tgd = dev_in(px), dev_in(tg)
        for w1, w2 in WEIGHTS:
            xrec, sums, dpix = Guarded((B, Cc, H, W), F32), Guarded(2, F64, OLD_SUMS), Guarded((M, K), F32)
            rc = L.enh_unpatchify_loss_f32(ptr(pxd), ptr(tgd), B, Cc, H, W, p, w1, w2, ptr(xrec.t), ptr(sums.t), ptr(dpix.t), C._stream())
            assert rc == 0, L.enh_last_error().decode()
            tag = f"unpatchify {what} w=({w1}, {w2}){' dyadic' if exact else ''}"
            all_intact(tag, xrec, sums, dpix)
            assert bits_equal(xrec.cpu(), from_patches(px, B, Cc, H, W, p).contiguous()), tag + ": xrec"
            s_ref, g_ref, s_bound, g_bound = pixel_loss_ref(px, tg, p, w1, w2, 1.0, None)
            if exact:
                assert torch.equal(sums.cpu(), s_ref + OLD_SUMS), tag + ": sums are not exact"
            note("pixel-loss sums f32", check(sums.cpu(), s_ref + OLD_SUMS, s_bound, tag + " sums"))
            note("dpix f32", check(dpix.cpu(), g_ref, g_bound, tag + " dpix"))
            if w2 == 0.0:
                assert bits_equal(dpix.cpu(), _expected_l1_grad(px, tg, p, w1, 1.0, numel, None)), tag + ": the L1 gradient is not exactly 0 / +-w_l1 / numel"


def test_patch_rejections(C):
    L = C.lib()
    s = C._stream()
    src = torch.zeros(4096, device="cuda")
    o16, o32, sums = Guarded(4096, BF16), Guarded(4096, F32), Guarded(2, F64)
    assert L.enh_patchify(ptr(src), 1, 1, 12, 12, 6, ptr(o16.t), C.DT_BF16, s) != 0                                                       # p % 4 != 0
    assert L.enh_patchify(ptr(src), 1, 1, 12, 16, 8, ptr(o16.t), C.DT_BF16, s) != 0                                                       # H % p != 0
    assert L.enh_unpatchify_loss(ptr(src), ptr(src), 1, 1, 12, 12, 6, 1.0, 1.0, ptr(o32.t), ptr(sums.t), ptr(o16.t), None, C.DT_BF16, s) != 0
    assert L.enh_unpatchify_loss(ptr(src), ptr(src), 1, 1, 12, 16, 8, 1.0, 1.0, ptr(o32.t), ptr(sums.t), ptr(o16.t), None, C.DT_BF16, s) != 0
    assert L.enh_patch_perm_f32(ptr(src), ptr(o32.t), 1, 1, 12, 16, 8, 1, s) != 0
    assert L.enh_unpatchify_loss_f32(ptr(src), ptr(src), 1, 1, 12, 16, 8, 1.0, 1.0, ptr(o32.t), ptr(sums.t), ptr(o32.t), s) != 0
    torch.cuda.synchronize()
    for o in (o16, o32, sums):
        assert bool(torch.isnan(o.cpu().double()).all()) and o.intact(), "a rejected call wrote its output"


# =====================================================================================================================================================
# casts
# =====================================================================================================================================================
@DTS
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_casts(C, n, dt):
    L = C.lib()
    dti = C.DT_BF16 if dt == BF16 else C.DT_F16
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3
    y, xd = Guarded(n, dt), dev_in(x)
    assert L.enh_cast_f32_h16(ptr(xd), ptr(y.t), n, dti, C._stream()) == 0, L.enh_last_error().decode()
    all_intact(f"cast n={n}", y)
    assert bits_equal(y.cpu(), x.to(dt)), f"cast n={n} {dt}"
    alpha = 0.3
    for ns in sorted({0, 4 if n >= 4 else 0, n // 4 * 4}):
        want = x.clone()
        want[:ns] = want[:ns] * torch.tensor(alpha, dtype=F32)          # one f32 product, then the one rounding of the cast
        y = Guarded(n, dt)
        assert L.enh_cast_f32_h16_head_scaled(ptr(xd), ptr(y.t), n, ns, alpha, dti, C._stream()) == 0, L.enh_last_error().decode()
        all_intact(f"head-scaled cast n={n} n_scaled={ns}", y)
        assert bits_equal(y.cpu(), want.to(dt)), f"head-scaled cast n={n} n_scaled={ns} {dt}"
        # the strided form: three blocks, a gap between the outputs that keeps its sentinel
        count, xs, ys = 3, (n + 3) // 4 * 4 + 4, (n + 3) // 4 * 4 + 8
        xb = torch.randn(count, xs, generator=g)
        yb, xbd = Guarded((count, ys), dt, SENTINEL), dev_in(xb)
        rc = L.enh_cast_f32_h16_head_scaled_strided(ptr(xbd), xs, ptr(yb.t), ys, n, ns, alpha, count, dti, C._stream())
        assert rc == 0, L.enh_last_error().decode()
        all_intact(f"strided cast n={n}", yb)
        wb = xb[:, :n].clone()
        wb[:, :ns] = wb[:, :ns] * torch.tensor(alpha, dtype=F32)
        got = yb.cpu()
        assert bits_equal(got[:, :n].contiguous(), wb.to(dt)), f"strided cast n={n} n_scaled={ns} {dt}"
        assert bits_equal(got[:, n:].contiguous(), torch.full((count, ys - n), SENTINEL).to(dt)), f"strided cast n={n}: the gap between the outputs was written"


# =====================================================================================================================================================
# LayerNorm forward and backward
# =====================================================================================================================================================
# NCH 1 (one lane; full), 2 (one live lane in the second chunk), 3, 4, 5, and 8 (with and without idle chunks)
LN_SHAPES = [(M, D) for D in (4, 256, 260, 768, 1024, 1280, 1540, 2048) for M in (1, 3, 37)] + [(1027, 768)]
# (16-bit dy, workspace form, dres, dx16 + dx_colsum): every level of every factor in both forms
LN_WAYS = [(False, False, True, True), (False, True, False, False), (True, False, False, True), (True, True, True, False)]


def _ln_backward(L, C, ws_form, dy16, dyd, xd, wd, mean, rstd, dresd, M, D, old, extras, dt, dti):
    """one launch of enh_layernorm_backward / _ws.  CONTRACT: both forms ADD into dw, db and dx_colsum (pre-filled with old values here); dx and dx16 are
    overwritten (pre-filled with NaN).  Returns the outputs on the CPU."""
    dx, dx16 = Guarded((M, D), F32), (Guarded((M, D), dt) if extras else None)
    dw, db = Guarded(D, F32, old[0]), Guarded(D, F32, old[1])
    dxs = Guarded(D, F32, old[2]) if extras else None
    args = [None if dy16 else ptr(dyd), ptr(dyd) if dy16 else None, ptr(xd), ptr(wd), ptr(mean), ptr(rstd), ptr(dresd), M, D, ptr(dx.t),
            None if dx16 is None else ptr(dx16.t), ptr(dw.t), ptr(db.t), None if dxs is None else ptr(dxs.t)]
    ws = None
    if ws_form:
        nb = L.enh_layernorm_backward_workspace_bytes(M, D)
        ws = Guarded(nb // 4, F32)
        rc = L.enh_layernorm_backward_ws(*args, ptr(ws.t), nb, dti, C._stream())
    else:
        rc = L.enh_layernorm_backward(*args, dti, C._stream())
    assert rc == 0, L.enh_last_error().decode()
    all_intact(f"layernorm backward {M}x{D} ws={ws_form}", dx, dx16, dw, db, dxs, ws)
    got = dict(dx=dx.cpu(), dw=dw.cpu(), db=db.cpu())
    if extras:
        got.update(dx16=dx16.cpu(), dx_colsum=dxs.cpu())
    return got


def _ln_check_backward(got, refs, what, dt):
    for k, t in got.items():
        note(f"layernorm {k}", check(t, *refs[k], f"{what} {k}"))
    if "dx16" in got:
        assert bits_equal(got["dx16"], got["dx"].to(dt)), what + ": dx16 is not the rounded dx"


@DTS
@pytest.mark.parametrize("M,D", LN_SHAPES, ids=lambda v: str(v))
def test_layernorm(C, M, D, dt):
    L = C.lib()
    dti = C.DT_BF16 if dt == BF16 else C.DT_F16
    g = torch.Generator().manual_seed(M * 3 + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dy32 = torch.randn(M, D, generator=g)
    dres = torch.randn(M, D, generator=g)
    old = [torch.randn(D, generator=g) for _ in range(3)]
    what = f"layernorm {M}x{D} {dt}"
    xd, wd, bd = dev_in(x), dev_in(w), dev_in(b)
    y16, y32, mean, rstd = Guarded((M, D), dt), Guarded((M, D), F32), Guarded(M, F32), Guarded(M, F32)
    rc = L.enh_layernorm_forward(ptr(xd), ptr(wd), ptr(bd), M, D, 1e-5, ptr(y16.t), ptr(y32.t), ptr(mean.t), ptr(rstd.t), dti, C._stream())
    assert rc == 0, L.enh_last_error().decode()
    all_intact(what + " forward", y16, y32, mean, rstd)
    fwd = ln_ref(x, w, b, dt=dt)
    for k, t in (("mean", mean), ("rstd", rstd), ("y32", y32), ("y16", y16)):
        note(f"layernorm {k}", check(t.cpu(), *fwd[k], f"{what} {k}"))
    assert bits_equal(y16.cpu(), y32.cpu().to(dt)), what + ": y16 is not the rounded y32"
    ways = [(a, f, r, e, 0) for a, f, r, e in LN_WAYS]
    if M == 37 and D in (260, 768):          # two workgroups: five rows per workgroup through the pipelined row loop, idle waves in the last pass
        ways += [(False, False, True, True, 2), (True, True, True, True, 2)]
    budget0 = C.get_cu_budget()
    for dy16, ws_form, use_dres, extras, budget in ways:
        dy = h16r(dy32, dt) if dy16 else dy32
        refs = ln_ref(x, w, b, dy, dres if use_dres else None, old, dt)
        dyd, dresd = dev_in(dy, dt if dy16 else F32), (dev_in(dres) if use_dres else None)
        tag = f"{what} dy16={dy16} ws={ws_form} dres={use_dres} extras={extras} budget={budget}"
        try:
            if budget:
                C.set_cu_budget(budget)
            got = _ln_backward(L, C, ws_form, dy16, dyd, xd, wd, mean.t, rstd.t, dresd, M, D, old, extras, dt, dti)
            again = _ln_backward(L, C, ws_form, dy16, dyd, xd, wd, mean.t, rstd.t, dresd, M, D, old, extras, dt, dti) if ws_form else None
        finally:
            C.set_cu_budget(budget0)
        _ln_check_backward(got, refs, tag, dt)
        if again is not None:
            assert all(bits_equal(got[k], again[k]) for k in got), tag + ": two launches of the _ws form differ"


def test_layernorm_rejections(C):
    L = C.lib()
    s = C._stream()
    z = torch.zeros(4 * 2052, device="cuda")
    z16 = torch.zeros(4 * 2052, dtype=BF16, device="cuda")
    out = [Guarded(4 * 2052, F32) for _ in range(4)]
    o16 = Guarded(4 * 2052, BF16)
    fwd = lambda D: L.enh_layernorm_forward(ptr(z), ptr(z), ptr(z), 4, D, 1e-5, ptr(o16.t), ptr(out[0].t), ptr(out[1].t), ptr(out[2].t), C.DT_BF16, s)
    bwd = lambda D, dy, dy16: L.enh_layernorm_backward(dy, dy16, ptr(z), ptr(z), ptr(z), ptr(z), None, 4, D, ptr(out[0].t), ptr(o16.t), ptr(out[1].t),
                                                       ptr(out[2].t), ptr(out[3].t), C.DT_BF16, s)
    assert fwd(6) != 0 and fwd(2052) != 0
    assert bwd(6, ptr(z), None) != 0 and bwd(2052, ptr(z), None) != 0
    assert bwd(8, ptr(z), ptr(z16)) != 0 and bwd(8, None, None) != 0          # both, neither of dy / dy_bf16
    nb = L.enh_layernorm_backward_workspace_bytes(4, 8)
    assert L.enh_layernorm_backward_ws(ptr(z), None, ptr(z), ptr(z), ptr(z), ptr(z), None, 4, 8, ptr(out[0].t), ptr(o16.t), ptr(out[1].t), ptr(out[2].t),
                                       ptr(out[3].t), ptr(z), nb - 1, C.DT_BF16, s) != 0
    torch.cuda.synchronize()
    for o in out + [o16]:
        assert bool(torch.isnan(o.cpu().float()).all()) and o.intact(), "a rejected call wrote its output"


# =====================================================================================================================================================
# AdamW
# =====================================================================================================================================================
ADAM_STEPS = (1, 2, 3, 1000, 100000)


def _adamw_case(n: int, seed: int):
    """gradients: most about 1e-2, a slice about 1e-8, a slice exactly zero, one element 1e3.  Parameters: N(0, 1), and (where the slices exist) values
    that overflow the fp16 shadow and values in its subnormal range — placed in the zero-gradient slice, where the step leaves them in their range."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 1e-2
    ordinary = torch.ones(n, dtype=torch.bool)
    if n >= 8:
        s = n // 8
        g[s:2 * s] = torch.randn(s, generator=gen) * 1e-8
        g[2 * s:3 * s] = 0.0
        g[n - 1] = 1e3
        p[2 * s:2 * s + 4] = torch.tensor([70000.0, -1.0e5, 3.0e-6, -5.0e-8])
        ordinary[2 * s:2 * s + 4] = False
    return p, g, ordinary


@DTS
@pytest.mark.parametrize("lr,wd", [(1e-2, 0.1), (4.5e-6, 1e-4)], ids=["visible_decay", "shipped"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4101])
def test_adamw(C, n, lr, wd, dt):
    p0, g, ordinary = _adamw_case(n, n)
    f32, ref = TorchAdamW(p0, F32, lr, wd), TorchAdamW(p0, F64, lr, wd)
    p, m, v, p16 = Guarded(n, F32, p0), Guarded(n, F32, 0.0), Guarded(n, F32, 0.0), Guarded(n, dt)
    skip = torch.ones(1, device="cuda")
    what = f"AdamW n={n} lr={lr} wd={wd} {dt}"
    for t in ADAM_STEPS:
        gt = g * (1.0 + 0.25 * (t % 3))
        gd = dev_in(gt)
        before = [b.whole.clone() for b in (p, m, v, p16)]
        C.adamw_step(p.t, gd, m.t, v.t, p16.t, t, lr, weight_decay=wd, skip_flag=skip)          # a skipped step: every byte stays
        torch.cuda.synchronize()
        assert all(bits_equal(b.whole, o) for b, o in zip((p, m, v, p16), before)), f"{what} step {t}: a skipped step wrote"
        C.adamw_step(p.t, gd, m.t, v.t, p16.t, t, lr, weight_decay=wd)
        all_intact(f"{what} step {t}", p, m, v, p16)
        note("AdamW", adamw_check((p.cpu(), m.cpu(), v.cpu()), f32.step(gt, t), ref.step(gt, t), f"{what} step {t}", keep=ordinary))
        assert bits_equal(p16.cpu(), p.cpu().to(dt)), f"{what} step {t}: the 16-bit shadow is not the rounded p"
    if n >= 8 and dt == F16:
        s = n // 8
        sh = p16.cpu()[2 * s:2 * s + 4].float()
        assert bool(torch.isinf(sh[:2]).all()) and 0 < abs(sh[2].item()) < 2.0 ** -14 and 0 < abs(sh[3].item()) < 2.0 ** -14, "the special parameters left their ranges"


# =====================================================================================================================================================
# enh_gemm_f32
# =====================================================================================================================================================
GEMM_EPILOGUES = ["none", "bias", "bias_tanh", "dtanh_strided_aux", "bias_res_in_place", "pos_table", "accumulate"]


def _padded(x: torch.Tensor, ld: int, fill: float):
    """x [R, Cn] stored with row stride ld, `fill` in the padding; returns the guarded buffer [R, ld]"""
    R, Cn = x.shape
    host = torch.full((R, ld), fill)
    host[:, :Cn] = x
    return Guarded((R, ld), F32, host)


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(70, 66, 19), (64, 64, 16), (1, 5, 3)])
def test_gemm_f32(C, M, N, K, ta, tb):
    L = C.lib()
    g = torch.Generator().manual_seed(M + N + K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.3
    bias, h = torch.randn(N, generator=g), torch.tanh(torch.randn(M, N, generator=g))
    res, pos, old = torch.randn(M, N, generator=g), torch.randn(7, N, generator=g), torch.randn(M, N, generator=g)
    As, Bs = (A.t().contiguous() if ta else A), (B.t().contiguous() if tb else B)          # trans_a: A stored [K, M]; trans_b: B stored [K, N]
    lda, ldb, ldc = As.shape[1] + 3, Bs.shape[1] + 5, N + 3
    Ad, Bd = _padded(As, lda, NAN), _padded(Bs, ldb, NAN)
    biasd, auxd, posd = dev_in(bias), _padded(h, N + 5, NAN), _padded(pos, N + 2, NAN)
    for epi in GEMM_EPILOGUES:
        kw = dict(bias=None, act=C.ACT_NONE, aux=None, ldaux=0, res=None, ldres=0, res_rows=0, acc=0)
        init, ref = torch.full((M, N), NAN), None
        if epi == "none":
            ref = gemm_f32_ref(A, B)
        elif epi == "bias":
            kw.update(bias=biasd)
            ref = gemm_f32_ref(A, B, bias)
        elif epi == "bias_tanh":
            kw.update(bias=biasd, act=C.ACT_TANH)
            ref = gemm_f32_ref(A, B, bias, act="tanh")
        elif epi == "dtanh_strided_aux":
            kw.update(act=C.ACT_DTANH, aux=auxd.t, ldaux=N + 5)
            ref = gemm_f32_ref(A, B, act="dtanh", aux=h)
        elif epi == "bias_res_in_place":
            init = res
            ref = gemm_f32_ref(A, B, bias, res=res, res_rows=M)
        elif epi == "pos_table":
            kw.update(bias=biasd, res=posd.t, ldres=N + 2, res_rows=7)
            ref = gemm_f32_ref(A, B, bias, res=pos, res_rows=7)
        else:
            init = old
            kw.update(acc=1)
            ref = gemm_f32_ref(A, B, old=old)
        Cd = _padded(init, ldc, SENTINEL)
        if epi == "bias_res_in_place":
            kw.update(bias=biasd, res=Cd.t, ldres=ldc, res_rows=M)
        rc = L.enh_gemm_f32(ptr(Ad.t), lda, int(ta), ptr(Bd.t), ldb, int(tb), M, N, K, ptr(kw["bias"]), kw["act"], ptr(kw["aux"]), kw["ldaux"], ptr(kw["res"]),
                            kw["ldres"], kw["res_rows"], kw["acc"], ptr(Cd.t), ldc, C._stream())
        assert rc == 0, L.enh_last_error().decode()
        what = f"gemm_f32 {M}x{N}x{K} ta={ta} tb={tb} {epi}"
        all_intact(what, Cd, Ad, Bd, auxd, posd)
        got = Cd.cpu()
        assert bool((got[:, N:] == SENTINEL).all()), what + ": the padding of C was written"
        note("gemm_f32", check(got[:, :N], *ref, what))


def test_zz_report():
    """prints the largest err / bound seen per kernel and output in this session (the figures of the module docstring)"""
    print("step helpers, max err / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items())))
