"""References and per-element limits for the helper kernels of a stage-1 step (csrc/elementwise.hip, csrc/layernorm.hip and their f32 twins in
csrc/exact_f32.hip), shared by tests/test_step_helpers_cpu.py (which proves the limits have teeth on f32 restatements of the kernels) and
tests/test_step_helpers_gpu.py (which holds the kernels to them).

Every kernel has a plain fp64 reference computed from the same f32 / 16-bit inputs and a limit per element that follows from the operands alone, in
the manner of util.elem_bound:  u(dt) |ref| + sub(dt) + (2 k + 8) 2^-24 mag.  No constant here is measured or tuned.

Exact cases (no tolerance; any dropped or doubled element shows):
  * column sums of integers in [-4, 4] (exact in bf16 / fp16): every f32 partial sum is an integer below 2^24 (4 x 131077 < 2^20), so any order of
    f32 additions, atomic or not, gives the int64 sum bit for bit;
  * pixel-loss sums of operands on the grid of multiples of 1/8 in [-4, 4]: d is a multiple of 1/8 with |d| <= 8, d^2 a multiple of 1/64 <= 64, a
    workgroup's 1024 terms sum to at most 2^16 in units of 2^-6 (22 bits): exact in f32; the f64 atomics then add numbers of at most 40 bits;
  * data movement (patchify, xrec, patch_perm_f32, the casts, AdamW's 16-bit shadow): torch's permute and round-to-nearest-even cast, bit for bit.

Bounded cases, with `mag` the same operation on absolute values:
  * column sums, Gaussian data: elem_bound(ref, colsum |x| + |old|, k = M).
  * pixel-loss sums, Gaussian data: elem_bound(ref, ref, k = 1024) — a workgroup makes ONE f32 sum of 1024 non-negative terms (each term itself one
    or two roundings: the +8 of the bound), everything after it is f64.
  * dpix: one rounding to the stored format of (w_l1 sign d + 2 w_l2 d) scale / numel, a handful of f32 operations on a correctly rounded d:
    elem_bound(ref, (w_l1 |sign d| + 2 w_l2 |d|) scale / numel, 0, dt).
  * LayerNorm mean: elem_bound(mean, mean |x|, k = D) (an f32 sum of D terms and one division).
  * LayerNorm rstd = (var + eps)^-1/2, var = mean (x - mean)^2.  The f32 difference d^ = fl(x - mean^) is off by at most
        e_d = 2^-24 (|x| + |mean|) + b_mean          (the rounding of the subtraction, bounded by its operands: the cancellation term; + the mean's own)
    so d^2 is off by 2 |d| e_d (first order), var by  b_var = (2 D + 8) 2^-24 var + mean_j (2 |d_j| e_dj),  and rstd by
        b_rstd = 1/2 rstd^3 b_var + 8 * 2^-24 rstd    (the derivative of v^-1/2, plus the division, square root and reciprocal)
  * LayerNorm y32 = w x^ + b with x^ = d^ rstd^:  |w| (rstd e_d + |d| b_rstd) + 8 * 2^-24 (|w| |x^| + |b|).
    y16 keeps the formula of tests/test_elementwise_gpu.py test_layernorm_every_element: elem_bound(y, |w| |x^| + |b|, 0, dt); y16 == round(y32) bit for bit.
  * LayerNorm dx = rstd (w dy - mean(w dy) - x^ mean(w dy x^)) + dres: elem_bound(dx, mag_dx, k = D[, dt]) with the magnitude of
    test_layernorm_every_element; dx16 == round(dx) bit for bit.
  * LayerNorm dw, db, dx_colsum (both forms ADD into them): the magnitudes and k of tests/test_gpt_backward_kernels_gpu.py test_ln_timeshift_backward:
    k = D + M on sum_m |dy| |x^| + |old|, k = M on sum_m |dy| + |old|, k = 3 D + M on sum_m mag_dx + |old|.
  * AdamW: gpt_train_util.check_limit — error of the device <= 4 x the error of torch.optim.AdamW in f32 on the CPU + one f32 ulp, both against
    torch.optim.AdamW in fp64 fed the same f32 gradients; per tensor (2-norm) and for the worst element; p, m and v.  Both torch runs take the
    hyper-parameters as the f32 values the C ABI carries (lr, betas, eps, weight_decay are `float` arguments).  A first version of this reference
    used the Python doubles and the honest f32 restatement missed the limit on m at step 1 (1.07 x): 0.9f = 0.9 (1 - 2.6e-8), so 1 - beta1 is
    0.1 (1 + 2.4e-7), two ulps of m that no kernel behind this ABI can avoid.  The reference was wrong, not the limit, which is unchanged.
  * enh_gemm_f32: elem_bound(ref, |A| |B| + |bias| + |res| + |C_old|, K), the epilogue's derivative factor applied to the magnitude, TANH_ABS for tanh.
"""
import torch

from gpt_train_util import check_limit
from util import TANH_ABS, assert_elementwise, elem_bound

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
EPS24 = 2.0 ** -24
LN_EPS = 1e-5


# ---- column sums ------------------------------------------------------------------------------------------------------------------------------------
def int_matrix(M: int, N: int, seed: int) -> torch.Tensor:
    """integers in [-4, 4] as f32: exact in both 16-bit formats"""
    return torch.randint(-4, 5, (M, N), generator=torch.Generator().manual_seed(seed)).float()


def colsum_exact(x: torch.Tensor, old=None, times: int = 1) -> torch.Tensor:
    """the int64 column sums of an integer-valued matrix (`times` of them on top of integer-valued `old`), as f32: what every form must give bit for bit"""
    s = x.to(torch.int64).sum(0) * times
    if old is not None:
        s = s + old.to(torch.int64)
    assert int(s.abs().max()) < 2 ** 24
    return s.float()


def colsum_ref(x: torch.Tensor, old=None):
    """(fp64 column sums [+ old], element bound) of a matrix of f32 / 16-bit values"""
    xd = x.double()
    o = torch.zeros(x.shape[1], dtype=F64) if old is None else old.double()
    ref = xd.sum(0) + o
    return ref, elem_bound(ref, xd.abs().sum(0) + o.abs(), x.shape[0])


# ---- patch gather / scatter and the pixel loss ------------------------------------------------------------------------------------------------------
def to_patches(img: torch.Tensor, p: int) -> torch.Tensor:
    """[B, C, H, W] -> [B gy gx, C p p], rows ordered (b, gy, gx), columns (c, ph, pw): Conv2d(k = s = p)'s gather, by torch's permute"""
    B, C, H, W = img.shape
    return img.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // p) * (W // p), C * p * p)


def from_patches(pat: torch.Tensor, B: int, C: int, H: int, W: int, p: int) -> torch.Tensor:
    """the inverse scatter: [B gy gx, C p p] -> [B, C, H, W]"""
    return pat.reshape(B, H // p, W // p, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


def dyadic(shape, seed: int) -> torch.Tensor:
    """multiples of 1/8 in [-4, 4]"""
    return torch.randint(-32, 33, shape, generator=torch.Generator().manual_seed(seed)).float() / 8.0


def pixel_loss_ref(pix: torch.Tensor, target: torch.Tensor, p: int, w_l1: float, w_l2: float, scale: float = 1.0, dt=None):
    """pix [M, C p p] f32 (patch layout), target [B, C, H, W] f32 -> fp64 (sums [2], dpix [M, C p p], bound of sums, bound of dpix).  The weights and
    1 / numel enter as the f32 values the kernel is given."""
    d = pix.double() - to_patches(target, p).double()
    sums = torch.stack([d.abs().sum(), (d * d).sum()])
    w1, w2 = float(torch.tensor(w_l1, dtype=F32)), float(torch.tensor(w_l2, dtype=F32))
    k = scale / d.numel()
    g = (w1 * torch.sign(d) + 2.0 * w2 * d) * k
    mag = (w1 * torch.sign(d).abs() + 2.0 * w2 * d.abs()) * k
    return sums, g, elem_bound(sums, sums, 1024), elem_bound(g, mag, 0, dt)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------------
def ln_ref(x, w, b, dy=None, dres=None, old=None, dt=None, eps: float = LN_EPS):
    """fp64 LayerNorm forward (and backward when dy is given) of f32 / 16-bit operands; `old` = (dw, db, dx_colsum) the kernel adds into.
    Returns a dict name -> (reference, bound); the 16-bit outputs' bounds use the format `dt`."""
    xd, wd, bd = x.double(), w.double(), b.double()
    M, D = xd.shape
    mean = xd.mean(1, keepdim=True)
    d = xd - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = d * rstd
    y = xh * wd + bd
    b_mean = elem_bound(mean, xd.abs().mean(1, keepdim=True), D)
    e_d = EPS24 * (xd.abs() + mean.abs()) + b_mean
    b_var = (2 * D + 8) * EPS24 * var + (2 * d.abs() * e_d).mean(1, keepdim=True)
    b_rstd = 0.5 * rstd ** 3 * b_var + 8 * EPS24 * rstd
    mag_y = wd.abs() * xh.abs() + bd.abs()
    out = dict(mean=(mean.squeeze(1), b_mean.squeeze(1)), rstd=(rstd.squeeze(1), b_rstd.squeeze(1)),
               y32=(y, wd.abs() * (rstd * e_d + d.abs() * b_rstd) + 8 * EPS24 * mag_y), y16=(y, elem_bound(y, mag_y, 0, dt)))
    if dy is None:
        return out
    dyd = dy.double()
    r = torch.zeros(M, D, dtype=F64) if dres is None else dres.double()
    o = [torch.zeros(D, dtype=F64)] * 3 if old is None else [t.double() for t in old]
    g = wd * dyd
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) + r
    mag_dx = rstd * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)) + r.abs()
    dw, db, dxs = (dyd * xh).sum(0), dyd.sum(0), dx.sum(0)
    out.update(dx=(dx, elem_bound(dx, mag_dx, D)), dx16=(dx, elem_bound(dx, mag_dx, D, dt)),
               dw=(dw + o[0], elem_bound(dw, (dyd.abs() * xh.abs()).sum(0) + o[0].abs(), D + M)),
               db=(db + o[1], elem_bound(db, dyd.abs().sum(0) + o[1].abs(), M)),
               dx_colsum=(dxs + o[2], elem_bound(dxs, mag_dx.sum(0) + o[2].abs(), 3 * D + M)))
    return out


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------------------------------
def f32v(x: float) -> float:
    """the value of x after its trip through a C float argument"""
    return float(torch.tensor(x, dtype=F32))


class TorchAdamW:
    """torch.optim.AdamW on the CPU in `dtype` over one tensor; step(g, t) feeds the f32 gradient g and takes step number t (the bias corrections are
    those of t, whatever was taken before: the kernel's `step` argument).  The hyper-parameters enter as the f32 values the C ABI carries (0.9f is
    0.9 (1 - 2.6e-8), so 1 - beta1 is 0.1 (1 + 2.4e-7): the kernel is held to the numbers it is given, like every other operand here)."""

    def __init__(self, p0: torch.Tensor, dtype, lr: float, wd: float, betas=(0.9, 0.99), eps: float = 1e-8):
        lr, wd, eps, betas = f32v(lr), f32v(wd), f32v(eps), (f32v(betas[0]), f32v(betas[1]))
        self.q = torch.nn.Parameter(p0.detach().cpu().to(dtype).clone())
        self.opt = torch.optim.AdamW([self.q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
        self.dtype = dtype

    def step(self, g: torch.Tensor, t: int):
        self.q.grad = g.detach().cpu().to(self.dtype)
        st = self.opt.state[self.q]
        if "step" in st:
            st["step"].fill_(t - 1)
        else:
            assert t == 1
        self.opt.step()
        return self

    def p(self):
        return self.q.detach()

    def m(self):
        return self.opt.state[self.q]["exp_avg"]

    def v(self):
        return self.opt.state[self.q]["exp_avg_sq"]


def adamw_check(dev, f32: TorchAdamW, ref: TorchAdamW, what: str, keep=None):
    """check_limit for p, m and v (dev = (p, m, v)); keep: optional boolean mask — the limit applied to that subset as a tensor of its own (a few
    huge parameters otherwise set the f32 run's worst element error for everyone).  Returns the largest error / limit."""
    worst = 0.0
    for name, d, a, r in zip("pmv", dev, (f32.p(), f32.m(), f32.v()), (ref.p(), ref.m(), ref.v())):
        d = d.detach().cpu()
        worst = max(worst, *check_limit(d, a, r, f"{what} {name}"))
        if keep is not None and bool(keep.any()) and not bool(keep.all()):
            worst = max(worst, *check_limit(d[keep], a[keep], r[keep], f"{what} {name} (ordinary parameters)"))
    return worst


# ---- enh_gemm_f32 -----------------------------------------------------------------------------------------------------------------------------------------
def gemm_f32_ref(A, B, bias=None, act: str = "none", aux=None, res=None, res_rows: int = 0, old=None):
    """A [M, K], B [N, K] (logical, whatever the storage layout): fp64 epilogue(A B^T) and its element bound.  act: none | tanh | dtanh (aux = h);
    res [res_rows, N] is added to row m from row m % res_rows; old: what C held, added when the call accumulates."""
    Ad, Bd = A.double(), B.double()
    M, K = Ad.shape
    v, mag, extra = Ad @ Bd.t(), Ad.abs() @ Bd.abs().t(), 0.0
    if bias is not None:
        v, mag = v + bias.double(), mag + bias.double().abs()
    if act == "tanh":
        v = torch.tanh(v)
        mag, extra = mag * (1 - v ** 2), TANH_ABS
    elif act == "dtanh":
        dfac = 1 - aux.double() ** 2
        v, mag = v * dfac, mag * dfac.abs()
    if res is not None:
        rr = res.double()[torch.arange(M) % res_rows]
        v, mag = v + rr, mag + rr.abs()
    if old is not None:
        v, mag = v + old.double(), mag + old.double().abs()
    return v, elem_bound(v, mag, K, extra_abs=extra)


def check(out, ref, bound, what: str) -> float:
    return assert_elementwise(out, ref, bound, what)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """same shape, dtype and bit pattern (NaNs and signed zeros included)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))
