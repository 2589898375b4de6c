"""fp64 references, element bounds and f32 emulations of the loss-network kernels (csrc/conv_igemm.hip, conv_pointwise.hip, disc_ops.hip, lpips_ops.hip),
shared by tests/test_loss_kernels_elementwise_gpu.py (the kernels) and tests/test_loss_kernels_metric_cpu.py (an f32 emulation and injected faults).

Every bound is DERIVED: from the unit roundoffs of the formats (util.U16, util.SUB16, 2^-24 for f32) and the operation counts of the formula, never from
what a kernel produced.  Layouts here are torch's (NCHW); the tests permute to and from the kernels' channels-last tensors."""
import functools

import torch
import torch.nn.functional as F

from util import SUB16, U16, elem_bound, h16r

BF16, F16 = torch.bfloat16, torch.float16
E24 = 2.0 ** -24                                                   # unit roundoff of f32
SLOPE, ACT_SCALE, ALPHA = 0.2, 2 ** 0.5, 2 ** -0.5                 # FusedLeakyReLU's constants, the residual merge of a StyleBlock
VGG_SHIFT = torch.tensor([-.030, -.088, -.188])                    # lpips' ScalingLayer
VGG_SCALE = torch.tensor([.458, .448, .450])
LPIPS_EPS = float(torch.tensor(1e-10, dtype=torch.float32))        # the kernels' 1e-10f


def f32(v: float) -> float:
    """the value a Python float has once it is passed to a kernel as a C float"""
    return float(torch.tensor(v, dtype=torch.float32))


def packed_weight(w, scale, dt):
    """what conv_pack_weight hands to the MFMA, as f32.  bf16: the f32 product scale * w rounded to bf16.  fp16: the EXACT product rounded once (the
    compiler fuses the multiply into the conversion, one v_fma_mixlo_f16) — it differs from h16r(w * scale, fp16) by one ulp where the f32 product lands on
    an fp16 tie, about one weight in 8192.  numpy converts float64 to float16 directly (torch goes through f32), and the product of two f32 is exact in
    float64.  test_packed_weights_match_their_cpu_model compares the device with this bit for bit."""
    if dt == F16:
        import numpy as np
        return torch.from_numpy((w.numpy().astype(np.float64) * np.float64(np.float32(scale))).astype(np.float16)).float()
    return h16r(w * scale, dt)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def r16(x, dt):
    """one rounding of an fp64 / f32 tensor to `dt`, as float64"""
    return x.to(dt).double()


# ---------------------------------------------------------------------------------------------
# convolutions and their epilogues
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, Cin, Cout, k, s, p, dt):
    """operands (exactly representable in dt), the fp64 convolution `pre` without epilogue and the same on absolute values (`mag`), computed once per
    shape and format.  ws = packed_weight(w, scale, dt): what the pack kernel hands to the MFMA."""
    g = torch.Generator().manual_seed(1000 * Cin + Cout + 7 * H + (dt == F16))
    x = h16r(torch.randn(B, Cin, H, W, generator=g), dt)
    w = torch.randn(Cout, Cin, k, k, generator=g)
    scale = 1.0 / (Cin * k * k) ** 0.5
    ws = packed_weight(w, scale, dt)
    pre = F.conv2d(x.double(), ws.double(), stride=s, padding=p)
    mag = F.conv2d(x.double().abs(), ws.double().abs(), stride=s, padding=p)
    bias = torch.randn(Cout, generator=g)
    add = h16r(torch.randn(pre.shape, generator=g), dt)
    aux = h16r(torch.randn(pre.shape, generator=g), dt).clamp_min(0)         # a post-ReLU activation: about half of it exact zeros
    return dict(x=x, w=w, scale=scale, ws=ws, pre=pre, mag=mag, bias=bias, add=add, aux=aux, kk=Cin * k * k, geom=(B, H, W, Cin, Cout, k, s, p), dt=dt)


def special_values(dt):
    """+0, -0, the smallest positive and negative subnormal, the smallest normal of either sign, as a dt tensor (from their bit patterns)"""
    nrm = 0x0080 if dt == BF16 else 0x0400
    bits = [0x0000, 0x8000, 0x0001, 0x8001, nrm, 0x8000 | nrm]
    return torch.tensor([b - 0x10000 if b >= 0x8000 else b for b in bits], dtype=torch.int16).view(dt)


def crafted_aux(aux, dt):
    """`aux` (NCHW f32, post-ReLU) with its first output row (b = 0, y = 0) replaced by the six special values in turn; returned as a dt tensor, since
    the expected mask is `aux > 0` as torch evaluates it on the CPU in that format"""
    a = aux.to(dt).clone()
    sp = special_values(dt)
    C, Wd = a.shape[1], a.shape[3]
    idx = (torch.arange(C)[:, None] + torch.arange(Wd)[None, :]) % 6
    a[0, :, 0, :] = sp[idx]
    return a


def epilogue_ref(case, mode, bias=None, add=None, aux_dt=None, p0=0.0, p1=1.0):
    """fp64 result of epilogue `mode` of conv_igemm.hip on the case's convolution and its element bound.
    mode 0 relu(acc + bias) and mode 3 lrelu(acc + bias, p0) * p1: both maps have Lipschitz constant <= 1 (times p1), so an error of the pre-activation
    passes through at most unchanged, a sign that differs between f32 and fp64 included: the magnitude is NOT multiplied by the gate.
    mode 1 (acc + add) * (aux > 0): the mask is exact (a comparison of a stored value), so reference and magnitude are masked alike.
    mode 4 acc + p0 * add.  p0 / p1 enter the reference with the values they have as C floats."""
    pre, mag, dt, k = case["pre"], case["mag"], case["dt"], case["kk"]
    b = bias.double().view(1, -1, 1, 1) if bias is not None else torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    if mode == 0:
        ref, m = F.relu(pre + b), mag + b.abs()
    elif mode == 1:
        keep = (aux_dt > 0).double()
        a = add.double() if add is not None else torch.zeros_like(pre)
        ref, m = (pre + a) * keep, (mag + a.abs()) * keep
    elif mode == 2:
        ref, m = pre, mag
    elif mode == 3:
        ref, m = F.leaky_relu(pre + b, f32(p0)) * f32(p1), (mag + b.abs()) * f32(p1)
    elif mode == 4:
        ref, m = pre + f32(p0) * add.double(), mag + (f32(p0) * add.double()).abs()
    else:
        raise ValueError(mode)
    return ref, elem_bound(ref, m, k, dt)


def epilogue_emulated(case, mode, bias=None, add=None, aux_dt=None, p0=0.0, p1=1.0):
    """the kernel's arithmetic in torch on the CPU: f32 convolution, the epilogue in f32, ONE rounding to dt (returned as f32)"""
    B, H, W, Cin, Cout, k, s, p = case["geom"]
    acc = F.conv2d(case["x"], case["ws"], stride=s, padding=p)
    b = bias.view(1, -1, 1, 1) if bias is not None else 0.0
    if mode == 0:
        v = F.relu(acc + b)
    elif mode == 1:
        v = torch.where(aux_dt > 0, acc + (add if add is not None else 0.0), torch.zeros_like(acc))
    elif mode == 2:
        v = acc
    elif mode == 3:
        a = acc + b
        v = torch.where(a > 0, a, a * torch.tensor(p0, dtype=torch.float32)) * torch.tensor(p1, dtype=torch.float32)
    else:
        v = acc + torch.tensor(p0, dtype=torch.float32) * add
    return h16r(v, case["dt"])


def conv_grads64(x, ws, g, s, p):
    """fp64 input and weight gradient of conv2d(x, ws) under the upstream gradient g, and the same two contractions on absolute values"""
    xr, wr = x.double().requires_grad_(True), ws.double().requires_grad_(True)
    F.conv2d(xr, wr, stride=s, padding=p).backward(g.double())
    xa, wa = x.double().abs().requires_grad_(True), ws.double().abs().requires_grad_(True)
    F.conv2d(xa, wa, stride=s, padding=p).backward(g.double().abs())
    return xr.grad, wr.grad, xa.grad, wa.grad


# ---------------------------------------------------------------------------------------------
# LPIPS: first VGG convolution, max-pool, head
# ---------------------------------------------------------------------------------------------
def vgg_scaled(img64, normalize: bool):
    a, b = (2.0, -1.0) if normalize else (1.0, 0.0)
    return ((a * img64 + b) - VGG_SHIFT.double().view(1, 3, 1, 1)) / VGG_SCALE.double().view(1, 3, 1, 1)


@functools.lru_cache(maxsize=None)
def vgg_conv1_case(B, H, W, normalize, dt):
    """image (f32), weights and bias (f32: the kernel reads them as they are), an upstream gradient representable in dt; fp64 forward, backward, bounds.
    forward : relu(conv(scaled x, w) + bias) rounded once: elem_bound(ref, conv(|scaled x|, |w|) + |bias|, 27 + 4, dt); the + 4: the scaling's own
              multiply-add, subtraction, reciprocal and product, each one f32 rounding of a factor of every product
    backward: (a / scale_ci) * sum over 9 taps x 64 channels in f32: elem_bound(ref, mag, 9 * 64), the positive factor on reference and magnitude"""
    g = torch.Generator().manual_seed(B * 100 + H + (dt == F16))
    img = torch.rand(B, 3, H, W, generator=g) if normalize else torch.rand(B, 3, H, W, generator=g) * 2 - 1
    w, bias = torch.randn(64, 3, 3, 3, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1
    gpre = h16r(torch.randn(B, 64, H, W, generator=g), dt)
    it = img.double().requires_grad_(True)
    pre = F.conv2d(vgg_scaled(it, normalize), w.double(), bias.double(), padding=1)
    pre.backward(gpre.double())
    ia = img.double().requires_grad_(True)
    F.conv2d(vgg_scaled(ia, normalize), w.double().abs(), padding=1).backward(gpre.double().abs())
    ref = F.relu(pre.detach())
    mag = F.conv2d(vgg_scaled(img.double(), normalize).abs(), w.double().abs(), padding=1) + bias.double().abs().view(1, -1, 1, 1)
    return dict(img=img, w=w, bias=bias, gpre=gpre, ref=ref, bound=elem_bound(ref, mag, 27 + 4, dt), dimg=it.grad, dimg_bound=elem_bound(it.grad, ia.grad, 9 * 64))


def vgg_conv1_emulated(c, normalize, dt, swap_hw=False):
    """f32 torch restatement of vgg_conv1_fwd_kernel; swap_hw: the fault "H and W swapped in the pixel decomposition" (pixel index hw split as
    (hw / H, hw % H) instead of (hw / W, hw % W): the outputs of each image land where the transposed raster puts them)"""
    a, b = (2.0, -1.0) if normalize else (1.0, 0.0)
    xs = ((a * c["img"] + b) - VGG_SHIFT.view(1, 3, 1, 1)) * (1.0 / VGG_SCALE).view(1, 3, 1, 1)
    y = h16r(F.relu(F.conv2d(xs, c["w"], c["bias"], padding=1)), dt)
    if swap_hw:
        Bn, Cn, H, W = y.shape
        y = y.transpose(2, 3).reshape(Bn, Cn, H, W)      # element hw of the raster is computed for pixel (hw / H, hw % H) of the W x H transposed image
    return y


def maxpool_case(dt, B=2, H=8, W=12, C=64):
    """post-ReLU input whose first channel group (channels 0..7) has a POSITIVE tie in every 2 x 2 window, random data in the other channels:
    window w of the group ties (first, second), (first, last), all four, (second, third) in turn; every other entry of the window is smaller and positive"""
    g = torch.Generator().manual_seed(17 + (dt == F16))
    x = h16r(torch.randn(B, C, H, W, generator=g), dt).clamp_min(0)
    pats = [(0, 1), (0, 3), (0, 1, 2, 3), (1, 2)]
    n = 0
    for b in range(B):
        for c in range(8):
            for ho in range(H // 2):
                for wo in range(W // 2):
                    top = 1.0 + 0.125 * ((n * 5) % 8)                      # representable in both formats
                    win = torch.full((4,), top / 4)
                    win[list(pats[n % 4])] = top
                    x[b, c, 2 * ho:2 * ho + 2, 2 * wo:2 * wo + 2] = win.view(2, 2)
                    n += 1
    gy = h16r(torch.randn(B, C, H // 2, W // 2, generator=g), dt)
    add = h16r(torch.randn(B, C, H, W, generator=g), dt)
    return x, gy, add


def positive_ties(x):
    """number of 2 x 2 windows whose maximum is positive and attained more than once"""
    win = F.unfold(x.reshape(-1, 1, *x.shape[2:]), 2, stride=2)            # [B*C, 4, windows]
    m = win.max(dim=1, keepdim=True).values
    return int(((m > 0) & ((win == m).sum(1, keepdim=True) > 1)).sum())


def maxpool_backward_ref(x, gy, add, dt, last=False):
    """F.max_pool2d's autograd (torch routes a tie to the FIRST maximum in scan order) + add, masked by x > 0, rounded once.
    last: the fault "tie routed to the last maximum" (the same on the window flipped in both axes)"""
    xt = x.double().clone().requires_grad_(True)
    if last:
        B, C, H, W = x.shape
        v = xt.view(B, C, H // 2, 2, W // 2, 2).flip(3, 5).reshape(B, C, H, W)
        F.max_pool2d(v, 2, 2).backward(gy.double())
    else:
        F.max_pool2d(xt, 2, 2).backward(gy.double())
    t = xt.grad + (add.double() if add is not None else 0.0)
    return (t * (x > 0)).to(dt)


def lpips_head_case(B, h, w, C, dt):
    """features [2B, C, h, w] (post-ReLU, representable in dt; images 0..B-1 the inputs, B..2B-1 the reconstructions), lin >= 0, gout.  Pixel 0 of image 0
    has an all-zero f0, pixel 1 an all-zero f1, pixel 2 both."""
    g = torch.Generator().manual_seed(C + h + (dt == F16))
    f = h16r(torch.randn(2 * B, C, h, w, generator=g).clamp_min(0), dt)
    f[0, :, 0, 0] = 0
    f[B, :, 0, 1] = 0
    f[0, :, 0, 2] = 0
    f[B, :, 0, 2] = 0
    lin = torch.rand(C, generator=g)
    gout = torch.randn(B, generator=g)
    return f, lin, gout


def lpips_head_ref(f, lin, B):
    """fp64 val [B, h, w], out [B] and their bounds.

    val_p = sum_c lin_c (n0_c - n1_c)^2, n = f / (||f|| + eps).  In f32: ||f||^2 is a sum of C squares (relative error C 2^-24 in any order), the square
    root halves it and adds its own rounding (<= 2 ulp allowed), then + eps, the reciprocal (<= 2 ulp) and the product f * i: every n_c carries
    e_n = (C / 2 + 6) 2^-24 relative.  u = n0 - n1: |du| <= (e_n + 2^-24) (|n0| + |n1|).  lin u^2: 2 |u| |du| <= 2 (e_n + 2^-24) (|n0| + |n1|)^2, two
    more roundings (lin * u, the fma) and the sum over C terms (C 2^-24):   (2 (C / 2 + 7) + 2 + C) 2^-24 = (2 C + 16) 2^-24   times
    sum_c |lin_c| (|n0_c| + |n1_c|)^2 — the issue's estimate, confirmed.
    out_b = mean_p val_p: the per-pixel bounds averaged plus an f32 sum of HW terms, (HW + 4) 2^-24 mean |val|."""
    C = f.shape[1]
    f0, f1 = f[:B].double(), f[B:].double()
    n0 = f0 / (f0.norm(dim=1, keepdim=True) + LPIPS_EPS)
    n1 = f1 / (f1.norm(dim=1, keepdim=True) + LPIPS_EPS)
    l = lin.double().view(1, C, 1, 1)
    val = (l * (n0 - n1) ** 2).sum(1)
    vb = (2 * C + 16) * E24 * (l.abs() * (n0.abs() + n1.abs()) ** 2).sum(1)
    HW = val.shape[1] * val.shape[2]
    out = val.mean((1, 2))
    ob = vb.mean((1, 2)) + (HW + 4) * E24 * val.abs().mean((1, 2))
    return val, vb, out, ob


def lpips_head_emulated(f, lin, B):
    """f32 restatement of lpips_head_fwd_kernel + lpips_head_reduce_kernel: val [B, h, w], out [B]"""
    C = f.shape[1]
    f0, f1 = f[:B], f[B:]
    i0 = 1.0 / (f0.square().sum(1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32))
    i1 = 1.0 / (f1.square().sum(1, keepdim=True).sqrt() + torch.tensor(1e-10, dtype=torch.float32))
    u = f0 * i0 - f1 * i1
    val = (lin.view(1, C, 1, 1) * u * u).sum(1)
    return val, val.sum((1, 2)) / (val.shape[1] * val.shape[2])


def lpips_head_backward_ref(f, lin, gout, B, dt):
    """fp64 gradient with respect to f1 by the ANALYTIC formula of lpips_head_bwd_kernel's header and its element bound:

        u = n0 - n1;  g_c = -2 lin_c u_c gout_b / HW;  df1_k = g_k i1 - (sum_c g_c f1_c) f1_k i1^2 / ||f1||,  the second term 0 where ||f1|| = 0

    (i1 = 1 / (||f1|| + eps): the exact derivative of f / (||f|| + eps)).  torch's autograd of the same expression returns NaN at ||f1|| = 0 (the backward
    of sqrt at 0 is inf, times a zero gradient); the kernel documents 0 for that term, and at such a pixel df1_k = g_k * 1e10 — finite in bf16, beyond
    fp16's range, where the correctly rounded result is +-inf.

    Bound: u(dt) |ref| + sub(dt) + an f32 term on the CANCELLING pair, with hatted magnitudes gh_c = 2 |lin_c| |go| (|n0_c| + |n1_c|) >= |g_c|,
    Dh = sum_c gh_c |f1_c| >= |dot|, Kh = Dh i1^2 / ||f1||:
        e_n = (C/2 + 6) 2^-24 (lpips_head_ref)           e_g = e_n + 6 2^-24 (the subtraction, -2 * lin * u * go, go = gout / HW)
        e_d = e_g + C 2^-24 (the sum over C)             e_k = e_d + 3 e_n + 3 2^-24 (i1, i1, 1 / n1 and three operations)
        |err| <= (e_g + e_n + 2 2^-24) gh_k i1 + (e_k + 2 2^-24) Kh |f1_k|
    Returns ref, bound, and the mask of pixels with ||f1|| > 0."""
    C = f.shape[1]
    HW = f.shape[2] * f.shape[3]
    f0, f1 = f[:B].double(), f[B:].double()
    nn1 = f1.norm(dim=1, keepdim=True)
    i0, i1 = 1.0 / (f0.norm(dim=1, keepdim=True) + LPIPS_EPS), 1.0 / (nn1 + LPIPS_EPS)
    l = lin.double().view(1, C, 1, 1)
    go = (gout.double() / HW).view(B, 1, 1, 1)
    n0, n1 = f0 * i0, f1 * i1
    gq = -2 * l * (n0 - n1) * go
    dot = (gq * f1).sum(1, keepdim=True)
    live = nn1 > 0
    k2 = torch.where(live, dot * i1 * i1 / nn1.clamp_min(1e-300), torch.zeros_like(dot))
    ref = gq * i1 - k2 * f1
    gh = 2 * l.abs() * go.abs() * (n0.abs() + n1.abs())
    Kh = torch.where(live, (gh * f1.abs()).sum(1, keepdim=True) * i1 * i1 / nn1.clamp_min(1e-300), torch.zeros_like(dot))
    e_n = (C / 2 + 6) * E24
    e_g = e_n + 6 * E24
    e_k = e_g + C * E24 + 3 * e_n + 3 * E24
    bound = U16[dt] * ref.abs() + SUB16.get(dt, 0.0) + (e_g + e_n + 2 * E24) * gh * i1 + (e_k + 2 * E24) * Kh * f1.abs()
    return ref, bound, live.expand_as(ref)


def lpips_head_backward_autograd(f, lin, gout, B):
    """torch autograd of the same expression in fp64 (NaN where ||f1|| = 0)"""
    C = f.shape[1]
    f0, f1 = f[:B].double(), f[B:].double().clone().requires_grad_(True)
    n0 = f0 / (f0.norm(dim=1, keepdim=True) + LPIPS_EPS)
    n1 = f1 / (f1.square().sum(1, keepdim=True).sqrt() + LPIPS_EPS)
    val = (lin.double().view(1, C, 1, 1) * (n0 - n1) ** 2).sum(1).mean((1, 2))
    (val * gout.double()).sum().backward()
    return f1.grad


def lpips_head_backward_emulated(f, lin, gout, B, dt):
    """f32 restatement of lpips_head_bwd_kernel, one rounding to dt"""
    C, HW = f.shape[1], f.shape[2] * f.shape[3]
    f0, f1 = f[:B], f[B:]
    eps = torch.tensor(1e-10, dtype=torch.float32)
    n1 = f1.square().sum(1, keepdim=True).sqrt()
    i0, i1 = 1.0 / (f0.square().sum(1, keepdim=True).sqrt() + eps), 1.0 / (n1 + eps)
    go = (gout / HW).view(B, 1, 1, 1)
    gq = -2.0 * lin.view(1, C, 1, 1) * (f0 * i0 - f1 * i1) * go
    dot = (gq * f1).sum(1, keepdim=True)
    k2 = torch.where(n1 > 0, dot * i1 * i1 / n1.clamp_min(1e-30), torch.zeros_like(dot))
    return h16r(gq * i1 - k2 * f1, dt)


# ---------------------------------------------------------------------------------------------
# blur and minibatch standard deviation
# ---------------------------------------------------------------------------------------------
def blur_kernel4():
    """the asymmetric 4 x 4 kernel of tests/test_conv_nhwc_gpu.py (asymmetric, so that the flip conventions are tested)"""
    k1 = torch.tensor([1., 3., 3., 1.])
    kern = k1[None, :] * k1[:, None]
    kern = kern / kern.sum()
    kern[0, 1] += 0.01
    return kern


def blur64(x, kern, pad, flip=False):
    """upfirdn2d(x, kern, pad) with unit up / down factors in the dtype of x (NCHW): out[oy, ox] = sum_ij kern[kh-1-i][kw-1-j] xpad[oy + i, ox + j], a true
    convolution; flip: the adjoint's tap order kern[i][j]"""
    C = x.shape[1]
    k = kern.to(x.dtype)
    wgt = (k if flip else k.flip(0, 1))[None, None].expand(C, 1, *k.shape).contiguous()
    return F.conv2d(F.pad(x, (pad[0], pad[1], pad[0], pad[1])), wgt, groups=C)


def blur_case(shape, pad, dt, kern):
    """x [B, H, W, C] (channels-last shape as the kernel sees it); fp64 forward and adjoint with elem_bound(ref, blur(|x|, |k|), taps, dt)"""
    g = torch.Generator().manual_seed(shape[1] * 10 + pad[0] + (dt == F16))
    B, H, W, C = shape
    x = h16r(torch.randn(B, C, H, W, generator=g), dt)
    n = kern.numel()
    xr = x.double().requires_grad_(True)
    y = blur64(xr, kern, pad)
    gy = h16r(torch.randn(y.shape, generator=g), dt)
    y.backward(gy.double())
    xa = x.double().abs().requires_grad_(True)
    ya = blur64(xa, kern.abs(), pad)
    ya.backward(gy.double().abs())
    return dict(x=x, gy=gy, y=y.detach(), y_bound=elem_bound(y.detach(), ya.detach(), n, dt), dx=xr.grad, dx_bound=elem_bound(xr.grad, xa.grad, n, dt))


def stddev_case(B, group, C, dt, identical_slot=None, HW=16):
    """x [B, HW, C] and an upstream gradient [B, HW, Cp] representable in dt (flattened channels-last: the statistic does not see the layout);
    identical_slot: the samples of that slot are made identical (variance 0 at every position)"""
    g = torch.Generator().manual_seed(B * 31 + C + (dt == F16))
    x = h16r(torch.randn(B, HW, C, generator=g), dt)
    n = B // group
    if identical_slot is not None:
        for gi in range(group):
            x[gi * n + identical_slot] = x[identical_slot]
    gy = h16r(torch.randn(B, HW, pad8(C + 1), generator=g), dt)
    return x, gy


def stddev_ref(x, gy, group, dt):
    """Minibatch standard deviation as the reference project defines it (its StyleDiscriminator.forward, stddev_feat = 1), restated in fp64 on [B, HW, C]:
    sample b belongs to slot b % (B / group); per position the BIASED variance over the slot's `group` samples; sd = sqrt(var + 1e-8); the statistic of
    a slot is the mean of sd over all HW * C positions.  Backward: dx = g + gsd * (x - m) / (group * sd), gsd = (sum of the slot's g[..., C]) / (HW C).

    Returns stat [B], its bound, dx [B, HW, C], its bound.  With P = HW C, mean|x| the mean of |x| over the group at a position:
      m = sum / group in f32 carries dm = (group + 1) 2^-24 mean|x|  (it does NOT shrink with x - m: that is how the cancellation in d = x - m enters;
          |d(d)| <= dm + 2^-24 |d|);
      var = mean d^2: |d var| <= 2 dm mean|d| + (group + 4) 2^-24 var, mean|d| <= sd, so |d sd| <= dm + (group / 2 + 4) 2^-24 sd (sqrt and + eps included);
      stat: one rounding to dt + mean_p |d sd_p| + (P + 8) 2^-24 stat (an f32 sum of P positive terms in any order, the division);
      dx = g + coef d, coef = gsd / (group sd): gsd carries (group HW + 4) 2^-24 on gsd_abs = sum|g_C| / P;
          |err| <= u |ref| + sub + 4 2^-24 (|g| + |coef| |d|) + |coef| dm + |d| (coef_abs (group HW + group + 16) 2^-24 + |coef| dm / sd)."""
    B, HW, C = x.shape
    n = B // group
    P = HW * C
    eps = f32(1e-8)
    xg = x.double().view(group, n, HW, C)                       # sample gi * n + slot
    m = xg.mean(0, keepdim=True)
    d = xg - m
    sd = (d.square().mean(0, keepdim=True) + eps).sqrt()        # [1, n, HW, C]
    dm = (group + 1) * E24 * xg.abs().mean(0, keepdim=True)
    stat_slot = sd.mean((2, 3)).view(n)
    dsd = dm + (group / 2 + 4) * E24 * sd
    stat_b_slot = dsd.mean((2, 3)).view(n) + (P + 8) * E24 * stat_slot
    stat = stat_slot.repeat(group)
    stat_bound = U16[dt] * stat.abs() + SUB16.get(dt, 0.0) + stat_b_slot.repeat(group)
    gC = gy.double()[..., C].view(group, n, HW)
    gsd = (gC.sum((0, 2)) / P).view(1, n, 1, 1)
    gsd_abs = (gC.abs().sum((0, 2)) / P).view(1, n, 1, 1)
    coef, coef_abs = gsd / (group * sd), gsd_abs / (group * sd)
    gx = gy.double()[..., :C].view(group, n, HW, C)
    dx = gx + coef * d
    f32t = 4 * E24 * (gx.abs() + coef.abs() * d.abs()) + coef.abs() * dm + d.abs() * (coef_abs * (group * HW + group + 16) * E24 + coef.abs() * dm / sd)
    dx_bound = U16[dt] * dx.abs() + SUB16.get(dt, 0.0) + f32t
    return stat, stat_bound, dx.reshape(B, HW, C), dx_bound.reshape(B, HW, C)


def stddev_emulated(x, gy, group, dt):
    """f32 restatement of stddev_fwd_kernel / stddev_bwd_kernel: stat [B] and dx [B, HW, C], one rounding to dt each"""
    B, HW, C = x.shape
    n, P = B // group, HW * C
    xg = x.view(group, n, HW, C)
    m = xg.sum(0, keepdim=True) / group
    d = xg - m
    sd = ((d * d).sum(0, keepdim=True) / group + torch.tensor(1e-8, dtype=torch.float32)).sqrt()
    stat = (sd.sum((2, 3)) / P).view(n).repeat(group)
    gsd = (gy[..., C].view(group, n, HW).sum((0, 2)) / P).view(1, n, 1, 1)
    dx = gy[..., :C].view(group, n, HW, C) + (gsd / (group * sd)) * d
    return h16r(stat, dt), h16r(dx.reshape(B, HW, C), dt)


# ---------------------------------------------------------------------------------------------
# the Cauchy-Schwarz magnitude of a convolution (no second fp64 convolution at real layer sizes)
# ---------------------------------------------------------------------------------------------
def conv_mag_upper(x, ws, k, s, p):
    """an upper bound of conv(|x|, |ws|) [B, Cout, Ho, Wo] without a convolution over channels:
        sum_{tap, c} |x| |w| <= sqrt(sum_{tap, c} x^2 over the patch) * ||w_co||_2        (Cauchy-Schwarz over the patch)
    = sqrt(box filter (k x k, stride s, padding p) of the channel sum of x^2) times the weight-row norms"""
    sq = x.double().square().sum(1, keepdim=True)
    box = F.conv2d(sq, torch.ones(1, 1, k, k, dtype=torch.float64), stride=s, padding=p)
    return box.sqrt() * ws.double().flatten(1).norm(dim=1).view(1, -1, 1, 1)
