"""The loss networks' 16-bit kernels at their REAL layer sizes, in both operand formats, against float64 on the CPU, and fp16's range edges.

Every config with a GAN or LPIPS term runs the StyleGAN discriminator and the LPIPS VGG16 trunk on fp16 operands under a loss scale
(enhancing/losses/vqperceptual.py loss_operands); the op tests (test_conv_nhwc_gpu.py, test_lpips_gpu.py) stop at ~70 x 66 pixels.  Here:

  * the layer tables: every layer of StyleDiscriminator(size=256) at B = 2 and every LPIPS VGG16 op at 256 x 256 (two images), each compared with ONE
    float64 reference per layer and format, computed from operands that are exactly representable in that format (fp16 operands drawn at full fp16
    precision, not reused bf16 values), under every convolution family (auto, reg, t128, t256).  Tolerance classes of test_conv_nhwc_gpu.py: a 16-bit
    output rounded once <= 1.25 x its rounding floor; f32 weight gradients <= 2e-5, scaled with the square root of the longest f32 summation chain past
    the ~1e5 terms that bound was set for (see _wgrad_bound);
  * fp16 overflow: results past 65520 (the round-to-nearest-even threshold) must leave every packing kernel as +-inf exactly where the correctly rounded
    result is +-inf — no 65504, no NaN — and an inf in the upstream gradient must make the f32 weight gradient non-finite (LossScaler's found-inf);
  * fp16 subnormals: upstream gradients scaled so that >= 20 % of the correctly rounded nonzero outputs are subnormal; the error stays within 1.25 x the
    (subnormal-aware) floor and nothing is flushed to zero; and the fp16 floor of the LPIPS-head gradient at HW = 65536 over the loss scales the dynamic
    scaler visits (reported, not bounded).

Measured on MI355X (largest error / floor, bf16 | fp16, over this file and the op tests' fp16 twins):
  conv forward, all epilogues 1.000 | 1.005   dgrad 1.000 | 1.005   gate + dgrad (two roundings) 1.42 | 1.42   f32 wgrad 4.6e-7 | 7.0e-7 (absolute)
  blur + adjoint, stddev backward, conv3x3_nhwc modes 0 / 1 / 2, vgg_conv1, lpips_head backward 1.000 | 1.000   conv2d_gradfix dx 1.012 | 1.015
  fp16 overflow: 1.3 - 22 % of the outputs +-inf, the finite part <= 1.001; subnormals: 38 - 65 % of the nonzero outputs, every kernel 1.000, none
  flushed.  LPIPS head at HW = 65536: fp16 floor 2.2e-2 at 2^10, 5.4e-3 at 2^12, 1.35e-3 at 2^14, 3.6e-4 at 2^16 (bf16 1.66e-3 at every scale);
  subnormal share of the nonzero gradient 100 % up to 2^13, 82.5 % at 2^16.  Wall time of this file 22 - 42 s.
  A kernel trace of these tests lists the fp16 instance of every loss-network kernel: conv_igemm / conv_igemm_glds / conv_splitk_finish /
  conv_igemm_w256<F16, 4> / conv_igemm_w512 / conv_wgrad_w256<F16, false | true> / conv_wgrad_igemm / conv_pw_fwd | dgrad | wgrad /
  conv_pack_weight / blur4x4_nhwc<F16, 13 | 5> / blur_nhwc / lrelu_gate_h16 / img_to_nhwc8 / nhwc8_to_img / stddev_fwd | bwd / vgg_conv1_fwd | bwd /
  maxpool2_fwd | bwd / lpips_head_fwd | bwd<F16, 1 | 2 | 4 | 8>, and im2col / col2im<1>."""
import ctypes
import time

import pytest
import torch
import torch.nn.functional as F

from nonfinite_util import check_overflow, floor_bound, pow2_scale as _pow2_scale
from util import floor16, h16r, rel

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
FAMILIES = ["auto", "reg", "t128", "t256"]
SUB = 2.0 ** -14                 # smallest fp16 normal
ALPHA = 2 ** -0.5                # StyleBlock's residual merge


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from enhancing import _C
    from enhancing.losses.op import conv_nhwc
    _C.lib()
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))      # the fp64 references: at most 16 CPUs
    t0 = time.time()
    yield conv_nhwc
    torch.set_num_threads(threads)
    _C.conv_set_kernel("auto")
    print(f"\ntest_loss_layers_gpu wall time {time.time() - t0:.1f} s")


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.float().cpu().permute(0, 3, 1, 2).contiguous()


def _draw(shape, g, dt, scale=1.0, shift=0.0):
    """an operand exactly representable in dt, drawn at dt's full precision (and within fp16's finite range)"""
    return h16r((torch.randn(*shape, generator=g) * scale + shift).clamp(-65504.0, 65504.0), dt)


def _blur_kernel():
    k1 = torch.tensor([1., 3., 3., 1.])
    k = k1[None, :] * k1[:, None]
    return k / k.sum()


def _blur_ref(x64, kern, pad):
    """upfirdn2d with unit factors (the Blur of layers.py) in float64: zero padding, then correlation with the flipped kernel"""
    C = x64.shape[1]
    xp = F.pad(x64, (pad[0], pad[1], pad[0], pad[1]))
    return F.conv2d(xp, kern.flip(0, 1).double().view(1, 1, 4, 4).expand(C, 1, 4, 4).contiguous(), groups=C)


def _wgrad_bound(ops, B, H, W, Cp, Cout, k, s, p):
    """The f32 weight gradient: exact 16-bit products summed in f32 over n = B * Ho * Wo pixels.  Rounding errors of a sequential f32 sum grow like the
    square root of its length in rms; 2e-5 holds for chains of up to ~1e5 terms (test_conv_nhwc_gpu.py).  The split plan (enh_conv_wgrad_workspace_bytes:
    slices of the pixel axis summed separately, then added in a fixed order) only shortens the chains, so the unsplit length n is the worst case over
    the families; the plan is reported."""
    from enhancing import _C
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    n = B * Ho * Wo
    geom = dict(B=B, Hs=H, Ws=W, C=Cp, Hm=Ho, Wm=Wo, gs=s, oy0=-p, ox0=-p, nty=k, ntx=k, sty=1, stx=1, N=Cout, HO=Ho, WO=Wo, os=1, oph=0, opw=0)
    nb = _C.lib().enh_conv_wgrad_workspace_bytes(ctypes.byref(_C._geom(geom)))
    splits = max(1, nb // (4 * Cout * k * k * Cp))
    return 2e-5 * max(1.0, (n / 1e5) ** 0.5), n, splits


# ---------------------------------------------------------------------------------------------
# discriminator layer table: StyleDiscriminator(size=256), B = 2
# ---------------------------------------------------------------------------------------------
def _disc_layers():
    ch = {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128}
    rows = [("conv0 1x1 3->128 @256", "bias_lrelu", 256, 3, 128, 1, 1, 0)]
    H, cin = 256, 128
    while H > 4:
        cout = ch[H // 2]
        rows += [(f"b{H} conv1 3x3 {cin}->{cin}", "bias_lrelu", H, cin, cin, 3, 1, 1),
                 (f"b{H} blur(2,2) {cin}", "blur22", H, cin, cin, 4, 1, 2),
                 (f"b{H} conv2 3x3/2 {cin}->{cout}", "bias_lrelu", H + 1, cin, cout, 3, 2, 0),
                 (f"b{H} blur(1,1) {cin}", "blur11", H, cin, cin, 4, 1, 1),
                 (f"b{H} skip 1x1/2 {cin}->{cout} + merge", "add", H - 1, cin, cout, 1, 2, 0)]
        H, cin = H // 2, cout
    rows.append(("final 3x3 513(520)->512 @4", "bias_lrelu", 4, 513, 512, 3, 1, 1))
    return rows


DISC = _disc_layers()


@DTS
@pytest.mark.parametrize("layer", DISC, ids=[r[0] for r in DISC])
def test_discriminator_layer(ops, dt, layer):
    name, kind, H, Cin, Cout, k, s, p = layer
    B = 2
    g = torch.Generator().manual_seed(H * 1000 + Cin + Cout + (7 if dt == F16 else 0))
    if kind.startswith("blur"):
        return _disc_blur(ops, dt, name, B, H, Cin, (p, p))
    Cp = ops.pad8(Cin)
    x = _draw((B, Cin, H, H), g, dt)
    w = torch.randn(Cout, Cin, k, k, generator=g)
    scale = 1.0 / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    x64 = x.double()
    # forward reference: the fused epilogue (bias + leaky-ReLU * sqrt 2, or the residual merge with alpha folded into the packed weights)
    if kind == "bias_lrelu":
        ws = h16r(w * scale, dt)
        conv = F.conv2d(x64, ws.double(), stride=s, padding=p)
        y_ref = F.leaky_relu(conv + bias.double().view(1, -1, 1, 1), 0.2) * 2 ** 0.5
        add = None
    else:
        ws = h16r(w * (scale * ALPHA), dt)
        conv = F.conv2d(x64, ws.double(), stride=s, padding=p)
        add = _draw(conv.shape, g, dt)
        y_ref = conv + ALPHA * add.double()
    del conv
    # backward reference of the convolution triangle (plain conv: dgrad and wgrad kernels, upstream gradient in dt)
    wsp = h16r(w * scale, dt)
    Ho = y_ref.shape[2]
    dy = _draw((B, Cout, Ho, Ho), g, dt)
    xr, wr = x64.clone().requires_grad_(True), wsp.double().clone().requires_grad_(True)
    F.conv2d(xr, wr, stride=s, padding=p).backward(dy.double())
    dx_ref, dw_ref = xr.grad, scale * wr.grad
    del xr, wr
    f_y, f_x = floor16(y_ref, dt), floor16(dx_ref, dt)
    wb, n, splits = _wgrad_bound(ops, B, H, H, Cp, Cout, k, s, p)
    xp = torch.zeros(B, H, H, Cp, dtype=dt)
    xp[..., :Cin] = _nhwc(x).to(dt)
    xd_base = xp.cuda()
    wd = w.cuda()
    from enhancing import _C
    worst = [0.0, 0.0, 0.0]
    for fam in FAMILIES:
        _C.conv_set_kernel(fam)
        try:
            if kind == "bias_lrelu":
                y = ops.conv_bias_lrelu(xd_base, wd, bias.cuda(), scale, s, p)
            else:
                y = ops.conv_add(xd_base, wd, _nhwc(add).to(dt).cuda(), scale * ALPHA, s, p, ALPHA)
            xd, wdg = xd_base.clone().requires_grad_(True), wd.clone().requires_grad_(True)
            ops.conv(xd, wdg, scale, s, p).backward(_nhwc(dy).to(dt).cuda())
            torch.cuda.synchronize()
        finally:
            _C.conv_set_kernel("auto")
        e_y = rel(_nchw(y), y_ref) / f_y
        gx = _nchw(xd.grad)
        e_x = rel(gx[:, :Cin], dx_ref) / f_x
        e_w = rel(wdg.grad, dw_ref)
        print(f"disc {dt} {name} [{fam}]: y {e_y:.3f} x floor ({f_y:.2e}), dx {e_x:.3f} x floor ({f_x:.2e}), dw {e_w:.2e} "
              f"(bound {wb:.2e}: {n} pixels, {splits} slice(s))")
        assert e_y <= 1.25 and e_x <= 1.25 and e_w <= wb, (fam, e_y, e_x, e_w)
        if Cp > Cin:
            assert not gx[:, Cin:].abs().sum().item()
        worst = [max(worst[0], e_y), max(worst[1], e_x), max(worst[2], e_w)]
    print(f"disc {dt} {name}: worst y {worst[0]:.3f}, dx {worst[1]:.3f} x floor, dw {worst[2]:.2e}")


def _disc_blur(ops, dt, name, B, H, C, pad):
    g = torch.Generator().manual_seed(H + C + (7 if dt == F16 else 0))
    kern = _blur_kernel()
    x = _draw((B, C, H, H), g, dt)
    y_ref = _blur_ref(x.double(), kern, pad)
    gy = _draw(y_ref.shape, g, dt)
    # the adjoint: the same FIR with the kernel flipped and padding kh - 1 - pad (conv_nhwc._Blur.backward), i.e. a transposed correlation
    xr = x.double().clone().requires_grad_(True)
    _blur_ref(xr, kern, pad).backward(gy.double())
    xd = _nhwc(x).to(dt).cuda().requires_grad_(True)
    y = ops.blur(xd, kern.cuda(), pad)
    y.backward(_nhwc(gy).to(dt).cuda())
    e_y, e_x = rel(_nchw(y), y_ref) / floor16(y_ref, dt), rel(_nchw(xd.grad), xr.grad) / floor16(xr.grad, dt)
    print(f"disc {dt} {name}: blur {e_y:.3f} x floor, adjoint {e_x:.3f} x floor")
    assert e_y <= 1.25 and e_x <= 1.25


@DTS
@pytest.mark.parametrize("B,group", [(2, 2), (8, 4)])
def test_discriminator_stddev_layer(ops, dt, B, group):
    """minibatch stddev at 4 x 4 x 512 (group 2 at B = 2, group 4 at B = 8): copy bit-exact, the statistic rounded once, the backward at the floor"""
    g = torch.Generator().manual_seed(B + (7 if dt == F16 else 0))
    C = 512
    Cp = ops.pad8(C + 1)
    x = _draw((B, 4, 4, C), g, dt)
    xr = x.double().clone().requires_grad_(True)
    y_ref = ops._stddev_torch(xr, group, Cp)
    gy = _draw(y_ref.shape, g, dt)
    y_ref.backward(gy.double())
    xd = x.to(dt).cuda().requires_grad_(True)
    y = ops.minibatch_stddev(xd, group)
    assert torch.equal(y[..., :C].cpu(), x.to(dt)) and not y[..., C + 1:].float().abs().sum().item()
    stat, stat_ref = y[..., C].float().cpu(), y_ref[..., C].detach()
    e_s = rel(stat, stat_ref)
    y.backward(gy.to(dt).cuda())
    e_x = rel(xd.grad.float(), xr.grad) / floor16(xr.grad, dt)
    print(f"stddev {dt} B={B} group={group}: statistic {e_s:.2e} (floor {floor16(stat_ref, dt):.2e}), backward {e_x:.3f} x floor")
    assert e_s <= floor16(stat_ref, dt) + 1e-5       # one rounding of an f32 reduction over 8192 positions
    assert e_x <= 1.25


# ---------------------------------------------------------------------------------------------
# LPIPS layer table: VGG16 slices of enhancing/losses/lpips.py at 256 x 256, two images
# ---------------------------------------------------------------------------------------------
def _lpips_convs():
    from enhancing.losses.lpips import _SLICES
    rows, H = [], 256
    for k, convs in enumerate(_SLICES):
        for idx, cin, cout in convs:
            if idx:                     # conv 0 (3 -> 64) is vgg_conv1
                rows.append((f"slice{k + 1}.{idx} {cin}->{cout} @{H}", H, cin, cout))
        H //= 2
    return rows


LPIPS_CONVS = _lpips_convs()


@DTS
@pytest.mark.parametrize("layer", LPIPS_CONVS, ids=[r[0] for r in LPIPS_CONVS])
def test_lpips_conv3x3_layer(ops, dt, layer):
    """conv3x3_nhwc in mode 0 (bias + ReLU), 2 (input gradient) and 1 (input gradient + add, masked by aux > 0), every family"""
    from enhancing import _C
    name, H, Cin, Cout = layer
    B = 2
    g = torch.Generator().manual_seed(H + Cin + Cout + (7 if dt == F16 else 0))
    x = _draw((B, Cin, H, H), g, dt).clamp_min(0)
    w = _draw((Cout, Cin, 3, 3), g, dt, (2.0 / (9 * Cout)) ** 0.5)
    bias = torch.randn(Cout, generator=g) * 0.1
    y_ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), padding=1))
    gy = _draw((B, Cout, H, H), g, dt)
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), padding=1)
    aux, add = _draw((B, Cin, H, H), g, dt), _draw((B, Cin, H, H), g, dt)
    m1_ref = (dx_ref + add.double()) * (aux > 0)
    f0, f2, f1 = floor16(y_ref, dt), floor16(dx_ref, dt), floor16(m1_ref, dt)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).to(dt).cuda()
    wb = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).to(dt).cuda()
    xd, gyd, auxd, addd = (_nhwc(t).to(dt).cuda() for t in (x, gy, aux, add))
    for fam in FAMILIES:
        _C.conv_set_kernel(fam)
        try:
            out = torch.empty(B, H, H, Cout, dtype=dt, device="cuda")
            _C.conv3x3_nhwc(xd, wt, B, H, H, Cin, Cout, out, bias=bias.cuda(), mode=0)
            gx = torch.empty(B, H, H, Cin, dtype=dt, device="cuda")
            _C.conv3x3_nhwc(gyd, wb, B, H, H, Cout, Cin, gx, mode=2)
            gx1 = torch.empty(B, H, H, Cin, dtype=dt, device="cuda")
            _C.conv3x3_nhwc(gyd, wb, B, H, H, Cout, Cin, gx1, mode=1, aux=auxd, add=addd)
            torch.cuda.synchronize()
        finally:
            _C.conv_set_kernel("auto")
        e0, e2, e1 = rel(_nchw(out), y_ref) / f0, rel(_nchw(gx), dx_ref) / f2, rel(_nchw(gx1), m1_ref) / f1
        print(f"lpips {dt} {name} [{fam}]: mode 0 {e0:.3f}, mode 2 {e2:.3f}, mode 1 {e1:.3f} x floor")
        assert max(e0, e1, e2) <= 1.25, (fam, e0, e2, e1)


@DTS
def test_lpips_first_conv_and_pools(ops, dt):
    """vgg_conv1 forward / backward at 256 x 256 and the four 2 x 2 max-pools (256 -> 128 ... 32 -> 16) with their backward"""
    import lpips_oracle as LO
    from enhancing import _C
    g = torch.Generator().manual_seed(5 + (7 if dt == F16 else 0))
    B, H = 2, 256
    img = torch.rand(B, 3, H, H, generator=g)
    w, b = torch.randn(64, 3, 3, 3, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1
    sh, sc = LO.SHIFT.double(), LO.SCALE.double()
    it = img.double().clone().requires_grad_(True)
    pre = F.conv2d(((2 * it - 1) - sh) / sc, w.double(), b.double(), padding=1)
    y_ref = F.relu(pre)
    gpre = _draw(pre.shape, g, dt)
    pre.backward(gpre.double())
    out = torch.empty(B, H, H, 64, dtype=dt, device="cuda")
    _C.vgg_conv1(img.cuda(), w.cuda(), b.cuda(), LO.SHIFT.reshape(-1).cuda(), LO.SCALE.reshape(-1).cuda(), True, out)
    dimg = torch.empty(B, 3, H, H, device="cuda")
    _C.vgg_conv1_backward(_nhwc(gpre).to(dt).cuda(), w.cuda(), LO.SCALE.reshape(-1).cuda(), True, B, H, H, dimg)
    e_c, e_i = rel(_nchw(out), y_ref) / floor16(y_ref, dt), rel(dimg, it.grad)
    print(f"lpips {dt} vgg_conv1 @256: forward {e_c:.3f} x floor, image gradient {e_i:.2e}")
    assert e_c <= 1.25 and e_i <= 1e-5
    for Hp, C in ((256, 64), (128, 128), (64, 256), (32, 512)):
        x = _draw((B, C, Hp, Hp), g, dt).clamp_min(0)
        y = torch.empty(B, Hp // 2, Hp // 2, C, dtype=dt, device="cuda")
        _C.maxpool2_nhwc(_nhwc(x).to(dt).cuda(), B, Hp, Hp, C, y)
        assert torch.equal(_nchw(y), F.max_pool2d(x, 2, 2)), Hp
        gy, add = _draw((B, C, Hp // 2, Hp // 2), g, dt), _draw((B, C, Hp, Hp), g, dt)
        xt = x.double().clone().requires_grad_(True)
        F.max_pool2d(xt, 2, 2).backward(gy.double())
        want = ((xt.grad + add.double()) * (x > 0)).to(dt)          # one rounding of an exact sum
        gx = torch.empty(B, Hp, Hp, C, dtype=dt, device="cuda")
        _C.maxpool2_nhwc_backward(_nhwc(x).to(dt).cuda(), _nhwc(gy).to(dt).cuda(), _nhwc(add).to(dt).cuda(), B, Hp, Hp, C, gx)
        assert torch.equal(_nchw(gx).to(dt), want), Hp


def _head_ref(f, lin, B, gout):
    """LPIPS head of one slice in float64 (lpips_oracle.normalize_tensor): value per image and d value / d f1, f = [2B, C, h, w]"""
    import lpips_oracle as LO
    f64 = f.double()
    f1 = f64[B:].clone().requires_grad_(True)
    d = (LO.normalize_tensor(f64[:B]) - LO.normalize_tensor(f1)) ** 2
    val = (d * lin.double().view(1, -1, 1, 1)).sum(1).mean([1, 2])
    (val * gout.double()).sum().backward()
    return val.detach(), f1.grad


@DTS
@pytest.mark.parametrize("HW,C", [(256, 64), (128, 128), (64, 256), (32, 512), (16, 512)])
def test_lpips_head_layer(ops, dt, HW, C):
    from enhancing import _C
    g = torch.Generator().manual_seed(HW + C + (7 if dt == F16 else 0))
    B = 1
    f0 = torch.randn(B, C, HW, HW, generator=g).clamp_min(0)
    f = h16r(torch.cat([f0, (f0 + 0.3 * torch.randn(B, C, HW, HW, generator=g)).clamp_min(0)]), dt)
    lin = torch.rand(C, generator=g)
    gout = torch.randn(B, generator=g)
    val, df_ref = _head_ref(f, lin, B, gout)
    fd = _nhwc(f).to(dt).cuda()
    out, ws = torch.empty(B, device="cuda"), torch.empty(B * HW * HW, device="cuda")
    _C.lpips_head(fd, lin.cuda(), B, HW * HW, C, ws, out, False)
    df = torch.empty(B, HW, HW, C, dtype=dt, device="cuda")
    _C.lpips_head_backward(fd, lin.cuda(), gout.cuda(), B, HW * HW, C, df)
    e_v, e_d = rel(out, val), rel(_nchw(df), df_ref) / floor16(df_ref, dt)
    print(f"lpips {dt} head HW={HW}^2 C={C}: value {e_v:.2e}, gradient {e_d:.3f} x floor")
    assert e_v <= 1e-5 and e_d <= 1.25


# ---------------------------------------------------------------------------------------------
# fp16 overflow: +-inf exactly where the correctly rounded result is +-inf
# ---------------------------------------------------------------------------------------------
def _check_overflow(got, ref, what):
    """got: the kernel's fp16 output (any layout, as f32 on the host), ref: the exact result in float64, same layout (nonfinite_util.check_overflow with
    this file's bound: the finite part within 1.25 x its rounding floor)"""
    check_overflow(got, ref, floor_bound(1.25, F16), what, exact=True)


# (B, H, Cin, Cout, k) and the kernels each reaches (conv_igemm.hip / conv_pointwise.hip dispatch):
#   64 -> 128 3x3   forward glds | register-staged; input gradient (C = 128, 18 K stages) split-K under auto
#   128 -> 256 3x3  forward split-K (modes 3, 4) under auto, 256 x 256 tiles under t256; input gradient split-K under auto, 512 x 128 tiles under t256
#   3 -> 128 1x1    conv_pw_fwd (mode 3) and conv_pw_dgrad under auto
OVERFLOW_CONVS = [(2, 12, 64, 128, 3), (2, 16, 128, 256, 3), (2, 16, 3, 128, 1)]


@pytest.mark.parametrize("B,H,Cin,Cout,k", OVERFLOW_CONVS)
def test_fp16_overflow_conv_epilogues_and_dgrad(ops, B, H, Cin, Cout, k):
    """conv + bias + leaky-ReLU and conv + residual merge (the forward kernels' epilogues) and the input gradient, every family"""
    from enhancing import _C
    g = torch.Generator().manual_seed(1 + Cin)
    p, Cp = k // 2, ops.pad8(Cin)
    x = _draw((B, Cin, H, H), g, F16)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 16.0
    scale = 1.0 / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=g)
    ws, wa = h16r(w * scale, F16), h16r(w * (scale * ALPHA), F16)
    x = x * _pow2_scale(F.conv2d(x.double(), ws.double(), padding=p))
    y_ref = F.leaky_relu(F.conv2d(x.double(), ws.double(), padding=p) + bias.double().view(1, -1, 1, 1), 0.2) * 2 ** 0.5
    add = _draw(y_ref.shape, g, F16, 2e4)
    z_ref = F.conv2d(x.double(), wa.double(), padding=p) + ALPHA * add.double()
    dy = _draw((B, Cout, H, H), g, F16)                            # upstream gradient scaled past the range of the input gradient
    dy = dy * _pow2_scale(torch.nn.grad.conv2d_input(x.shape, ws.double(), dy.double(), padding=p))
    dx_ref = torch.nn.grad.conv2d_input(x.shape, ws.double(), dy.double(), padding=p)
    xp = torch.zeros(B, H, H, Cp, dtype=F16)
    xp[..., :Cin] = _nhwc(x).to(F16)
    xd = xp.cuda()
    for fam in FAMILIES:
        _C.conv_set_kernel(fam)
        try:
            y = ops.conv_bias_lrelu(xd, w.cuda(), bias.cuda(), scale, 1, p)
            z = ops.conv_add(xd, w.cuda(), _nhwc(add).to(F16).cuda(), scale * ALPHA, 1, p, ALPHA)
            xg = torch.zeros(B, H, H, Cp, dtype=F16, device="cuda").requires_grad_(True)
            ops.conv(xg, w.cuda(), scale, 1, p).backward(_nhwc(dy).to(F16).cuda())
        finally:
            _C.conv_set_kernel("auto")
        _check_overflow(_nchw(y), y_ref, f"{Cin}->{Cout} k{k} conv + bias + lrelu [{fam}]")
        _check_overflow(_nchw(z), z_ref, f"{Cin}->{Cout} k{k} conv_add [{fam}]")
        _check_overflow(_nchw(xg.grad)[:, :Cin], dx_ref, f"{Cin}->{Cout} k{k} dgrad [{fam}]")


# 64 -> 128: glds | register-staged kernels, no split; 128 -> 256: mode 0 split-K under auto and 256 x 256 tiles under t256, modes 1 and 2 (C = 256,
# N = 128) split-K under auto and 512 x 128 tiles under t256
@pytest.mark.parametrize("B,H,Cin,Cout", [(2, 16, 64, 128), (2, 16, 128, 256)])
def test_fp16_overflow_conv3x3_modes(ops, B, H, Cin, Cout):
    from enhancing import _C
    g = torch.Generator().manual_seed(2 + Cin)
    x = _draw((B, Cin, H, H), g, F16).clamp_min(0)
    w = _draw((Cout, Cin, 3, 3), g, F16, 16.0 / (9 * Cin) ** 0.5)
    bias = torch.randn(Cout, generator=g)
    x = x * _pow2_scale(F.conv2d(x.double(), w.double(), padding=1))
    y_ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), padding=1))
    gy = _draw((B, Cout, H, H), g, F16)
    gy = gy * _pow2_scale(torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), padding=1))
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), padding=1)
    aux, add = _draw((B, Cin, H, H), g, F16), _draw((B, Cin, H, H), g, F16, 3e4)
    m1_ref = (dx_ref + add.double()) * (aux > 0)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).to(F16).cuda()
    wb = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).to(F16).cuda()
    for fam in FAMILIES:
        _C.conv_set_kernel(fam)
        try:
            out = torch.empty(B, H, H, Cout, dtype=F16, device="cuda")
            _C.conv3x3_nhwc(_nhwc(x).to(F16).cuda(), wt, B, H, H, Cin, Cout, out, bias=bias.cuda(), mode=0)
            gx = torch.empty(B, H, H, Cin, dtype=F16, device="cuda")
            _C.conv3x3_nhwc(_nhwc(gy).to(F16).cuda(), wb, B, H, H, Cout, Cin, gx, mode=2)
            gx1 = torch.empty(B, H, H, Cin, dtype=F16, device="cuda")
            _C.conv3x3_nhwc(_nhwc(gy).to(F16).cuda(), wb, B, H, H, Cout, Cin, gx1, mode=1, aux=_nhwc(aux).to(F16).cuda(), add=_nhwc(add).to(F16).cuda())
        finally:
            _C.conv_set_kernel("auto")
        _check_overflow(_nchw(out), y_ref, f"conv3x3 {Cin}->{Cout} mode 0 [{fam}]")
        _check_overflow(_nchw(gx), dx_ref, f"conv3x3 {Cin}->{Cout} mode 2 [{fam}]")
        _check_overflow(_nchw(gx1), m1_ref, f"conv3x3 {Cin}->{Cout} mode 1 [{fam}]")


def test_fp16_overflow_elementwise_kernels(ops):
    """blur, lrelu_gate, vgg_conv1, lpips_head_backward and im2col"""
    import lpips_oracle as LO
    from enhancing import _C
    g = torch.Generator().manual_seed(3)
    kern = _blur_kernel() * 2.0
    x = _draw((2, 16, 20, 20), g, F16, 3e4, 2e4)
    y = ops.blur(_nhwc(x).to(F16).cuda(), kern.cuda(), (2, 2))
    _check_overflow(_nchw(y), _blur_ref(x.double(), kern, (2, 2)), "blur")
    a, r = _draw((3, 9, 11, 24), g, F16, 3e4), _draw((3, 9, 11, 24), g, F16)
    y = _C.lrelu_gate(a.to(F16).cuda(), r.to(F16).cuda(), 0.2, 2 ** 0.5)
    _check_overflow(y.float().cpu(), a.double() * torch.where(r > 0, 1.0, 0.2).double() * 2 ** 0.5, "lrelu_gate")
    img = torch.rand(2, 3, 16, 16, generator=g)
    w, b = torch.randn(64, 3, 3, 3, generator=g) * 1e4, torch.randn(64, generator=g)
    out = torch.empty(2, 16, 16, 64, dtype=F16, device="cuda")
    _C.vgg_conv1(img.cuda(), w.cuda(), b.cuda(), LO.SHIFT.reshape(-1).cuda(), LO.SCALE.reshape(-1).cuda(), True, out)
    ref = F.relu(F.conv2d(((2 * img.double() - 1) - LO.SHIFT.double()) / LO.SCALE.double(), w.double(), b.double(), padding=1))
    _check_overflow(_nchw(out), ref, "vgg_conv1")
    B, HW, C = 1, 8, 64
    f0 = torch.randn(B, C, HW, HW, generator=g).clamp_min(0)
    f = h16r(torch.cat([f0, torch.randn(B, C, HW, HW, generator=g).clamp_min(0)]), F16)
    lin = torch.rand(C, generator=g)
    _, unit = _head_ref(f, lin, B, torch.tensor([1.0]))
    gout = torch.tensor([2.0 ** round(torch.log2(3 * 65504.0 / unit.abs().max()).item())])    # the largest results ~3x past the range
    _, df_ref = _head_ref(f, lin, B, gout)
    df = torch.empty(B, HW, HW, C, dtype=F16, device="cuda")
    _C.lpips_head_backward(_nhwc(f).to(F16).cuda(), lin.cuda(), gout.cuda(), B, HW * HW, C, df)
    _check_overflow(_nchw(df), df_ref, "lpips_head_backward")
    xi = torch.randn(2, 5, 9, 9, generator=g) * 6e4
    cols = _C.im2col(xi.cuda(), 5 * 81, 81, 2, 5, 9, 9, 3, 1, 1, dtype=F16)
    ref = F.unfold(xi.double(), 3, padding=1).permute(0, 2, 1).reshape(-1, 45)
    _check_overflow(cols[:, :45].float().cpu(), ref, "im2col")
    assert torch.equal(cols[:, :45].cpu().view(torch.int16), ref.float().to(F16).view(torch.int16))


def test_fp16_inf_upstream_gradient_makes_the_weight_gradient_nonfinite(ops):
    """one inf in the fp16 upstream gradient of a conv layer: the f32 weight gradient must be non-finite, so that LossScaler's found-inf
    (enh_nonfinite_flag) drops the step"""
    from enhancing import _C
    g = torch.Generator().manual_seed(4)
    for (B, H, Cin, Cout, k, s, p) in [(2, 16, 64, 128, 3, 1, 1), (2, 17, 128, 256, 3, 2, 0), (2, 32, 3, 128, 1, 1, 0)]:
        Cp = ops.pad8(Cin)
        x = torch.zeros(B, H, H, Cp, dtype=F16)
        x[..., :Cin] = _draw((B, H, H, Cin), g, F16).to(F16)
        Ho = (H + 2 * p - k) // s + 1
        dy = _draw((B, Ho, Ho, Cout), g, F16).to(F16)
        dy[1, Ho // 2, Ho // 3, 5] = float("inf")
        for fam in FAMILIES:
            _C.conv_set_kernel(fam)
            try:
                wd = torch.randn(Cout, Cin, k, k, generator=g).cuda().requires_grad_(True)
                ops.conv(x.cuda(), wd, 1.0 / (Cin * k * k) ** 0.5, s, p).backward(dy.cuda())
                flag = torch.zeros(1, device="cuda")
                _C.nonfinite_flag(wd.grad.reshape(-1), flag)
            finally:
                _C.conv_set_kernel("auto")
            assert not torch.isfinite(wd.grad).all() and flag.item() == 1.0, (B, H, Cin, Cout, k, s, fam)


# ---------------------------------------------------------------------------------------------
# fp16 subnormals: gradient-carrying kernels keep them
# ---------------------------------------------------------------------------------------------
def _check_subnormal(got, ref, what):
    want = ref.to(F16).float()
    frac = (want.abs() < SUB)[ref != 0].float().mean().item()      # (exact zeros do not count as subnormal results)
    e = rel(got, ref) / floor16(ref, F16)
    flushed = ((got == 0) & (want.abs() >= 2.0 ** -23)).sum().item()
    print(f"subnormal {what}: {frac * 100:.1f} % of the nonzero rounded outputs subnormal, error {e:.3f} x floor, {flushed} flushed")
    assert frac >= 0.2, (what, frac)
    assert e <= 1.25 and flushed == 0, (what, e, flushed)


def _tiny(shape, g, target_rms):
    """an fp16 upstream gradient whose exact result has about target_rms (unit-scale operands times a power of two, then rounded: subnormal operands too)"""
    return h16r(torch.randn(*shape, generator=g) * target_rms, F16)


def test_fp16_subnormal_gradients_of_the_discriminator_kernels(ops):
    """dgrad, blur adjoint, lrelu_gate, stddev backward: outputs of rms ~1.2e-4 (about 40 % below 2^-14)"""
    from enhancing import _C
    g = torch.Generator().manual_seed(6)
    B, H, Cin, Cout = 2, 16, 64, 128
    w = torch.randn(Cout, Cin, 3, 3, generator=g)
    scale = 1.0 / (Cin * 9) ** 0.5
    ws = h16r(w * scale, F16)
    for s, p in ((1, 1), (2, 0)):
        Ho = (H + 2 * p - 3) // s + 1
        dy = _tiny((B, Cout, Ho, Ho), g, 1.2e-4 / (2 ** 0.5 if s == 1 else 0.71))    # rms(dx) = rms(dy) sqrt(taps per class * Cout / (9 Cin))
        dx_ref = torch.nn.grad.conv2d_input((B, Cin, H, H), ws.double(), dy.double(), stride=s, padding=p)
        for fam in FAMILIES:
            _C.conv_set_kernel(fam)
            try:
                xg = torch.zeros(B, H, H, Cin, dtype=F16, device="cuda").requires_grad_(True)
                ops.conv(xg, w.cuda(), scale, s, p).backward(_nhwc(dy).to(F16).cuda())
            finally:
                _C.conv_set_kernel("auto")
            _check_subnormal(_nchw(xg.grad), dx_ref, f"dgrad stride {s} [{fam}]")
    kern = _blur_kernel()
    gy = _tiny((2, 16, 21, 21), g, 4e-4)
    xr = torch.zeros(2, 16, 20, 20, dtype=torch.float64, requires_grad=True)
    _blur_ref(xr, kern, (2, 2)).backward(gy.double())
    xd = torch.zeros(2, 20, 20, 16, dtype=F16, device="cuda").requires_grad_(True)
    ops.blur(xd, kern.cuda(), (2, 2)).backward(_nhwc(gy).to(F16).cuda())
    _check_subnormal(_nchw(xd.grad), xr.grad, "blur adjoint")
    a, r = _tiny((3, 9, 11, 24), g, 1e-4), _draw((3, 9, 11, 24), g, F16)
    y = _C.lrelu_gate(a.to(F16).cuda(), r.to(F16).cuda(), 0.2, 2 ** 0.5)
    _check_subnormal(y.float().cpu(), a.double() * torch.where(r > 0, 1.0, 0.2).double() * 2 ** 0.5, "lrelu_gate")
    C_ = 512
    x = _draw((8, 4, 4, C_), g, F16)
    xr = x.double().clone().requires_grad_(True)
    yr = ops._stddev_torch(xr, 4, ops.pad8(C_ + 1))
    gy = _tiny(yr.shape, g, 1.2e-4)
    yr.backward(gy.double())
    xd = x.to(F16).cuda().requires_grad_(True)
    ops.minibatch_stddev(xd, 4).backward(gy.to(F16).cuda())
    _check_subnormal(xd.grad.float().cpu(), xr.grad, "stddev backward")


def test_fp16_subnormal_gradients_of_the_lpips_kernels(ops):
    """maxpool2 backward, conv3x3_nhwc modes 1 and 2, lpips_head_backward"""
    from enhancing import _C
    g = torch.Generator().manual_seed(7)
    B, H, C = 2, 16, 64
    x = _draw((B, C, H, H), g, F16).clamp_min(0)
    gy, add = _tiny((B, C, H // 2, H // 2), g, 1.2e-4), _tiny((B, C, H, H), g, 5e-5)
    xt = x.double().clone().requires_grad_(True)
    F.max_pool2d(xt, 2, 2).backward(gy.double())
    ref = (xt.grad + add.double()) * (x > 0)
    gx = torch.empty(B, H, H, C, dtype=F16, device="cuda")
    _C.maxpool2_nhwc_backward(_nhwc(x).to(F16).cuda(), _nhwc(gy).to(F16).cuda(), _nhwc(add).to(F16).cuda(), B, H, H, C, gx)
    sel = (x > 0)
    _check_subnormal(_nchw(gx)[sel], ref[sel], "maxpool2 backward")
    Cin, Cout = 64, 128
    w = _draw((Cout, Cin, 3, 3), g, F16, (2.0 / (9 * Cout)) ** 0.5)
    gy = _tiny((B, Cout, H, H), g, 8e-5)                 # rms(dx) = rms(gy) sqrt(2): ~40 % of it below 2^-14
    dx_ref = torch.nn.grad.conv2d_input((B, Cin, H, H), w.double(), gy.double(), padding=1)
    aux, add = _draw((B, Cin, H, H), g, F16), _tiny((B, Cin, H, H), g, 5e-5)
    m1_ref = (dx_ref + add.double()) * (aux > 0)
    wb = w.flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, 9 * Cout).to(F16).cuda()
    for fam in FAMILIES:
        _C.conv_set_kernel(fam)
        try:
            gx = torch.empty(B, H, H, Cin, dtype=F16, device="cuda")
            _C.conv3x3_nhwc(_nhwc(gy).to(F16).cuda(), wb, B, H, H, Cout, Cin, gx, mode=2)
            gx1 = torch.empty(B, H, H, Cin, dtype=F16, device="cuda")
            _C.conv3x3_nhwc(_nhwc(gy).to(F16).cuda(), wb, B, H, H, Cout, Cin, gx1, mode=1, aux=_nhwc(aux).to(F16).cuda(), add=_nhwc(add).to(F16).cuda())
        finally:
            _C.conv_set_kernel("auto")
        _check_subnormal(_nchw(gx), dx_ref, f"conv3x3 mode 2 [{fam}]")
        sel = (aux > 0)
        _check_subnormal(_nchw(gx1)[sel], m1_ref[sel], f"conv3x3 mode 1 [{fam}]")
    HW = 16
    f0 = torch.randn(1, C, HW, HW, generator=g).clamp_min(0)
    f = h16r(torch.cat([f0, (f0 + 0.3 * torch.randn(1, C, HW, HW, generator=g)).clamp_min(0)]), F16)
    lin = torch.rand(C, generator=g)
    _, unit = _head_ref(f, lin, 1, torch.tensor([1.0]))
    gout = torch.tensor([2.0 ** round(torch.log2(1.2e-4 / unit.pow(2).mean().sqrt()).item())])   # rms of the result ~1.2e-4
    _, df_ref = _head_ref(f, lin, 1, gout)
    df = torch.empty(1, HW, HW, C, dtype=F16, device="cuda")
    _C.lpips_head_backward(_nhwc(f).to(F16).cuda(), lin.cuda(), gout.cuda(), 1, HW * HW, C, df)
    _check_subnormal(_nchw(df), df_ref, "lpips_head_backward")


def test_fp16_lpips_head_gradient_floor_at_256px_over_the_loss_scales(ops):
    """Report: the fp16 floor of LPIPS's first-slice head gradient at HW = 65536 for the magnitude a generator step produces (perceptual_weight 0.1 of
    configs/imagenet_vitvq_base_full.yaml, the mean over its batch of 8, times the loss scale), and the share of it in fp16's subnormal range.  The
    generator step's LPIPS backward runs under the engine's scale (engine/stage1.py: ENH_LOSS_SCALE, 2^16 by default, halved on every overflow); the
    2^12 default of engine/optim.py's LossScaler is the discriminator step's.  Swept over 2^10 .. 2^16, the range a backed-off dynamic scale visits.
    The features are synthetic (clamped Gaussians, the reconstruction's = the input's + 10 % noise), not VGG activations: the numbers are an estimate.
    The kernel is held to its class (1.25 x the floor) at every scale; the floor itself is the number reported."""
    from enhancing import _C
    g = torch.Generator().manual_seed(8)
    HW, C, batch = 256, 64, 8
    f0 = torch.randn(1, C, HW, HW, generator=g).clamp_min(0)
    f = h16r(torch.cat([f0, (f0 + 0.1 * torch.randn(1, C, HW, HW, generator=g)).clamp_min(0)]), F16)
    lin = torch.rand(C, generator=g)
    _, unit = _head_ref(f, lin, 1, torch.tensor([1.0]))          # linear in gout: one fp64 gradient, scaled exactly below
    fd = _nhwc(f).to(F16).cuda()
    nz = unit != 0                  # (exact zeros: channels where both images' features are zero)
    for k in range(10, 17):
        go = 0.1 / batch * 2.0 ** k
        ref = unit * go
        df = torch.empty(1, HW, HW, C, dtype=F16, device="cuda")
        _C.lpips_head_backward(fd, lin.cuda(), torch.tensor([go], device="cuda"), 1, HW * HW, C, df)
        fl = floor16(ref, F16)
        want = ref.to(F16).float()
        frac, zero = (want.abs() < SUB)[nz].float().mean().item(), (want == 0)[nz].float().mean().item()
        e = rel(_nchw(df), ref) / fl
        print(f"lpips head gradient @256^2, loss scale 2^{k}{' (the generator default)' if k == 16 else ''}: fp16 floor {fl:.2e} "
              f"(bf16 {floor16(ref, BF16):.2e}); of the nonzero values {frac * 100:.1f} % subnormal, {zero * 100:.2f} % rounded to zero; kernel {e:.3f} x floor")
        assert e <= 1.25
