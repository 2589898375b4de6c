"""The discriminator and LPIPS kernels (csrc/conv_igemm.hip, conv_pointwise.hip, disc_ops.hip, lpips_ops.hip) held to a bound PER ELEMENT against fp64,
on every kernel variant and epilogue, at the smallest shapes that reach each of them, with the edge values the random inputs of the other op tests never
contain (tests/test_local_error_metric_cpu.py records why one Frobenius number per tensor is not enough; tests/test_loss_kernels_metric_cpu.py shows these
bounds on an f32 emulation and on injected faults).

Pattern of every test: operands exactly representable in the format under test (drawn separately for bf16 and fp16), reference in plain fp64 torch on the
CPU (tests/loss_kernels_util.py), limit util.elem_bound or a bound derived the same way from the number formats — DERIVED, not fitted: no bound was changed
after a kernel's figure was seen — output buffers pre-filled with NaN wherever the call takes the buffer (the autograd wrappers allocate their own: there
a NaN block of the same size is handed back to the allocator just before), util.assert_elementwise reports the worst element, its err / bound is printed.
An honest kernel's ratio is at most 1.  The device trace (torch.profiler) proves which kernel ran: a case that does not reach its named kernel fails.

  part 1  epilogue modes 0, 1 (with / without add; post-ReLU aux; +-0, subnormals, smallest normals in aux), 2, 3 (with / without bias), 4 on
          conv_igemm_kernel (auto and reg), conv_igemm_glds_kernel unsplit, glds + conv_splitk_finish_kernel, conv_igemm_w256_kernel,
          conv_igemm_w512_kernel, conv_pw_fwd_kernel (modes 2, 3; 1, 2, 4, 8, 16 groups).  Modes 3 and 4 go through _C.conv_nhwc like conv_nhwc._fwd
          does, with a NaN-filled output buffer (which _fwd cannot take); conv_bias_lrelu / conv_add themselves run in part 3
  part 2  conv_pw_dgrad_kernel at 1 .. 64 lane groups, conv_pw_wgrad_kernel (+ conv_pw_reduce_kernel) at 1 .. 16 groups, one slab and several
  part 3  the fused backward of conv_bias_lrelu / conv_add launch by launch from the device's own stored tensors, and the R1-style second-order dw
  part 4  vgg_conv1 forward / backward (non-square, both scalings), max-pool backward on positive ties, the LPIPS head and its backward with zero vectors
  part 5  blur and its adjoint (4 x 4 and a 3 x 3 kernel), minibatch stddev against the reference project's definition restated in fp64

Measured on MI355X (largest err / bound per kernel over its cases and modes, bf16 | fp16; the bounds are derived, not fitted, and every figure is <= 1):
  conv_igemm_kernel, all epilogues 0.945 | 0.835 (auto = reg), 1 x 1 stride-2 mode 4 0.976 | 0.946     conv_igemm_glds_kernel 0.932 | 0.623
  glds + conv_splitk_finish_kernel 0.806 | 0.441     conv_igemm_w256_kernel 0.909 | 0.656     conv_igemm_w512_kernel 0.918 | 0.688
  conv_pw_fwd_kernel 0.996 | 0.993     conv_pw_dgrad_kernel 0.979 | 0.956     conv_pw_wgrad_kernel (+ conv_pw_reduce_kernel) 0.0067 | 0.0081 of the f32 bound
  fused backward: y 0.946 | 0.752, dx 0.934 | 0.747, dw 0.0097 | 0.0081, db 0.0000 | 0.0009, second-order dw 0.0080 | 0.0090; conv_add 0.939 | 0.781
  vgg_conv1 0.991 | 0.969, its image gradient 0.0024 | 0.0021 (f32)     max-pool forward / backward bit-exact (387 | 384 windows with a positive tie)
  lpips_head val 0.022 | 0.019, out 0.003 | 0.003, gradient 0.994 | 0.999 (fp16: 31 - 246 elements +-inf at the zero-f1 pixel, exactly the reference's)
  blur 0.995 | 0.982, adjoint 0.993 | 0.990, 3 x 3 kernel 0.984 | 0.976     minibatch stddev statistic 0.481 | 0.515, backward 0.989 | 0.995
  (16-bit outputs sit near 1 because the bound IS half an ulp at the bottom of a binade; f32 outputs use a sliver of the any-order summation bound.)
The whole file runs in about 5 s; the slowest test (the first, which starts the profiler) takes 1.8 s.

Found by part 1: conv_pack_weight_kernel<F16> rounds the EXACT product scale * w once to fp16 (one v_fma_mixlo_f16) where the bf16 instance and
h16r(w * scale) round the f32 product: one fp16 ulp on about one weight in 8192, err / bound 1.01 (24 -> 72, mode 2) and 2.64 (40 -> 64 stride 2, mode 4)
at the affected channels.  Forcing the f32 product in the kernel moved test_disc_model_gpu's fp16 golden case past its limit (leaky-ReLU gates of the
random-init net flip), so the kernel stays as it is and the references here use the operand it really produces (loss_kernels_util.packed_weight, pinned
bit for bit by test_packed_weights_match_their_cpu_model).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import loss_kernels_util as K
from util import assert_elementwise, elem_bound, h16r

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from enhancing import _C
    from enhancing.losses.op import conv_nhwc
    _C.lib()
    yield conv_nhwc
    _C.conv_set_kernel("auto")


def _launched(fn):
    """names of the GPU kernels that fn() launches (torch.profiler's device trace), as tests/test_conv_nhwc_gpu.py does"""
    from torch.profiler import ProfilerActivity, profile, supported_activities
    assert ProfilerActivity.CUDA in supported_activities()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events()}


def _ran(names, kernel):
    return any(kernel in n for n in names)


def _poison(shape, dt):
    """best effort for buffers a wrapper allocates itself: a NaN block of the same size goes back to the caching allocator, which hands the most recently
    freed fitting block to the next request"""
    t = torch.full(shape, NAN, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    del t


def _dev(x_nchw, dt, Cp=None):
    """NCHW f32 host -> channels-last dt on the device, channels zero-padded to Cp"""
    x = K.nhwc(x_nchw)
    if Cp is not None and Cp > x.shape[-1]:
        x = torch.cat([x, x.new_zeros(*x.shape[:-1], Cp - x.shape[-1])], -1)
    return x.to(dt).cuda()


def _host(y_nhwc):
    return K.nchw(y_nhwc.float().cpu())


def _fwd_geom(B, H, W, Cp, Cout, k, s, p):
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return dict(B=B, Hs=H, Ws=W, C=Cp, Hm=Ho, Wm=Wo, gs=s, oy0=-p, ox0=-p, nty=k, ntx=k, sty=1, stx=1, N=Cout, HO=Ho, WO=Wo, os=1, oph=0, opw=0)


def _conv(ops, case, xd, wd, mode, bias=None, aux=None, add=None, p0=0.0, p1=1.0):
    """one forward launch as conv_nhwc._fwd makes it, into a NaN-filled buffer"""
    from enhancing import _C
    B, H, W, Cin, Cout, k, s, p = case["geom"]
    Cp = xd.shape[-1]
    wt = ops._pack(wd, case["scale"], False, 0, 0, 1, k, k, Cout, Cp, dtype=xd.dtype)
    geom = _fwd_geom(B, H, W, Cp, Cout, k, s, p)
    out = torch.full((B, geom["HO"], geom["WO"], Cout), NAN, dtype=xd.dtype, device="cuda")
    _C.conv_nhwc(xd, wt, geom, mode, bias=bias, aux=aux, add=add, p0=p0, p1=p1, out=out)
    return _host(out)


# ---------------------------------------------------------------------------------------------
# part 1: every epilogue on every forward kernel
# ---------------------------------------------------------------------------------------------
A_IGEMM, A_SKIP, A_GLDS, A_SPLIT, A_W256, A_W512 = ((1, 9, 7, 24, 72, 3, 1, 1), (2, 15, 15, 40, 64, 1, 2, 0), (2, 9, 7, 64, 136, 3, 1, 1),
                                                    (2, 6, 5, 128, 136, 3, 1, 1), (1, 20, 13, 64, 256, 3, 1, 1), (1, 23, 23, 64, 128, 3, 1, 1))
ALL_MODES = ("0", "1add", "1", "1special", "2", "3", "3nobias", "4")
# (id, family, geometry, kernels the trace must show, modes, tile of the error report)
EPILOGUE_ROWS = [
    ("igemm-auto", "auto", A_IGEMM, ("conv_igemm_kernel",), ALL_MODES, (128, 128)),
    ("igemm-reg", "reg", A_IGEMM, ("conv_igemm_kernel",), ALL_MODES, (128, 128)),
    ("igemm-skip-auto", "auto", A_SKIP, ("conv_igemm_kernel",), ("4",), (128, 128)),
    ("igemm-skip-reg", "reg", A_SKIP, ("conv_igemm_kernel",), ("4",), (128, 128)),
    ("glds", "auto", A_GLDS, ("conv_igemm_glds_kernel",), ALL_MODES, (128, 128)),
    ("glds-splitk", "auto", A_SPLIT, ("conv_igemm_glds_kernel", "conv_splitk_finish_kernel"), ALL_MODES, (128, 128)),
    ("w256", "t256", A_W256, ("conv_igemm_w256_kernel",), ALL_MODES, (256, 256)),
    ("w512", "t256", A_W512, ("conv_igemm_w512_kernel",), ALL_MODES, (512, 128)),
]


def _epilogue_cases(case, dt):
    """mode id -> (mode, kernel arguments as host tensors, reference arguments)"""
    bias, add, aux = case["bias"], case["add"], case["aux"]
    aux_dt, aux_sp = aux.to(dt), K.crafted_aux(aux, dt)
    zeros = (aux_dt == 0).float().mean().item()
    assert zeros >= 0.3, f"the post-ReLU aux holds {zeros:.2f} exact zeros"
    sp = aux_sp[0, :, 0, :]
    assert len(sp.contiguous().view(torch.int16).unique()) == 6 and bool((sp > 0).any()) and bool((sp == 0).any()) and bool((sp < 0).any())
    return {"0": (0, dict(bias=bias), {}), "1add": (1, dict(add=add, aux_dt=aux_dt), {}), "1": (1, dict(aux_dt=aux_dt), {}),
            "1special": (1, dict(add=add, aux_dt=aux_sp), {}), "2": (2, {}, {}),
            "3": (3, dict(bias=bias), dict(p0=K.SLOPE, p1=K.ACT_SCALE)), "3nobias": (3, {}, dict(p0=K.SLOPE, p1=K.ACT_SCALE)),
            "4": (4, dict(add=add), dict(p0=K.ALPHA))}


@DTS
@pytest.mark.parametrize("row", EPILOGUE_ROWS, ids=[r[0] for r in EPILOGUE_ROWS])
def test_every_epilogue_on_every_forward_kernel(ops, row, dt):
    from enhancing import _C
    name, family, geom, kernels, modes, tile = row
    case = K.conv_case(*geom, dt)
    B, H, W, Cin, Cout, k, s, p = geom
    if "conv_splitk_finish_kernel" in kernels:
        nb = _C.lib().enh_conv_workspace_bytes(ctypes.byref(_C._geom(_fwd_geom(B, H, W, Cin, Cout, k, s, p))))
        assert nb > 0, f"{geom}: the library plans no split over the contraction for this geometry on this device ({_C.device_cus()} CUs)"
    xd, wd = _dev(case["x"], dt), case["w"].cuda()
    table = _epilogue_cases(case, dt)
    got = {}

    def run():
        for m in modes:
            mode, args, par = table[m]
            dev = {}
            if "bias" in args:
                dev["bias"] = args["bias"].cuda()
            if "add" in args:
                dev["add"] = _dev(args["add"], dt)
            if "aux_dt" in args:
                dev["aux"] = K.nhwc(args["aux_dt"]).cuda()
            got[m] = _conv(ops, case, xd, wd, mode, **dev, **par)
    _C.conv_set_kernel(family)
    try:
        names = _launched(run)
    finally:
        _C.conv_set_kernel("auto")
    for kern in kernels:
        assert _ran(names, kern), f"{name}: {kern} did not run; launched {sorted(n.split('(')[0] for n in names if 'conv' in n)}"
    worst = {}
    for m in modes:
        mode, args, par = table[m]
        ref, bound = K.epilogue_ref(case, mode, **args, **par)
        # [B, C, H, W] -> rows = pixels, columns = channels, so that the tile coordinates of a failure are the kernel's
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cout)
        worst[m] = assert_elementwise(flat(got[m]), flat(ref), flat(bound), f"{name} {dt} mode {m} {geom}", tile=tile)
    print(f"{name} {dt}: max err / bound per mode " + "  ".join(f"{m} {v:.3f}" for m, v in worst.items()))


@DTS
def test_packed_weights_match_their_cpu_model(ops, dt):
    """conv_pack_weight against loss_kernels_util.packed_weight bit for bit, both layouts.  The fp16 instance rounds the EXACT product scale * w once, the
    bf16 instance the f32 product; the weights hold f32 products on an fp16 tie (asserted), where the two differ by one ulp — the references of this file
    use the operand the kernel really produces (with h16r(w * scale) the epilogue tests of conv_igemm_kernel show err / bound 1.01 and 2.64 in fp16)."""
    from enhancing import _C
    g = torch.Generator().manual_seed(4)
    w = torch.randn(256, 40, 3, 3, generator=g)
    scale = 1.0 / 360 ** 0.5
    want = K.packed_weight(w, scale, dt)
    if dt == F16:
        assert 4 <= int((want != h16r(w * scale, dt)).sum()) <= 40       # ~ 92160 / 8192 double-rounding ties
    for transposed, rows, cols in ((False, 256, 40), (True, 40, 256)):
        wt = _C.conv_pack_weight(w.cuda(), scale, transposed, 0, 0, 1, 3, 3, rows, cols, dtype=dt).cpu().float()
        ref = (want.permute(0, 2, 3, 1) if not transposed else want.permute(1, 2, 3, 0)).reshape(rows, 9 * cols)
        assert torch.equal(wt, ref), f"{int((wt != ref).sum())} packed weights differ from the CPU model"


PW_COUTS = [8, 16, 32, 64, 128]


@DTS
@pytest.mark.parametrize("Cout", PW_COUTS)
def test_pointwise_forward_every_group_count(ops, Cout, dt):
    """conv_pw_fwd_kernel (Cin = 3 padded to 8; 1, 2, 4, 8, 16 groups of 8 output channels) in modes 2 and 3 (the discriminator's first layer) at 189
    pixels: no multiple of any pixels-per-workgroup unit"""
    geom = (3, 7, 9, 3, Cout, 1, 1, 0)
    case = K.conv_case(*geom, dt)
    xd, wd, bd = _dev(case["x"], dt, 8), case["w"].cuda(), case["bias"].cuda()
    got = {}

    def run():
        got["2"] = _conv(ops, case, xd, wd, 2)
        got["3"] = _conv(ops, case, xd, wd, 3, bias=bd, p0=K.SLOPE, p1=K.ACT_SCALE)
        got["3nobias"] = _conv(ops, case, xd, wd, 3, p0=K.SLOPE, p1=K.ACT_SCALE)
    names = _launched(run)
    assert _ran(names, "conv_pw_fwd_kernel") and not any("igemm" in n for n in names), sorted(names)
    refs = {"2": K.epilogue_ref(case, 2), "3": K.epilogue_ref(case, 3, bias=case["bias"], p0=K.SLOPE, p1=K.ACT_SCALE),
            "3nobias": K.epilogue_ref(case, 3, p0=K.SLOPE, p1=K.ACT_SCALE)}
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Cout)
    worst = {m: assert_elementwise(flat(got[m]), flat(refs[m][0]), flat(refs[m][1]), f"pointwise forward {dt} Cout {Cout} mode {m}", tile=(2048 // Cout, 8))
             for m in got}
    print(f"conv_pw_fwd {dt} Cout {Cout}: max err / bound " + "  ".join(f"{m} {v:.3f}" for m, v in worst.items()))


# ---------------------------------------------------------------------------------------------
# part 2: the pointwise input and weight gradients at every group count
# ---------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("Cout", [8, 16, 32, 64, 128, 256, 512])
def test_pointwise_input_gradient_every_group_count(ops, Cout, dt):
    """conv_pw_dgrad_kernel: dx[p][c] = sum_n dy[p][n] w[n][c] over Cout / 8 = 2 .. 64 lanes per pixel (16: the DPP row rotations; 32, 64: the
    __shfl_xor butterfly); one 16-bit rounding of an f32 sum of Cout products; the five zero padding channels receive exactly zero.
    Cout = 8 (one group) is an 8 -> 8 geometry, which conv_pointwise_forward hands to conv_pw_fwd_kernel before it looks at the input-gradient form: the
    one-group instance of conv_pw_dgrad_kernel cannot be reached through the library, and the trace assertion says which kernel ran."""
    from enhancing import _C
    B, H, W, Cin = 3, 7, 9, 3
    g = torch.Generator().manual_seed(Cout + (dt == F16))
    w = torch.randn(Cout, Cin, 1, 1, generator=g)
    scale = 1.0 / Cin ** 0.5
    ws = K.packed_weight(w, scale, dt).double().view(Cout, Cin)
    dy = h16r(torch.randn(B, Cout, H, W, generator=g), dt)
    ref = torch.einsum("bnhw,nc->bchw", dy.double(), ws)
    mag = torch.einsum("bnhw,nc->bchw", dy.double().abs(), ws.abs())
    dyd, wd = _dev(dy, dt), w.cuda()
    out = torch.full((B, H, W, 8), NAN, dtype=dt, device="cuda")

    def run():
        wt = ops._pack(wd, scale, True, 0, 0, 1, 1, 1, 8, Cout, dtype=dt)
        geom = dict(B=B, Hs=H, Ws=W, C=Cout, Hm=H, Wm=W, gs=1, oy0=0, ox0=0, nty=1, ntx=1, sty=-1, stx=-1, N=8, HO=H, WO=W, os=1, oph=0, opw=0)   # conv_nhwc._dgrad
        _C.conv_nhwc(dyd, wt, geom, 2, out=out)
    names = _launched(run)
    assert _ran(names, "conv_pw_dgrad_kernel" if Cout > 8 else "conv_pw_fwd_kernel") and not any("igemm" in n for n in names), sorted(names)
    gx = _host(out)
    r = assert_elementwise(gx[:, :Cin], ref, elem_bound(ref, mag, Cout, dt), f"pointwise input gradient {dt} Cout {Cout}")
    assert torch.equal(gx[:, Cin:], torch.zeros(B, 8 - Cin, H, W)), "gradient of the zero padding channels"
    print(f"conv_pw_dgrad {dt} {Cout // 8} groups: max err / bound {r:.3f}")


@DTS
@pytest.mark.parametrize("Cout", PW_COUTS)
@pytest.mark.parametrize("shape", [(1, 5, 9), (2, 37, 41)], ids=["one-slab", "slabs"])
def test_pointwise_weight_gradient_every_group_count(ops, shape, Cout, dt):
    """conv_pw_wgrad_kernel: dw[n][c] = sum_p dy[p][n] x[p][c] in f32.  45 pixels are one slab at every width (pw_pix_per_wg: a slab is at least
    4 * 256 / groups >= 64 pixels), written straight to dw; 3034 pixels are 3 (Cout 8) to 48 (Cout 128) slabs, added by conv_pw_reduce_kernel (48 > 16: its
    waves walk more than one slab each).  The packed [Cout, 8] result is compared, before conv_unpack_wgrad; two calls agree bit for bit."""
    from enhancing import _C
    B, H, W = shape
    Cin, M = 3, B * H * W
    g = torch.Generator().manual_seed(Cout + M + (dt == F16))
    x = h16r(torch.randn(B, Cin, H, W, generator=g), dt)
    dy = h16r(torch.randn(B, Cout, H, W, generator=g), dt)
    ref = torch.einsum("bnhw,bchw->nc", dy.double(), x.double())
    mag = torch.einsum("bnhw,bchw->nc", dy.double().abs(), x.double().abs())
    xd, dyd = _dev(x, dt, 8), _dev(dy, dt)
    geom = _C._geom(_fwd_geom(B, H, W, 8, Cout, 1, 1, 0))
    nb = _C.lib().enh_conv_wgrad_workspace_bytes(ctypes.byref(geom))
    unit = 4 * (256 // (Cout // 8))                                        # pw_pix_per_wg of conv_pointwise.hip: whole passes of four pixels per thread
    per = max(unit, -(-(-(-M // 512)) // unit) * unit)
    slabs = -(-M // per)
    assert (slabs > 1) == (M > 64) and (slabs == 1 or nb >= slabs * Cout * 8 * 4), (slabs, M, nb)
    ws = _C._gemm_workspace(xd.device, nb) if nb else None
    outs = [torch.full((Cout, 8), NAN, device="cuda") for _ in range(2)]

    def run():
        for dw in outs:     # _C.conv_wgrad_nhwc with a NaN-filled result buffer
            _C._check(_C.lib().enh_conv_wgrad_nhwc_h16(_C._p(xd, _C.H16, "src"), _C._p(dyd, _C.H16, "dy"), ctypes.byref(geom), _C._p(dw), _C._p(ws), nb,
                                                       _C._dt(xd, dyd), _C._stream()), "enh_conv_wgrad_nhwc_h16")
    names = _launched(run)
    assert _ran(names, "conv_pw_wgrad_kernel") and _ran(names, "conv_pw_reduce_kernel") == (slabs > 1) and not any("igemm" in n for n in names), sorted(names)
    dw = outs[0].cpu()
    r = assert_elementwise(dw[:, :Cin], ref, elem_bound(ref, mag, M), f"pointwise weight gradient {dt} Cout {Cout} {M} pixels")
    assert torch.equal(dw[:, Cin:], torch.zeros(Cout, 8 - Cin)) and torch.equal(outs[0], outs[1])
    print(f"conv_pw_wgrad {dt} {Cout // 8} groups, {slabs} slabs: max err / f32 bound {r:.4f}")


# ---------------------------------------------------------------------------------------------
# part 3: the fused backward, launch by launch from stored tensors
# ---------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("geom", [(2, 9, 7, 64, 136, 3, 1, 1), (2, 17, 17, 32, 64, 3, 2, 0)], ids=["s1p1-64-136", "s2p0-32-64"])
def test_fused_backward_from_stored_tensors(ops, geom, dt):
    """conv_bias_lrelu and conv_add: forward per element; then the backward started from what the device STORED (as tests/test_elementwise_gpu.py starts
    the attention backward from the stored out): g_pre = lrelu_gate(g, out) on the device's own out equals its torch restatement bit for bit, and dx, dw, db
    are held per element against fp64 computed from that g_pre — dx one 16-bit rounding of a sum of Cout k^2 products, dw and db f32 sums over the
    B Ho Wo pixels.  Then the R1-style term: w.grad of |d out / d x|^2 is a weight gradient of G = 2 gxd (exact in 16 bits) against the stored g_pre, held
    per element against fp64 from those two device tensors (the derived bound for what test_conv_nhwc_gpu.py limits by `second-order dw <= 2e-2`)."""
    from enhancing import _C
    from enhancing.losses.op import conv2d_gradfix
    B, H, W, Cin, Cout, k, s, p = geom
    case = K.conv_case(*geom, dt)
    x, w, scale, ws = case["x"], case["w"], case["scale"], case["ws"]
    n_pix = B * case["pre"].shape[2] * case["pre"].shape[3]
    gen = torch.Generator().manual_seed(Cin + (dt == F16))
    gy = h16r(torch.randn(case["pre"].shape, generator=gen), dt)
    gyd = _dev(gy, dt)
    what = f"fused {dt} {geom}"
    xd, wd, bd = _dev(x, dt).requires_grad_(True), w.cuda().requires_grad_(True), case["bias"].cuda().requires_grad_(True)
    _poison((B, case["pre"].shape[2], case["pre"].shape[3], Cout), dt)
    y = ops.conv_bias_lrelu(xd, wd, bd, scale, s, p)
    ref, bound = K.epilogue_ref(case, 3, bias=case["bias"], p0=K.SLOPE, p1=K.ACT_SCALE)
    r_y = assert_elementwise(_host(y.detach()), ref, bound, what + " conv_bias_lrelu")
    # the gate on the device's own out, and its torch restatement (the kernel's association: g * (gate * scale))
    g_pre = _C.lrelu_gate(gyd, y.detach(), K.SLOPE, K.ACT_SCALE)
    want = (K.nhwc(gy) * (torch.where(y.detach().float().cpu() > 0, 1.0, K.SLOPE) * K.ACT_SCALE)).to(dt)
    assert torch.equal(g_pre.cpu(), want), what + ": lrelu_gate on the stored out differs from its torch restatement"
    gp = _host(g_pre)
    y.backward(gyd, retain_graph=True)
    dx_ref, dw_ref, dx_mag, dw_mag = K.conv_grads64(x, ws, gp, s, p)
    r_x = assert_elementwise(_host(xd.grad), dx_ref, elem_bound(dx_ref, dx_mag, Cout * k * k, dt), what + " dx")
    r_w = assert_elementwise(wd.grad.cpu(), scale * dw_ref, elem_bound(scale * dw_ref, scale * dw_mag, n_pix), what + " dw")
    db_ref, db_mag = gp.double().sum((0, 2, 3)), gp.double().abs().sum((0, 2, 3))
    r_b = assert_elementwise(bd.grad.cpu(), db_ref, elem_bound(db_ref, db_mag, n_pix), what + " db")
    # R1-style second-order term
    wd.grad = None; bd.grad = None; xd.grad = None
    with conv2d_gradfix.no_weight_gradients():
        gxd, = torch.autograd.grad(y, xd, gyd, create_graph=True)
    gxd.float().square().sum().backward()
    G = 2 * _host(gxd.detach())
    assert torch.equal(h16r(G, dt), G)                                    # the upstream gradient of the square: exact in 16 bits
    _, dw2_ref, _, dw2_mag = K.conv_grads64(G, ws, gp, s, p)                # weight gradient with x := G, dy := the stored g_pre
    r_2 = assert_elementwise(wd.grad.cpu(), scale * dw2_ref, elem_bound(scale * dw2_ref, scale * dw2_mag, n_pix), what + " second-order dw")
    assert bd.grad is None or not bd.grad.abs().sum().item()
    # residual merge: alpha * (conv + add) with alpha folded into the weights; its backward from the upstream gradient itself
    xa, wa = _dev(x, dt).requires_grad_(True), w.cuda().requires_grad_(True)
    addd = _dev(case["add"], dt).requires_grad_(True)
    _poison(tuple(y.shape), dt)
    z = ops.conv_add(xa, wa, addd, scale, s, p, K.ALPHA)
    ref, bound = K.epilogue_ref(case, 4, add=case["add"], p0=K.ALPHA)
    r_z = assert_elementwise(_host(z.detach()), ref, bound, what + " conv_add")
    z.backward(gyd)
    dx_ref, dw_ref, dx_mag, dw_mag = K.conv_grads64(x, ws, gy, s, p)
    r_zx = assert_elementwise(_host(xa.grad), dx_ref, elem_bound(dx_ref, dx_mag, Cout * k * k, dt), what + " conv_add dx")
    r_zw = assert_elementwise(wa.grad.cpu(), scale * dw_ref, elem_bound(scale * dw_ref, scale * dw_mag, n_pix), what + " conv_add dw")
    assert torch.equal(addd.grad.cpu(), (K.nhwc(gy) * K.ALPHA).to(dt)), what + ": d add = (g * alpha) rounded once"
    print(f"{what}: max err / bound  y {r_y:.3f}  dx {r_x:.3f}  dw {r_w:.4f}  db {r_b:.4f}  second-order dw {r_2:.4f}  |  add {r_z:.3f}  dx {r_zx:.3f}  dw {r_zw:.4f}")


# ---------------------------------------------------------------------------------------------
# part 4: the LPIPS kernels of lpips_ops.hip
# ---------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "plain"])
@pytest.mark.parametrize("shape", [(2, 5, 11), (1, 16, 24)])
def test_vgg_conv1_nonsquare(ops, shape, normalize, dt):
    """the first VGG convolution fused with lpips' scaling layer, and its image gradient, at non-square sizes (a swapped H / W in the pixel decomposition is
    the identity at the square sizes of the other tests), with both input scalings.  2 x 5 x 11: 1760 forward threads and 110 backward threads, no multiple
    of 256 (a ragged last workgroup); 1 x 16 x 24: whole workgroups in the forward (6144 threads), a ragged one in the backward (384)"""
    from enhancing import _C
    B, H, W = shape
    assert H != W and (B * H * W) % 256
    c = K.vgg_conv1_case(B, H, W, normalize, dt)
    sh, sc, wd = K.VGG_SHIFT.cuda(), K.VGG_SCALE.cuda(), c["w"].cuda()
    out = torch.full((B, H, W, 64), NAN, dtype=dt, device="cuda")
    _C.vgg_conv1(c["img"].cuda(), wd, c["bias"].cuda(), sh, sc, normalize, out)
    r_f = assert_elementwise(_host(out), c["ref"], c["bound"], f"vgg_conv1 {dt} {shape} normalize={normalize}")
    dimg = torch.full((B, 3, H, W), NAN, device="cuda")
    _C.vgg_conv1_backward(_dev(c["gpre"], dt), wd, sc, normalize, B, H, W, dimg)
    r_b = assert_elementwise(dimg.cpu(), c["dimg"], c["dimg_bound"], f"vgg_conv1_backward {dt} {shape} normalize={normalize}")
    print(f"vgg_conv1 {dt} {shape} normalize={normalize}: max err / bound forward {r_f:.3f}, image gradient (f32) {r_b:.4f}")


@DTS
def test_maxpool_backward_routes_positive_ties_to_the_first_maximum(ops, dt):
    """every 2 x 2 window of the first channel group holds a POSITIVE tie (ties at 0 are masked by x > 0 whatever the argmax was): forward and backward,
    with and without the head's addend, equal F.max_pool2d and its autograd (first maximum in scan order) bit for bit"""
    from enhancing import _C
    x, gy, add = K.maxpool_case(dt)
    B, C, H, W = x.shape
    ties = K.positive_ties(x)
    assert ties >= 64 and K.positive_ties(x[:, :8]) == B * 8 * (H // 2) * (W // 2), ties
    xd, gyd = _dev(x, dt), _dev(gy, dt)
    y = torch.full((B, H // 2, W // 2, C), NAN, dtype=dt, device="cuda")
    _C.maxpool2_nhwc(xd, B, H, W, C, y)
    assert torch.equal(_host(y), F.max_pool2d(x, 2, 2))
    for a in (add, None):
        gx = torch.full((B, H, W, C), NAN, dtype=dt, device="cuda")
        _C.maxpool2_nhwc_backward(xd, gyd, _dev(a, dt) if a is not None else None, B, H, W, C, gx)
        want = K.maxpool_backward_ref(x, gy, a, dt)
        got = K.nchw(gx.cpu())
        assert torch.equal(got, want), f"maxpool backward {dt} add={'given' if a is not None else None}: {int((got != want).sum())} elements differ"
        assert not torch.equal(want, K.maxpool_backward_ref(x, gy, a, dt, last=True))       # the input can tell the two tie rules apart
    print(f"maxpool2 {dt}: {ties} windows with a positive tie, forward and backward bit-exact")


@DTS
@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("shape", [(3, 3, 5), (1, 17, 19)])
def test_lpips_head_and_backward_with_zero_vectors(ops, shape, C, dt):
    """val per pixel, out per image (plain and accumulated) and the gradient with respect to f1, at P = 45 pixels (the grid tail (P + 3) / 4) and HW = 323
    (the reduction's 256-stride loop crosses once), with an all-zero f0, an all-zero f1 and both.  The gradient's reference is the analytic formula of the
    kernel's header (0 for its second term where ||f1|| = 0; torch autograd gives NaN there); away from the zero vectors autograd agrees with it in fp64.
    fp16: the zero-f1 pixel's correctly rounded gradient overflows (i1 = 1e10): +-inf exactly where the rounded reference is, and no NaN."""
    from enhancing import _C
    B, h, w = shape
    HW = h * w
    f, lin, gout = K.lpips_head_case(B, h, w, C, dt)
    fd, lind = _dev(f, dt), lin.cuda()
    val, vb, out, ob = K.lpips_head_ref(f, lin, B)
    ws, o = torch.full((B * HW,), NAN, device="cuda"), torch.full((B,), NAN, device="cuda")
    _C.lpips_head(fd, lind, B, HW, C, ws, o, False)
    r_v = assert_elementwise(ws.cpu().view(B, h, w), val, vb, f"lpips_head val {dt} C {C} {shape}")
    r_o = assert_elementwise(o.cpu(), out, ob, f"lpips_head out {dt} C {C} {shape}")
    ws.fill_(NAN)
    _C.lpips_head(fd, lind, B, HW, C, ws, o, True)
    r_a = assert_elementwise(o.cpu(), 2 * out, 2 * ob, f"lpips_head out accumulated {dt} C {C} {shape}")
    assert val[0, 0, 2] == 0 and ws.cpu().view(B, h, w)[0, 0, 2] == 0                   # both vectors zero: exactly 0
    # backward
    ref, bound, live = K.lpips_head_backward_ref(f, lin, gout, B, dt)
    auto = K.lpips_head_backward_autograd(f, lin, gout, B)
    assert torch.isnan(auto[~live]).all() and not torch.isnan(auto[live]).any()          # torch's behaviour at ||f1|| = 0, documented in the helper
    assert ((auto - ref)[live].abs() <= 1e-9 * ref[live].abs() + 1e-300).all(), "autograd and the analytic formula disagree away from the zero vectors"
    df = torch.full((B, h, w, C), NAN, dtype=dt, device="cuda")
    _C.lpips_head_backward(fd, lind, gout.cuda(), B, HW, C, df)
    got = _host(df)
    assert not torch.isnan(got).any(), "NaN in the head's gradient"
    want = ref.to(dt).float()
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf]), "+-inf must be exactly where the rounded reference is"
    assert bool(inf.any()) == (dt == F16) and not (inf & live).any()                      # fp16 overflows at the zero-f1 pixel, and only there
    fin = ~inf
    zero = torch.zeros_like(ref)
    r_g = assert_elementwise(torch.where(fin, got.double(), zero), torch.where(fin, ref, zero), bound.masked_fill(inf, 0.0), f"lpips_head_backward {dt} C {C} {shape}")
    assert not got[0, :, 0, 2].abs().sum()                                                # both zero: u = 0, no gradient
    print(f"lpips_head {dt} C {C} {shape}: max err / bound val {r_v:.3f}  out {r_o:.3f}  accumulated {r_a:.3f}  gradient {r_g:.3f} ({int(inf.sum())} +-inf)")


# ---------------------------------------------------------------------------------------------
# part 5: blur and minibatch stddev
# ---------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("pad", [(2, 2), (1, 1), (2, 1)])
@pytest.mark.parametrize("shape", [(3, 17, 23, 40), (1, 3, 2, 8)])
def test_blur_and_adjoint_per_element(ops, shape, pad, dt):
    """ops.blur with the asymmetric 4 x 4 kernel and its adjoint (autograd: the same kernel with the other tap order and the complementary padding), the
    second shape smaller than the kernel: one 16-bit rounding of an f32 sum of 16 products"""
    kern = K.blur_kernel4()
    c = K.blur_case(shape, pad, dt, kern)
    xd = _dev(c["x"], dt).requires_grad_(True)
    _poison(tuple(K.nhwc(c["y"]).shape), dt)
    y = ops.blur(xd, kern.cuda(), pad)
    r_y = assert_elementwise(_host(y.detach()), c["y"], c["y_bound"], f"blur {dt} {shape} pad {pad}")
    _poison(shape, dt)
    y.backward(_dev(c["gy"], dt))
    r_x = assert_elementwise(_host(xd.grad), c["dx"], c["dx_bound"], f"blur adjoint {dt} {shape} pad {pad}")
    print(f"blur {dt} {shape} pad {pad}: max err / bound forward {r_y:.3f}  adjoint {r_x:.3f}")


@DTS
@pytest.mark.parametrize("flip", [False, True])
def test_blur_3x3_on_the_generic_kernel(ops, flip, dt):
    """blur_nhwc_kernel with nine taps (the discriminator only ever runs four by four): both tap orders, asymmetric padding"""
    from enhancing import _C
    g = torch.Generator().manual_seed(9)
    kern = torch.rand(3, 3, generator=g) - 0.3
    B, H, W, C = 2, 7, 10, 24
    x = h16r(torch.randn(B, C, H, W, generator=g), dt)
    ref, mag = K.blur64(x.double(), kern, (2, 1), flip), K.blur64(x.double().abs(), kern.abs(), (2, 1), flip)
    _poison((B, H + 1, W + 1, C), dt)
    got = {}
    names = _launched(lambda: got.update(y=_C.blur_nhwc(_dev(x, dt), kern.cuda(), 2, 1, flip)))
    assert _ran(names, "blur_nhwc_kernel"), sorted(names)
    r = assert_elementwise(_host(got["y"]), ref, elem_bound(ref, mag, 9, dt), f"3 x 3 blur {dt} flip={flip}")
    print(f"blur 3 x 3 {dt} flip={flip}: max err / bound {r:.3f}")


STDDEV_CASES = [(8, 4, 512, None), (6, 3, 64, None), (16, 4, 512, None), (2, 2, 24, None), (6, 3, 64, 1)]      # test_conv_nhwc_gpu.STDDEV_CASES + a zero-variance slot


@DTS
@pytest.mark.parametrize("B,group,C,identical", STDDEV_CASES)
def test_minibatch_stddev_against_the_definition(ops, B, group, C, identical, dt):
    """the statistic and its backward against the reference project's definition restated in fp64 in loss_kernels_util.stddev_ref (not the package's own
    _stddev_torch); the copy is bit-exact, the padding zero; one case has a slot of identical samples (variance 0: sd = 1e-4, dx = g exactly)"""
    from enhancing import _C
    x, gy = K.stddev_case(B, group, C, dt, identical)
    Cp = K.pad8(C + 1)
    stat, stat_bound, dx, dx_bound = K.stddev_ref(x, gy, group, dt)
    xd = x.view(B, 4, 4, C).to(dt).cuda()
    _poison((B, 4, 4, Cp), dt)
    y = _C.minibatch_stddev_nhwc(xd, group, Cp).cpu()
    assert torch.equal(y[..., :C], x.view(B, 4, 4, C).to(dt)) and not y[..., C + 1:].float().abs().sum().item()
    s = y[..., C].float().reshape(B, 16)
    r_s = assert_elementwise(s, stat.view(B, 1).expand(B, 16), stat_bound.view(B, 1).expand(B, 16), f"minibatch stddev {dt} {(B, group, C)}")
    _poison((B, 4, 4, C), dt)
    g = _C.minibatch_stddev_nhwc_backward(xd, gy.view(B, 4, 4, Cp).to(dt).cuda(), group).float().cpu().view(B, 16, C)
    r_g = assert_elementwise(g, dx, dx_bound, f"minibatch stddev backward {dt} {(B, group, C)}")
    if identical is not None:
        n = B // group
        sl = torch.arange(B) % n == identical
        assert torch.equal(g[sl], gy[sl][..., :C]) and (stat[sl] - 1e-4).abs().max() < 1e-9
    print(f"minibatch stddev {dt} {(B, group, C)} identical slot {identical}: max err / bound statistic {r_s:.3f}  backward {r_g:.3f}")
