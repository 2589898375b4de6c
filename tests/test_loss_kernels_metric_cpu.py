"""The element bounds of tests/loss_kernels_util.py (the loss-network kernels: convolution epilogues, LPIPS kernels, blur, minibatch stddev) on a CPU
emulation, in the manner of tests/test_local_error_metric_cpu.py.  Proven here, without a GPU:

  * honest results — f32 arithmetic in torch, ONE rounding to the stored format — stay within every bound of tests/test_loss_kernels_elementwise_gpu.py
    in both formats (the worst ratio is printed), so the bounds are not too tight for an honest kernel;
  * local faults of the kind these kernels can have fail the element bound.  Next to each the output says whether the assertion the suite made until now
    (`rel <= 1.25 x floor`, or the test's own inputs) would have passed it.  The unwritten pixel at the first layer's real size is ASSERTED to pass it:
    that is the gap the element tests close;
  * the Cauchy-Schwarz magnitude that replaces a second fp64 convolution at real layer sizes is an upper bound of conv(|x|, |w|).
"""
import pytest
import torch
import torch.nn.functional as F

import loss_kernels_util as K
from util import assert_elementwise, elem_bound, floor16, h16r, rel

BF16, F16 = torch.bfloat16, torch.float16
DTS = pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "fp16"])
GLDS = (2, 9, 7, 64, 136, 3, 1, 1)                      # N = 136: one staged 128-column tile and one 8-column tile


def _flagged(bad, ref, bound, what, today: str):
    """the fault fails the element bound; prints today's verdict next to it"""
    with pytest.raises(AssertionError) as e:
        assert_elementwise(bad, ref, bound, what)
    print(f"{what}: element bound: fails ({str(e.value)[len(what) + 2:]}); today: {today}")


def _today(bad, ref, dt, limit=1.25):
    e, f = rel(bad, ref), floor16(ref, dt)
    return e <= limit * f, f"rel {e / f:.3f} x floor {'passes' if e <= limit * f else 'fails'} <= {limit} x floor"


# ---------------------------------------------------------------------------------------------
# honest results
# ---------------------------------------------------------------------------------------------
def _modes(case, dt):
    aux_dt, aux_sp = case["aux"].to(dt), K.crafted_aux(case["aux"], dt)
    act = dict(p0=K.SLOPE, p1=K.ACT_SCALE)
    return {"0": (0, dict(bias=case["bias"])), "1add": (1, dict(add=case["add"], aux_dt=aux_dt)), "1": (1, dict(aux_dt=aux_dt)),
            "1special": (1, dict(add=case["add"], aux_dt=aux_sp)), "2": (2, {}), "3": (3, dict(bias=case["bias"], **act)), "3nobias": (3, dict(**act)),
            "4": (4, dict(add=case["add"], p0=K.ALPHA))}


@DTS
def test_honest_epilogues_are_within_the_element_bound(dt):
    case = K.conv_case(*GLDS, dt)
    worst = {}
    for m, (mode, args) in _modes(case, dt).items():
        ref, bound = K.epilogue_ref(case, mode, **args)
        worst[m] = assert_elementwise(K.epilogue_emulated(case, mode, **args), ref, bound, f"emulated mode {m} {dt}")
    print(f"honest epilogues {dt}: err / bound " + "  ".join(f"{m} {v:.3f}" for m, v in worst.items()))
    assert max(worst.values()) <= 1.0 and worst["2"] >= 0.5          # tight: half an ulp at the bottom of a binade


@DTS
def test_special_aux_values_gate_like_torch(dt):
    """the six special values and the mask torch evaluates for them on the CPU; the kernel's bit test (magnitude bits nonzero and sign bit clear) is the same
    predicate, restated here on the bit patterns"""
    sp = K.special_values(dt)
    assert (sp > 0).tolist() == [False, False, True, False, True, False]
    bits = sp.view(torch.int16).int() & 0xffff
    assert (((bits & 0x7fff) != 0) & ((bits & 0x8000) == 0)).tolist() == (sp > 0).tolist()
    assert sp.float().abs().tolist()[2] > 0 and sp.float().abs().tolist()[4] == (2.0 ** -126 if dt == BF16 else 2.0 ** -14)


@DTS
@pytest.mark.parametrize("normalize", [True, False])
def test_honest_vgg_conv1_is_within_the_element_bound(normalize, dt):
    c = K.vgg_conv1_case(2, 5, 11, normalize, dt)
    r_f = assert_elementwise(K.vgg_conv1_emulated(c, normalize, dt), c["ref"], c["bound"], f"emulated vgg_conv1 {dt}")
    a = 2.0 if normalize else 1.0
    it = c["img"].clone().requires_grad_(True)
    xs = ((a * it + (-1.0 if normalize else 0.0)) - K.VGG_SHIFT.view(1, 3, 1, 1)) * (1.0 / K.VGG_SCALE).view(1, 3, 1, 1)
    F.conv2d(xs, c["w"], padding=1).backward(c["gpre"])
    r_b = assert_elementwise(it.grad, c["dimg"], c["dimg_bound"], f"emulated vgg_conv1 backward {dt}")
    print(f"honest vgg_conv1 {dt} normalize={normalize}: err / bound forward {r_f:.3f}, image gradient {r_b:.4f}")


@DTS
@pytest.mark.parametrize("C", [64, 512])
def test_honest_lpips_head_is_within_the_element_bound(C, dt):
    B, h, w = 3, 3, 5
    f, lin, gout = K.lpips_head_case(B, h, w, C, dt)
    val, vb, out, ob = K.lpips_head_ref(f, lin, B)
    v32, o32 = K.lpips_head_emulated(f, lin, B)
    r_v, r_o = assert_elementwise(v32, val, vb, f"emulated lpips_head val {dt}"), assert_elementwise(o32, out, ob, f"emulated lpips_head out {dt}")
    ref, bound, live = K.lpips_head_backward_ref(f, lin, gout, B, dt)
    got = K.lpips_head_backward_emulated(f, lin, gout, B, dt).double()
    inf = torch.isinf(ref.to(dt).float())
    assert torch.equal(torch.isinf(got), inf) and not torch.isnan(got).any() and bool(inf.any()) == (dt == F16)
    zero = torch.zeros_like(ref)
    r_g = assert_elementwise(torch.where(inf, zero, got), torch.where(inf, zero, ref), bound.masked_fill(inf, 0.0), f"emulated lpips_head backward {dt}")
    auto = K.lpips_head_backward_autograd(f, lin, gout, B)
    assert torch.isnan(auto[~live]).all() and ((auto - ref)[live].abs() <= 1e-9 * ref[live].abs() + 1e-300).all()      # NaN at ||f1|| = 0, the formula elsewhere
    print(f"honest lpips_head {dt} C {C}: err / bound val {r_v:.3f}  out {r_o:.3f}  gradient {r_g:.3f}")


@DTS
@pytest.mark.parametrize("pad", [(2, 2), (2, 1)])
def test_honest_blur_is_within_the_element_bound(pad, dt):
    kern = K.blur_kernel4()
    c = K.blur_case((3, 17, 23, 40), pad, dt, kern)
    xr = c["x"].clone().requires_grad_(True)
    y = K.blur64(xr, kern, pad)
    y.backward(c["gy"])
    r_y = assert_elementwise(h16r(y.detach(), dt), c["y"], c["y_bound"], f"emulated blur {dt}")
    r_x = assert_elementwise(h16r(xr.grad, dt), c["dx"], c["dx_bound"], f"emulated blur adjoint {dt}")
    print(f"honest blur {dt} pad {pad}: err / bound forward {r_y:.3f}  adjoint {r_x:.3f}")


@DTS
@pytest.mark.parametrize("B,group,C,identical", [(8, 4, 512, None), (6, 3, 64, None), (2, 2, 24, None), (6, 3, 64, 1)])
def test_honest_minibatch_stddev_is_within_the_element_bound(B, group, C, identical, dt):
    x, gy = K.stddev_case(B, group, C, dt, identical)
    stat, stat_bound, dx, dx_bound = K.stddev_ref(x, gy, group, dt)
    s16, g16 = K.stddev_emulated(x, gy, group, dt)
    r_s = assert_elementwise(s16, stat, stat_bound, f"emulated stddev {dt}")
    r_g = assert_elementwise(g16, dx, dx_bound, f"emulated stddev backward {dt}")
    # the definition agrees with autograd of the same expression in fp64
    xt = x.double().clone().requires_grad_(True)
    n = B // group
    sd = torch.sqrt(xt.view(group, n, 16, C).var(0, unbiased=False) + K.f32(1e-8)).mean((1, 2))
    ((sd.repeat(group).view(B, 1) * gy.double()[..., C]).sum() + (xt * gy.double()[..., :C]).sum()).backward()
    assert (xt.grad - dx).abs().max() <= 1e-9 * dx.abs().max()
    print(f"honest minibatch stddev {dt} {(B, group, C)} identical slot {identical}: err / bound statistic {r_s:.3f}  backward {r_g:.3f}")


@DTS
def test_maxpool_case_holds_positive_ties_and_tells_the_tie_rules_apart(dt):
    x, gy, add = K.maxpool_case(dt)
    assert K.positive_ties(x) >= 64 and K.positive_ties(x[:, :8]) == x.shape[0] * 8 * (x.shape[2] // 2) * (x.shape[3] // 2)
    # the random post-ReLU data the other op test draws: positive ties only by chance
    g = torch.Generator().manual_seed(3)
    rnd = h16r(torch.randn(2, 64, 8, 12, generator=g), dt).clamp_min(0)
    first, last = K.maxpool_backward_ref(x, gy, add, dt), K.maxpool_backward_ref(x, gy, add, dt, last=True)
    r_first, r_last = K.maxpool_backward_ref(rnd, gy, add, dt), K.maxpool_backward_ref(rnd, gy, add, dt, last=True)
    n_bad, n_rnd = int((first != last).sum()), int((r_first != r_last).sum())
    today = rel(r_last.float(), r_first.float()) <= 1e-6
    print(f"max-pool tie routed to the LAST maximum {dt}: element bound (bit equality): fails on {n_bad} elements of the crafted input; today: "
          f"{K.positive_ties(rnd)} of 3072 random windows hold a positive tie, {n_rnd} elements differ, rel <= 1e-6 {'passes' if today else 'fails'}")
    assert n_bad >= 2 * 64


# ---------------------------------------------------------------------------------------------
# injected faults
# ---------------------------------------------------------------------------------------------
@DTS
def test_bias_of_the_wrong_column_group_in_the_last_partial_tile_is_flagged(dt):
    """N = 136: columns 128..135 are the 8-column tail of the second column tile; the fault adds bias[0..7] (the tile's first group) instead of bias[128..135]"""
    case = K.conv_case(*GLDS, dt)
    ref, bound = K.epilogue_ref(case, 3, bias=case["bias"], p0=K.SLOPE, p1=K.ACT_SCALE)
    wrong = case["bias"].clone()
    wrong[128:] = case["bias"][:8]
    bad = K.epilogue_emulated(case, 3, bias=wrong, p0=K.SLOPE, p1=K.ACT_SCALE)
    _flagged(bad, ref, bound, f"bias of the wrong 8-column group in the last partial column tile {dt}", _today(bad, ref, dt)[1])


def test_unwritten_pixel_at_the_first_layers_real_size_passes_the_norm_and_is_flagged():
    """2 x 256 x 256 x 128 bf16 (the discriminator's first layer, 16.7 M elements): a random tensor as the exact result, its rounding as the honest output, one
    pixel x 8 channels never written (zeros).  The norm moves by far less than the 25 % margin: the fault PASSES 1.25 x floor, which is the point."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(2 * 256 * 256, 128, generator=g)
    bad = h16r(ref, BF16)
    bad[70000, 40:48] = 0
    ok, verdict = _today(bad, ref, BF16)
    assert ok, verdict
    bound = elem_bound(ref, torch.zeros_like(ref), 8, BF16)                # the rounding term alone
    _flagged(bad, ref, bound, "one pixel x 8 channels unwritten in 2 x 256 x 256 x 128 bf16", verdict)


@DTS
def test_mode_1_gate_taken_as_aux_ge_0_is_flagged(dt):
    case = K.conv_case(*GLDS, dt)
    aux_dt = case["aux"].to(dt)
    ref, bound = K.epilogue_ref(case, 1, aux_dt=aux_dt)
    bad = h16r(F.conv2d(case["x"], case["ws"], padding=1) * (aux_dt >= 0), dt)
    _flagged(bad, ref, bound, f"mode-1 gate aux >= 0 on a post-ReLU aux {dt}", _today(bad, ref, dt)[1] + "; the op tests draw aux from randn, where "
             f"aux >= 0 and aux > 0 differ on {int((h16r(torch.randn(10000, generator=torch.Generator().manual_seed(1)), dt) == 0).sum())} of 10000 values: passes")


@DTS
def test_one_pixel_left_out_of_an_lpips_head_mean_is_flagged(dt):
    B, h, w, C = 1, 17, 19, 64
    f, lin, gout = K.lpips_head_case(B, h, w, C, dt)
    val, vb, out, ob = K.lpips_head_ref(f, lin, B)
    v32, _ = K.lpips_head_emulated(f, lin, B)
    v32 = v32.clone()
    v32[0, 16, 18] = 0                                                      # the last pixel: past a ragged grid tail or stride loop
    bad = v32.sum((1, 2)) / (h * w)
    e = rel(bad, out)
    _flagged(bad, out, ob, f"one pixel's val left out of an LPIPS head mean, HW = 323 {dt}", f"rel {e:.2e} {'passes' if e <= 1e-5 else 'fails'} <= 1e-5 "
             "(and the op test's HW = 24 never reaches a ragged tail)")


@DTS
def test_swapped_h_and_w_in_vgg_conv1_is_flagged(dt):
    c = K.vgg_conv1_case(2, 5, 11, True, dt)
    bad = K.vgg_conv1_emulated(c, True, dt, swap_hw=True)
    _flagged(bad, c["ref"], c["bound"], f"H and W swapped in vgg_conv1's pixel decomposition at 5 x 11 {dt}",
             "the other tests run 16 x 16 and 256 x 256 only, where the swap is the identity: passes")


def test_cauchy_schwarz_magnitude_is_an_upper_bound():
    """loss_kernels_util.conv_mag_upper >= conv(|x|, |w|) at every output, padded borders and stride 2 included"""
    for geom in [(2, 9, 7, 24, 72, 3, 1, 1), (2, 15, 15, 40, 64, 1, 2, 0), (1, 17, 17, 32, 64, 3, 2, 0)]:
        case = K.conv_case(*geom, BF16)
        up = K.conv_mag_upper(case["x"], case["ws"], geom[5], geom[6], geom[7])
        assert up.shape == case["mag"].shape and bool((up >= case["mag"]).all())
        print(f"Cauchy-Schwarz magnitude {geom}: upper / exact between {(up / case['mag']).min().item():.2f} and {(up / case['mag']).max().item():.2f}")
