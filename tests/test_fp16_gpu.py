"""fp16 MFMA operands (ENH_DT_F16): the one-pass precision that meets north_star's 1e-3 clause, and the reference's own --use_amp dtype
(/root/reference/main.py:25,52: Lightning precision=16 = fp16 autocast + GradScaler).

Op level: every kernel that reads or writes 16-bit operands is a template over the operand type (csrc/common.h BF16 | F16); the fp16 instantiations
are checked here against fp64 products of the SAME fp16-representable operands, with the tolerance classes of tests/test_ops_gpu.py:
  * f32 outputs <= 1e-5 (only the f32 summation order differs);
  * fp16 outputs <= 1.15 x the fp16 rounding floor of the exact result (2^-12 worst case, ~2e-4 rms for Gaussian data: 8x below bf16's 1.66e-3);
  * persistent / one-tile kernel families and tile schedules: bit-identical.
Model level (BASELINE config 2 / 4 / 5 towers, B = 2, vs the fp32 CPU oracle with identical fp32 master weights): the bounds are the tolerance itself —
h <= 1e-3, xrec (same codes) <= 1e-3 — plus end-to-end code match-rates and one training step's gradients through the loss-scaled fp16 backward.
"""
import copy

import numpy as np
import pytest
import torch

from util import floor16, h16r, rel

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
F32_TOL = 1e-5


def f16r(x):
    return h16r(x, F16)


def f16_floor(ref):
    """relative Frobenius error of merely rounding the exact result to fp16"""
    return floor16(ref, F16)


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _mk(shape, g, scale=1.0):
    return f16r(torch.randn(*shape, generator=g) * scale)


# ---------------------------------------------------------------------------------------------
# conversions: RNE packing (v_cvt_pk_f16_f32, never the round-toward-zero v_cvt_pkrtz), widening, subnormals
# ---------------------------------------------------------------------------------------------
def test_cast_is_round_to_nearest_even_incl_subnormals_and_overflow(C):
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-5, torch.randn(4096, generator=g) * 1e-7,   # normals, subnormals, below half the smallest subnormal
                   torch.tensor([65504.0, 65519.9, 65520.0, 1e6, -1e6, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 0.0, -0.0])])
    x = torch.cat([x, torch.zeros((-x.numel()) % 4)])
    y = torch.empty(x.numel(), dtype=F16, device="cuda")
    C.cast_bf16(x.cuda(), y)
    want = x.to(F16)          # torch's CPU cast: IEEE round-to-nearest-even, overflow -> inf
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16)), "f32 -> fp16 packing must be round-to-nearest-even, bit for bit"
    yb = torch.empty(x.numel(), dtype=BF16, device="cuda")
    C.cast_bf16(x.cuda(), yb)
    assert torch.equal(yb.cpu().view(torch.int16), x.to(BF16).view(torch.int16))


def test_mixed_operand_formats_in_one_call_are_refused(C):
    a = torch.zeros(256, 64, dtype=F16, device="cuda")
    b = torch.zeros(256, 64, dtype=BF16, device="cuda")
    with pytest.raises(RuntimeError, match="all be bf16 or all be fp16"):
        C.gemm(a, b, 256, 256, 64, out_f32=torch.empty(256, 256, device="cuda"))
    L = C.lib()
    rc = L.enh_cast_f32_h16(None, None, 4, 7, None)
    assert rc != 0 and b"dtype" in L.enh_last_error()


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (1000, 192, 768), (136, 32, 64), (384, 768, 3072), (128, 2304, 32),
                                   (520, 768, 192), (768, 512, 2048), (1288, 264, 64), (1024, 1280, 832), (4096, 2304, 768), (768, 768, 8192)])
def test_gemm_layouts_fp16(C, ta, tb, M, N, K):
    if ta and M % 8:
        pytest.skip("trans_a needs M % 8 == 0")
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A, B = _mk((M, K), g), _mk((N, K), g)
    ref = A.double() @ B.double().t()
    a = (A.t().contiguous() if ta else A).to(F16).cuda()
    b = (B.t().contiguous() if tb else B).to(F16).cuda()
    out = torch.full((M, N), float("nan"), device="cuda")
    out16 = torch.empty(M, N, dtype=F16, device="cuda")
    C.gemm(a, b, M, N, K, trans_a=ta, trans_b=tb, out_f32=out, out_bf16=out16)
    assert rel(out, ref) <= F32_TOL, f"ta={ta} tb={tb}"
    assert rel(out16.float(), ref) <= 1.15 * f16_floor(ref) + 1e-6
    # accumulate-into-f32 (the weight-gradient form; split-K with the deterministic workspace where the planner splits)
    acc = torch.ones(M, N, device="cuda")
    C.gemm(a, b, M, N, K, trans_a=ta, trans_b=tb, accumulate=True, out_f32=acc)
    assert rel(acc, ref + 1.0) <= F32_TOL


@pytest.mark.parametrize("kernel_shape", [(512, 384, 256, 128), (1024, 768, 192, 256), (2048, 768, 768, 1024)])
def test_gemm_epilogues_fp16(C, kernel_shape):
    g = torch.Generator().manual_seed(5)
    M, N, K, T = kernel_shape
    A, B = _mk((M, K), g, 0.5), _mk((N, K), g, 0.1)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    pos = torch.randn(T, N, generator=g)
    a, b = A.to(F16).cuda(), B.to(F16).cuda()
    base = A.double() @ B.double().t()
    o16 = torch.empty(M, N, dtype=F16, device="cuda")
    C.gemm(a, b, M, N, K, bias=bias.cuda(), act=C.ACT_TANH, out_bf16=o16)
    t = torch.tanh(base + bias.double())
    assert rel(o16.float(), t) <= 1.15 * f16_floor(t) + 2e-7 / t.abs().mean().item()      # (the epilogue's tanh: exp2 + rcp, absolute error ~1e-7)
    x = res.clone().cuda()
    C.gemm(a, b, M, N, K, bias=bias.cuda(), res=x, res_rows=M, out_f32=x)
    assert rel(x, base + bias.double() + res.double()) <= F32_TOL
    o = torch.empty(M, N, device="cuda")
    C.gemm(a, b, M, N, K, bias=bias.cuda(), res=pos.cuda(), res_rows=T, out_f32=o)
    assert rel(o, base + bias.double() + pos.double().repeat(M // T, 1)) <= F32_TOL
    h = f16r(torch.tanh(torch.randn(M, N, generator=g)))
    C.gemm(a, b, M, N, K, act=C.ACT_DTANH, aux=h.to(F16).cuda(), out_bf16=o16)
    d = base * (1 - h.double() ** 2)
    assert rel(o16.float(), d) <= 1.15 * f16_floor(d) + 1e-6


@pytest.mark.parametrize("kind", ["fwd", "dgrad", "fwd_tanh", "dgrad_dtanh", "fwd_res", "fwd_f32"])
def test_persistent_gemm_is_bitwise_the_one_tile_kernel_fp16(C, kind):
    """the fp16 instantiations of gemm_w256p / gemm_w256r against gemm_w256 (same MFMA sequence per output element): bit-identical, both tile schedules"""
    L = C.lib()
    g = torch.Generator().manual_seed(31)
    tb = kind.startswith("dgrad")
    try:
        for (m, n, k) in ((1024, 768, 192), (256 * 37, 2304, 448), (256 * 50, 768, 384), (8192, 3072, 768)):
            A, B = _mk((m, k), g, 0.5), _mk((n, k), g, 0.1)
            a = A.to(F16).cuda()
            b = (B.t().contiguous() if tb else B).to(F16).cuda()
            kw = dict(trans_b=tb)
            if kind in ("fwd", "dgrad"):
                out = torch.empty(m, n, dtype=F16, device="cuda"); kw["out_bf16"] = out
            elif kind == "fwd_f32":
                out = torch.empty(m, n, device="cuda"); kw["out_f32"] = out
            elif kind == "fwd_tanh":
                out = torch.empty(m, n, dtype=F16, device="cuda"); kw.update(out_bf16=out, bias=torch.randn(n, generator=g).cuda(), act=C.ACT_TANH)
            elif kind == "fwd_res":
                out = torch.empty(m, n, device="cuda"); kw.update(out_f32=out, bias=torch.randn(n, generator=g).cuda(), res=torch.randn(m, n, generator=g).cuda(), res_rows=m)
            else:
                out = torch.empty(m, n, dtype=F16, device="cuda")
                kw.update(out_bf16=out, act=C.ACT_DTANH, aux=torch.tanh(torch.randn(m, n, generator=g)).to(F16).cuda())
            assert L.enh_gemm_set_kernel(7) == 0
            out.zero_(); C.gemm(a, b, m, n, k, **kw); torch.cuda.synchronize(); ref = out.clone()
            for fam in (8, 9):
                for dyn in (0, 1):
                    assert L.enh_gemm_set_kernel(fam) == 0 and L.enh_gemm_set_scheduler(dyn) == 0
                    out.fill_(7.0); C.gemm(a, b, m, n, k, **kw); torch.cuda.synchronize()
                    assert torch.equal(out, ref), f"family {fam} dyn {dyn} {kind} M={m} N={n} K={k}: {(out != ref).sum().item()} elements differ"
            if kind == "fwd" and m == 1024:
                e = A.double() @ B.double().t()
                assert rel(out.float(), e) <= 1.15 * f16_floor(e) + 1e-6
    finally:
        L.enh_gemm_set_kernel(-1)
        L.enh_gemm_set_scheduler(1)


@pytest.mark.parametrize("M,N,K", [(2048, 768, 192), (256 * 37, 3072, 768), (1000, 192, 256)])
def test_gemm_dtanh_with_fused_bias_gradient_fp16(C, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    A, B = _mk((M, K), g, 0.5), _mk((K, N), g, 0.1)     # B stored [K][N]: trans_b (the input-gradient layout)
    h = torch.tanh(torch.randn(M, N, generator=g)).to(F16)
    a, b, hd = A.to(F16).cuda(), B.to(F16).cuda(), h.cuda()
    out = torch.empty(M, N, dtype=F16, device="cuda")
    cs = torch.zeros(N, device="cuda")
    C.gemm_dtanh_colsum(a, b, M, N, K, hd, out, cs, trans_b=True, accumulate_colsum=False)
    ref16 = torch.empty(M, N, dtype=F16, device="cuda")
    C.gemm(a, b, M, N, K, trans_b=True, act=C.ACT_DTANH, aux=hd, out_bf16=ref16)
    assert torch.equal(out, ref16)
    assert rel(cs, out.double().sum(0)) <= F32_TOL
    d = (A.double() @ B.double()) * (1 - h.double() ** 2)
    assert rel(out.float(), d) <= 1.15 * f16_floor(d) + 1e-6


# ---------------------------------------------------------------------------------------------
# LayerNorm, column sums, patch movement, quantizer copies, optimizer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", [(1027, 768), (64, 128), (130, 1280), (33, 2048)])
def test_layernorm_fwd_bwd_fp16(C, M, D):
    g = torch.Generator().manual_seed(M + D)
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    w = 1 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    dy16 = (torch.randn(M, D, generator=g)).to(F16)
    dres = torch.randn(M, D, generator=g)
    xt, wt, bt = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xt, (D,), wt, bt, 1e-5)
    y.backward(dy16.float())
    xd = x.cuda()
    y16 = torch.empty(M, D, dtype=F16, device="cuda"); y32 = torch.empty(M, D, device="cuda")
    mean = torch.empty(M, device="cuda"); rstd = torch.empty(M, device="cuda")
    C.layernorm_forward(xd, w.cuda(), b.cuda(), 1e-5, y16, y32, mean, rstd)
    assert rel(y32, y) <= F32_TOL
    assert torch.equal(y16.cpu(), y32.cpu().to(F16)), "the fp16 operand copy is the RNE rounding of the f32 result"
    dx = torch.empty(M, D, device="cuda"); dx16 = torch.empty(M, D, dtype=F16, device="cuda")
    dw = torch.zeros(D, device="cuda"); db = torch.zeros(D, device="cuda"); dxs = torch.zeros(D, device="cuda")
    C.layernorm_backward(dy16.cuda(), xd, w.cuda(), mean, rstd, dres.cuda(), dx, dx16, dw, db, dxs)
    assert rel(dx, xt.grad + dres) <= F32_TOL and rel(dxs, (xt.grad + dres).double().sum(0)) <= F32_TOL
    assert rel(dw, wt.grad) <= F32_TOL and rel(db, bt.grad) <= F32_TOL
    assert torch.equal(dx16.cpu(), dx.cpu().to(F16))


def test_colsum_patchify_unpatchify_vq_copies_fp16(C):
    import vitvq_oracle as O
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3000, 768, generator=g).to(F16)
    out = torch.empty(768, device="cuda")
    C.colsum(x.cuda(), 3000, 768, out)
    assert rel(out, x.double().sum(0)) <= F32_TOL
    x2 = torch.randn(700, 192, generator=g).to(F16)       # narrow variant (N % 8 == 0 but ld not 16-byte-friendly is covered by the bf16 tests)
    out2 = torch.empty(192, device="cuda")
    C.colsum(x2.cuda(), 700, 192, out2)
    assert rel(out2, x2.double().sum(0)) <= F32_TOL
    img = torch.rand(2, 3, 64, 64, generator=g)
    p16 = torch.empty(2 * 64, 192, dtype=F16, device="cuda"); pb = torch.empty(2 * 64, 192, dtype=BF16, device="cuda")
    C.patchify(img.cuda(), 8, p16); C.patchify(img.cuda(), 8, pb)
    ref = img.view(2, 3, 8, 8, 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(128, 192)
    assert torch.equal(p16.cpu(), ref.to(F16)) and torch.equal(pb.cpu(), ref.to(BF16))
    pix = torch.randn(128, 192, generator=g)
    xrec = torch.empty(2, 3, 64, 64, device="cuda"); sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    d16 = torch.empty(128, 192, dtype=F16, device="cuda")
    S = 65536.0
    C.unpatchify_loss(pix.cuda(), img.cuda(), 2, 3, 64, 64, 8, 0.0, 1.0, xrec, sums, d16, grad_scale=torch.full((1,), S, device="cuda"))      # the loss scale as a DEVICE scalar
    rec = pix.view(2, 8, 8, 3, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(2, 3, 64, 64)
    gref = (2 * (rec - img) / img.numel() * S).view(2, 3, 8, 8, 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(128, 192)
    assert rel(d16.float(), gref) <= 1.15 * f16_floor(gref) + 1e-6
    assert abs(sums[1].item() / img.numel() - ((rec - img) ** 2).mean().item()) <= 1e-6      # the loss VALUE is not scaled
    z, E, gq = O.make_vq_inputs(5, 512, 1024)
    zq, zq16, idx, loss = C.vq_forward(z.cuda(), E.cuda(), 0.25, 1, True, h16=F16)
    assert zq16.dtype == F16 and torch.equal(zq16.cpu(), zq.cpu().to(F16))
    dE = torch.zeros(1024, 32, device="cuda")
    dz, dz16 = C.vq_backward(z.cuda(), E.cuda(), idx, gq.cuda(), 0.7, None, 0.25, 1, False, True, dE, h16=F16)
    assert torch.equal(dz16.cpu(), dz.cpu().to(F16))
    o, o16 = C.vq_lookup(E.cuda(), idx, True, h16=F16)
    assert torch.equal(o16.cpu(), o.cpu().to(F16))


def test_adamw_fp16_shadow_and_the_nonfinite_skip(C):
    import vitvq_oracle as O
    g = torch.Generator().manual_seed(9)
    n = 4096 * 5 + 8
    p = torch.randn(n, generator=g); gr = torch.randn(n, generator=g) * 1e-3
    m, v = torch.zeros(n), torch.zeros(n)
    pd, gd, md, vd = p.clone().cuda(), (gr * 65536.0).cuda(), m.clone().cuda(), v.clone().cuda()
    p16 = torch.zeros(n, dtype=F16, device="cuda")
    flag = torch.zeros(1, device="cuda")
    C.nonfinite_flag(gd, flag)
    assert flag.item() == 0.0
    C.adamw_step(pd, gd, md, vd, p16, 1, 1e-3, grad_scale=1.0 / 65536.0, skip_flag=flag)
    O.adamw_step(p, gr, m, v, 1, 1e-3)
    assert rel(pd, p) <= 1e-6 and rel(md, m) <= 1e-6 and rel(vd, v) <= 1e-6
    assert torch.equal(p16.cpu(), pd.cpu().to(F16)), "the fp16 operand shadow is the RNE image of the updated master"
    # an inf (or nan) anywhere in the flat gradient drops the step: nothing is written
    before = [t.clone() for t in (pd, md, vd, p16)]
    for bad, pos in ((float("inf"), 17), (float("nan"), n - 3), (-float("inf"), 4096 * 3)):
        gd2 = gd.clone(); gd2[pos] = bad
        flag.zero_()
        C.nonfinite_flag(gd2, flag)
        assert flag.item() == 1.0
        C.adamw_step(pd, gd2, md, vd, p16, 2, 1e-3, grad_scale=1.0 / 65536.0, skip_flag=flag)
        for t, b in zip((pd, md, vd, p16), before):
            assert torch.equal(t, b)
    # the same step with the unscale folded in through a device scalar (what the engine passes): identical bits to the host-float form
    p2, m2, v2 = p.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()      # (p is the oracle's post-step-1 state: any starting point will do)
    p3, m3, v3 = p2.clone(), m2.clone(), v2.clone()
    C.adamw_step(p2, gd, m2, v2, None, 1, 1e-3, grad_scale=1.0 / 65536.0)
    C.adamw_step(p3, gd, m3, v3, None, 1, 1e-3, grad_scale=1.0, loss_scale=torch.full((1,), 65536.0, device="cuda"))
    assert torch.equal(p2, p3) and torch.equal(m2, m3) and torch.equal(v2, v3)


def test_loss_scale_update_is_gradscaler_update(C):
    """enh_loss_scale_update against torch.cuda.amp.GradScaler's rule (growth 2, backoff 0.5, interval 3 here): overflow halves and resets the tracker, `interval`
    clean steps in a row double; the scale stays inside [1, 2^24]"""
    scale = torch.full((1,), 65536.0, device="cuda"); trk = torch.zeros(1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, device="cuda")
    ref_s, ref_t, seq = 65536.0, 0, [0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]
    for bad in seq:
        flag.fill_(float(bad))
        C.loss_scale_update(scale, flag, trk, 2.0, 0.5, 3)
        if bad:
            ref_s, ref_t = ref_s * 0.5, 0
        else:
            ref_t += 1
            if ref_t >= 3:
                ref_s, ref_t = ref_s * 2.0, 0
        assert scale.item() == ref_s and trk.item() == ref_t, (scale.item(), ref_s, trk.item(), ref_t)
    scale.fill_(2.0 ** 24); flag.zero_(); trk.fill_(2)
    C.loss_scale_update(scale, flag, trk, 2.0, 0.5, 3)
    assert scale.item() == 2.0 ** 24
    scale.fill_(1.0); flag.fill_(1.0)
    C.loss_scale_update(scale, flag, trk, 2.0, 0.5, 3)
    assert scale.item() == 1.0
    C.loss_scale_update(scale, flag.zero_(), trk, 2.0, 0.5, 0)      # interval 0: never grows
    assert scale.item() == 1.0 and trk.item() == 0


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def _attn_ref(q, k, v, scale):
    s = torch.einsum("bhnd,bhmd->bhnm", q, k) * scale
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhnm,bhmd->bhnd", p, v), torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize("B,N,H,pre", [(2, 256, 3, True), (1, 1024, 12, True), (2, 128, 2, False), (1, 1024, 16, True)])
def test_attention_forward_backward_fp16(C, B, N, H, pre):
    """fused attention on fp16 operands vs fp64 on the SAME fp16-representable q | k | v (and dO): forward <= 1.5 x the fp16 floor of the exact output
    (the probabilities are rounded to fp16 before P V: bf16 measured 1.10 x its floor), lse exact to f32; gradients (two chained fp16 roundings, S and dS
    recomputed from rounded P) within 2e-3 — bf16's bound for the same test is 1e-2."""
    g = torch.Generator().manual_seed(B * 1000 + N + H)
    scale = 64 ** -0.5
    alpha = scale * 1.4426950408889634
    qkv = torch.randn(B, N, 3 * H * 64, generator=g)
    qkv = f16r(qkv)
    q, k, v = (t.reshape(B, N, H, 64).permute(0, 2, 1, 3).double() for t in qkv.split(H * 64, dim=-1))
    stored = qkv.clone()
    if pre:      # the engine's convention: the q third holds q * scale * log2(e), rounded once
        stored[..., :H * 64] = f16r(qkv[..., :H * 64] * alpha)
        q = (stored[..., :H * 64] / alpha).reshape(B, N, H, 64).permute(0, 2, 1, 3).double()
    qd = stored.to(F16).cuda()
    out = torch.empty(B, N, H * 64, dtype=F16, device="cuda"); lse = torch.empty(B, H, N, device="cuda")
    C.attention_forward(qd, B, N, H, scale, out, lse, q_prescaled=pre)
    qt, kt, vt = q.clone().requires_grad_(True), k.clone().requires_grad_(True), v.clone().requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qt, kt, vt, scale)
    o_flat = o_ref.permute(0, 2, 1, 3).reshape(B, N, H * 64)
    e_o = rel(out.float(), o_flat)
    assert e_o <= 1.5 * f16_floor(o_flat.detach()) + 1e-6, (e_o, f16_floor(o_flat.detach()))
    assert rel(lse, lse_ref) <= 1e-5
    do = f16r(torch.randn(B, N, H * 64, generator=g) * 0.5)
    o_flat.backward(do.double())
    dqkv = torch.empty(B, N, 3 * H * 64, dtype=F16, device="cuda"); delta = torch.empty(B, H, N, device="cuda")
    C.attention_backward(qd, out, do.to(F16).cuda(), lse, B, N, H, scale, dqkv, delta, q_prescaled=pre)
    dq, dk, dv = (t.float().cpu().reshape(B, N, H, 64).permute(0, 2, 1, 3) for t in dqkv.split(H * 64, dim=-1))
    eq, ek, ev = rel(dq, qt.grad), rel(dk, kt.grad), rel(dv, vt.grad)
    print(f"fp16 attention B={B} N={N} H={H} pre={pre}: out {e_o:.2e} (floor {f16_floor(o_flat.detach()):.2e})  dq {eq:.2e} dk {ek:.2e} dv {ev:.2e}")
    assert max(eq, ek, ev) <= 2e-3, (eq, ek, ev)
    # bit-reproducible from launch to launch
    out2 = torch.empty_like(out); lse2 = torch.empty_like(lse); dqkv2 = torch.empty_like(dqkv)
    C.attention_forward(qd, B, N, H, scale, out2, lse2, q_prescaled=pre)
    C.attention_backward(qd, out, do.to(F16).cuda(), lse, B, N, H, scale, dqkv2, delta, q_prescaled=pre)
    assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)


# ---------------------------------------------------------------------------------------------
# model level: the tolerance of north_star on the single-pass fp16 path
# ---------------------------------------------------------------------------------------------
from test_parity_base_gpu import BASE, LARGE, _spread_codebook      # noqa: E402  (the benchmarked configurations and the trained-like codebook)

# (max residual-stream error over the layers, h, xrec downstream of the same codes, worst parameter gradient, minimum end-to-end code match-rate)
# h / xrec: the north_star clause itself (1e-3).  The others: regression bounds at 1.15 x the values measured on MI355X (profiles/r06_parity_fp16.txt).
FP16_BOUNDS = {
    "base":        (1e-3, 1e-3, 1e-3, 2.5e-3, 0.995),
    "rq4":         (1e-3, 1e-3, 1e-3, 2.5e-3, 0.990),
    "base_spread": (1e-3, 1e-3, 1e-3, 2.5e-3, 0.985),
    "rq4_spread":  (1e-3, 1e-3, 1e-3, 2.5e-3, 0.975),
    "large":       (1e-3, 1e-3, 1e-3, 2.5e-3, 0.995),
}


def _build16(cfg, P, precision="fp16"):
    from enhancing.modules.stage1.vitvqgan import ViTVQ
    from enhancing.utils.general import AttrDict
    loss = {"target": "enhancing.losses.vqperceptual.VQLPIPS",
            "params": dict(codebook_weight=1.0, loglaplace_weight=0.0, loggaussian_weight=1.0, perceptual_weight=0.0)}
    m = ViTVQ("image", cfg["image_size"], cfg["patch_size"], AttrDict.wrap(cfg["encoder"]), AttrDict.wrap(cfg["decoder"]),
              AttrDict.wrap(cfg["quantizer"]), AttrDict.wrap(loss))
    m.precision = precision
    m.load_state_dict(P, strict=True)
    assert m.engine.precision == precision and m.engine.adt == (F16 if precision == "fp16" else BF16)
    return m


def _run_fp16_case(label, case, cfg, B, seed, spread=False, min_distinct=0):
    import os
    import vitvq_oracle as O
    torch.set_num_threads(min(32, max(torch.get_num_threads(), 8)))
    stream_tol, h_tol, xrec_tol, grad_tol, match_min = FP16_BOUNDS[case]
    P = O.make_params(cfg, seed)
    x = O.make_images(seed + 1, B, cfg["image_size"], smooth=not spread)
    if spread:
        _spread_codebook(P, x, cfg, seed)
    m = _build16(cfg, P)
    eng = m.engine
    assert eng.loss_scale == 65536.0 and eng.codes_precision == "fp16"
    out = eng.forward_backward(x, w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
    torch.cuda.synchronize()
    M = B * eng.n_tok
    io = eng._io_bufs(B)
    codes = (out["indices"].view(B, eng.n_tok, -1) if eng.q.use_residual else out["indices"].view(B, eng.n_tok)).cpu()
    with torch.no_grad():
        o_q, o_ql, o_idx, o_h = O.encode(x, P, cfg)
        o_xrec_free = O.decode(o_q, P, cfg)
    match_e2e = (codes == o_idx).float().mean().item()
    e_x_free = rel(io["xrec"], o_xrec_free)
    _, _, idx_ob = O.quantizer_forward(io["h"].cpu().view(B, eng.n_tok, -1), P["quantizer.embedding.weight"], **O.qparams(cfg))
    match_ob = (codes == idx_ob).float().mean().item()
    ref = O.train_step_traced(x, P, cfg, force_idx=codes)
    rows = []
    for name, tower, tr in (("enc", eng.enc, ref["enc_trace"]), ("dec", eng.dec, ref["dec_trace"])):
        xs = tower.bufs(B, True)["x"]
        for i, t in enumerate(tr):
            rows.append((f"{name}.x[{i}]", rel(xs[i], t.reshape(M, -1))))
    e_h, e_x = rel(io["h"], ref["h"].reshape(M, -1)), rel(io["xrec"], ref["xrec"])
    S = eng.loss_scale
    errs = {k: rel(p.grad / S, ref["grads"][k]) for k, p in m.named_parameters() if k in ref["grads"]}      # the flat gradients carry the loss scale until the AdamW launch
    worst = max(errs, key=errs.get)
    finite = all(bool(torch.isfinite(p.grad).all()) for _, p in m.named_parameters() if p.grad is not None)
    lines = [f"== {label}: B={B}, fp16 MFMA operands (loss scale 2^16) vs fp32 CPU oracle =="]
    lines += [f"  {n:12s} rel {e:.2e}" for n, e in rows]
    lines += [f"  h            rel {e_h:.2e}", f"  xrec         rel {e_x:.2e}  (same codes)   {e_x_free:.2e} (oracle run freely, incl. index flips)",
              f"  loss {out['loss'].item():.6f} vs {ref['loss'].item():.6f}   qloss {out['quant_loss'].item():.6f} vs {ref['qloss'].item():.6f}",
              f"  code match-rate end-to-end {match_e2e:.4f}   at the op boundary (identical h) {match_ob:.6f}   distinct codes used {o_idx.unique().numel()}",
              f"  gradients (same codes, unscaled): median rel {np.median(list(errs.values())):.2e}, worst {worst} {errs[worst]:.2e}   all finite: {finite}",
              "  worst five: " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:5])]
    print("\n" + "\n".join(lines))
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "parity_fp16.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
    assert finite and set(errs) == set(ref["grads"])
    assert match_ob == 1.0, "indices must be bit-exact for identical quantizer input"
    assert o_idx.unique().numel() >= min_distinct
    assert max(e for _, e in rows) <= stream_tol, rows
    assert e_h <= h_tol and e_x <= xrec_tol, (e_h, e_x)
    assert abs(out["loss"].item() - ref["loss"].item()) <= 2e-3 * abs(ref["loss"].item())
    assert match_e2e >= match_min, match_e2e
    if spread:
        cb = errs.pop("quantizer.embedding.weight")      # a difference of nearly equal unit vectors (see test_parity_base_gpu.py): cancellation amplifies h's error ~12x
        assert cb <= 0.02, cb
        worst = max(errs, key=errs.get)
    assert errs[worst] <= grad_tol, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


def test_base_config2_fp16_meets_the_tolerance():
    _run_fp16_case("imagenet_vitvq_base (config 2)", "base", BASE, 2, 0)


def test_base_rq4_config4_fp16_meets_the_tolerance():
    cfg = copy.deepcopy(BASE)
    cfg["quantizer"].update(use_residual=True, num_quantizers=4)
    _run_fp16_case("imagenet_rqvae_base (config 4)", "rq4", cfg, 2, 3)


def test_base_config2_fp16_spread_codebook():
    _run_fp16_case("imagenet_vitvq_base (config 2), spread codebook", "base_spread", BASE, 2, 10, spread=True, min_distinct=1000)


def test_base_rq4_fp16_spread_codebook():
    cfg = copy.deepcopy(BASE)
    cfg["quantizer"].update(use_residual=True, num_quantizers=4)
    _run_fp16_case("imagenet_rqvae_base (config 4), spread codebook", "rq4_spread", cfg, 2, 13, spread=True, min_distinct=1000)


def test_large_config5_towers_fp16():
    _run_fp16_case("imagenet_vitvq_large towers (config 5)", "large", LARGE, 1, 5)


def test_fp16_training_steps_follow_the_oracle_and_skip_on_overflow():
    """five AdamW steps through the loss-scaled fp16 backward track the fp32 oracle's trajectory (tiny config: every kernel family incl. the small-shape
    GEMMs); then a step whose gradient is poisoned with an inf is dropped — parameters, moments and the fp16 operand shadow keep their bits — and counted;
    the update after it is the oracle's AdamW step 6 (the applied count), not 7."""
    import vitvq_oracle as O
    cfg = O.TINY_CFG
    P = O.make_params(cfg, 21)
    m = _build16(cfg, P)
    eng = m.engine
    xs = [O.make_images(30 + i, 2, cfg["image_size"]) for i in range(5)]
    Po = {k: v.clone() for k, v in P.items()}
    mo = {k: torch.zeros_like(v) for k, v in Po.items()}; vo = {k: torch.zeros_like(v) for k, v in Po.items()}
    lr = 1e-3
    for step, x in enumerate(xs, 1):
        out = eng.forward_backward(x, w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
        eng.optimizer_step(lr)
        o_loss, _, o_grads, _ = O.train_step_grads(x, Po, cfg)
        for k, gk in o_grads.items():
            O.adamw_step(Po[k], gk, mo[k], vo[k], step, lr)
        assert abs(out["loss"].item() - o_loss.item()) <= 2e-2 * abs(o_loss.item()), (step, out["loss"].item(), o_loss.item())
    torch.cuda.synchronize()
    assert eng.skipped_steps.item() == 0.0
    sd = {k: p.detach().cpu() for k, p in m.named_parameters()}
    worst = max(rel(sd[k], Po[k]) for k in o_grads)
    print(f"fp16 five-step trajectory: worst parameter rel error vs the fp32 oracle {worst:.2e}")
    assert worst <= 5e-3
    eng.forward_backward(xs[0], w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
    eng.store.g[12345 % eng.store.numel] = float("inf")
    before = (eng.store.p.clone(), eng.store.m.clone(), eng.store.v.clone(), eng.store.p16.clone())
    eng.optimizer_step(lr)
    torch.cuda.synchronize()
    assert eng.skipped_steps.item() == 1.0
    for t, b in zip((eng.store.p, eng.store.m, eng.store.v, eng.store.p16), before):
        assert torch.equal(t, b)
    assert eng.loss_scale == 32768.0, "GradScaler.update: an overflow halves the scale (on the device)"
    # the next step runs under the new scale and lands on the oracle's next step
    out = eng.forward_backward(xs[0], w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
    eng.unscale_grads()
    o_loss, _, o_grads, _ = O.train_step_grads(xs[0], {k: v.detach().cpu() for k, v in m.state_dict().items() if k in Po}, cfg)
    worst_g = max(rel(p.grad, o_grads[k]) for k, p in m.named_parameters() if k in o_grads)
    assert worst_g <= 5e-3, worst_g
    # and its update is AdamW's SIXTH step: the dropped one does not count (GradScaler.step does not call optimizer.step() on an overflow)
    eng.optimizer_step(lr)
    for k, gk in o_grads.items():
        O.adamw_step(Po[k], gk, mo[k], vo[k], 6, lr)
    sd = {k: p.detach().cpu() for k, p in m.named_parameters()}
    worst = max(rel(sd[k], Po[k]) for k in o_grads)
    print(f"fp16 update after the dropped step: worst parameter rel error vs the fp32 oracle at step 6 {worst:.2e}")
    assert worst <= 5e-3 and eng.store.step_count == 6 and eng.skipped_steps.item() == 1.0


def test_encode_codes_defaults_to_the_single_fp16_pass_and_x3_stays_available():
    import vitvq_oracle as O
    P = O.make_params(BASE, 0)
    x = O.make_images(1, 2, 256)
    m = _build16(BASE, P)
    with torch.no_grad():
        _, _, o_idx, _ = O.encode(x, P, BASE)
    c16 = m.encode_codes(x).cpu()
    c3 = m.encode_codes(x, precision="x3").cpu()
    m16, m3 = (c16 == o_idx).float().mean().item(), (c3 == o_idx).float().mean().item()
    print(f"encode_codes vs the fp32 oracle: fp16 single pass {m16:.4f}, x3 instrument {m3:.4f}")
    assert m16 >= 0.995 and m3 >= 0.9995
    xr = m(x)[0] if False else m.engine.reconstruct(x)[0]
    assert bool(torch.isfinite(xr).all())
