"""Quantizer code widths other than 32 (embed_dim % 8 == 0, 8 <= embed_dim <= 256) on the fused HIP kernels.

d <= 32 runs the width-32 kernels on zero-padded rows: bit-exact against the C oracle on the padded inputs.  Wider codes run the
DW = 64 / 128 / 256 family: indices against the reference formula (every mismatch an fp32 near-tie by the fp64 gap, bench.py's bound),
straight-through values and loss to fp32 rounding, and bit-for-bit padding consistency across the family.  Model-level tests mirror
tests/test_model_gpu.py at widths 8, 64 and 256."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import rel

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 1e-5, 2.5e-3          # as tests/test_ops_gpu.py
ACT_TOL, GRAD_TOL = 1e-2, 3e-2            # as tests/test_model_gpu.py
EXACT_TOL = 1e-5


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _pad(x, w):
    return F.pad(x, (0, w - x.shape[1]))


# ---------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 16, 24])
@pytest.mark.parametrize("K", [500, 8192])
@pytest.mark.parametrize("depth", [1, 4])
def test_narrow_codes_are_the_width32_kernel_on_zero_padded_rows(C, d, K, depth):
    import vitvq_oracle as O
    import vq_oracle as VC
    M = 1000
    z, E, _ = O.make_vq_inputs(300 + d + depth, M, K, d)
    zq_c, idx_c, loss_c = VC.forward(_pad(z, 32).numpy(), _pad(E, 32).numpy(), 0.25, depth)
    zq, zq16, idx, loss = C.vq_forward(z.cuda(), E.cuda(), 0.25, depth, True)
    assert zq.shape == (M, d) and zq16.shape == (M, d)
    assert torch.equal(idx.cpu(), torch.from_numpy(idx_c)), "code indices must be bit-exact"
    assert np.array_equal(zq.cpu().numpy().view(np.uint32), np.ascontiguousarray(zq_c[:, :d]).view(np.uint32)), "z_q must be bit-exact"
    ref = float(loss_c) * 32.0 / d          # the oracle averages over the padded 32 columns, the kernel over the true d
    assert abs(loss.item() - ref) <= 1e-6 * abs(ref)
    assert torch.equal(zq16.cpu(), zq.cpu().to(torch.bfloat16))


def _audit_wide(z, E, idx, depth, beta=0.25):
    """The reference's quantizer (vitvq_oracle.vq_distances, fp32) evaluated depth by depth on the residual left by the kernel's own
    earlier codes, so that a near-tie flip at one depth is not counted again at the next.  Returns (match rate, loss, z_q, agree mask)."""
    import vitvq_oracle as O
    M, d = z.shape
    en = O.l2norm(E)
    en64 = F.normalize(E.double(), dim=-1)
    bound = (6 * d + 12) * 2.0 ** -24       # bench.py VQ_NEAR_TIE_BOUND with n = d
    r = z.clone()
    agree = torch.ones(M, dtype=torch.bool, device=z.device)
    mism, losses = 0, []
    for i in range(depth):
        zn = O.l2norm(r)
        ki = idx[:, i]
        for s in range(0, M, 8192):
            it = torch.argmin(O.vq_distances(zn[s:s + 8192], en), dim=1)
            bad = (it != ki[s:s + 8192]).nonzero().view(-1)
            if len(bad):
                zb = F.normalize(r[s + bad].double(), dim=-1)
                dist = (zb ** 2).sum(1, keepdim=True) + (en64 ** 2).sum(1) - 2 * zb @ en64.t()
                rows = torch.arange(len(bad), device=z.device)
                gap = (dist[rows, it[bad]] - dist[rows, ki[s + bad]]).abs()
                assert bool((gap < bound).all()), f"depth {i}: non-near-tie mismatch, gaps {gap.max().item():.3e} >= {bound:.3e}"
                agree[s + bad] = False
                mism += len(bad)
        e = en[ki]
        m = torch.mean((e.double() - zn.double()) ** 2)
        losses.append(beta * m + m)
        r = r - e
    zq_sum = sum(en[idx[:, i]] for i in range(depth))
    zq = z + (zq_sum - z)
    return 1.0 - mism / (M * depth), torch.stack(losses).mean().item(), zq, agree


@pytest.mark.parametrize("d", [48, 64, 128, 256])
@pytest.mark.parametrize("depth", [1, 4])
def test_wide_codes_against_the_reference_formula(C, d, depth):
    import vitvq_oracle as O
    M, K = 65536, 8192
    z, E, _ = O.make_vq_inputs(500 + d + depth, M, K, d)
    z, E = z.cuda(), E.cuda()
    zq, zq16, idx, loss = C.vq_forward(z, E, 0.25, depth, True)
    assert zq.shape == (M, d) and idx.shape == (M, depth)
    rate, ref_loss, zq_ref, agree = _audit_wide(z, E, idx, depth)
    print(f"d={d} depth={depth}: index match rate {rate:.6f}, loss {loss.item():.7f} vs {ref_loss:.7f}")
    assert rate >= 0.999
    assert (zq[agree] - zq_ref[agree]).abs().max().item() <= 1e-6
    assert abs(loss.item() - ref_loss) <= 1e-5 * abs(ref_loss)
    assert torch.equal(zq16, zq.to(torch.bfloat16))


def test_padding_is_bit_exact_across_the_family(C):
    import vitvq_oracle as O
    z, E, _ = O.make_vq_inputs(48, 4096, 8192, 48)
    for depth in (1, 4):
        zq48, _, idx48, _ = C.vq_forward(z.cuda(), E.cuda(), 0.25, depth, True)
        zq64, _, idx64, _ = C.vq_forward(_pad(z, 64).cuda(), _pad(E, 64).cuda(), 0.25, depth, True)
        assert torch.equal(idx48, idx64)
        assert torch.equal(zq48.view(torch.int32), zq64[:, :48].contiguous().view(torch.int32))


@pytest.mark.parametrize("d,depth,resid", [(8, 1, False), (8, 4, True), (64, 1, False), (64, 4, True), (64, 8, True),
                                           (256, 1, False), (256, 4, True)])
def test_backward_vs_autograd(C, d, depth, resid):
    import vitvq_oracle as O
    M, K = 1024, 1024
    z, E, g = O.make_vq_inputs(70 + d + depth, M, K, d)
    zt = z.clone().requires_grad_(True)
    Et = E.clone().requires_grad_(True)
    zq, loss, idx = O.quantizer_forward(zt, Et, 0.25, True, resid, depth if resid else None)
    gl = 0.7
    ((zq * g).sum() + gl * loss).backward()
    dE = torch.zeros(K, d, device="cuda")
    idx_d = idx.view(M, -1).cuda()
    dz, dz16 = C.vq_backward(z.cuda(), E.cuda(), idx_d, g.cuda(), gl, None, 0.25, depth, resid, True, dE)
    assert dz.shape == (M, d)
    assert rel(dz, zt.grad) <= F32_TOL
    assert rel(dE, Et.grad) <= F32_TOL
    assert rel(dz16.float(), zt.grad) <= BF16_TOL
    dE2 = torch.zeros(K, d, device="cuda")
    C.vq_backward(z.cuda(), E.cuda(), idx_d, g.cuda(), gl, None, 0.25, depth, resid, True, dE2)
    assert torch.equal(dE.view(torch.int32), dE2.view(torch.int32)), "codebook gradient must be bit-reproducible"


@pytest.mark.parametrize("d", [8, 64, 256])
def test_codebook_gradient_is_bit_reproducible_under_usage_collapse(C, d):
    import vitvq_oracle as O
    M, K, depth = 32768, 1024, 4
    z, E, g = O.make_vq_inputs(90 + d, M, K, d)
    idx = torch.randint(0, 4, (M, depth), generator=torch.Generator().manual_seed(d)).cuda()
    outs = []
    for _ in range(2):
        dE = torch.zeros(K, d, device="cuda")
        C.vq_backward(z.cuda(), E.cuda(), idx, g.cuda(), 0.7, None, 0.25, depth, True, True, dE)
        outs.append(dE)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert outs[0][4:].abs().max().item() == 0.0 and outs[0][:4].abs().max().item() > 0.0


@pytest.mark.parametrize("d", [8, 64, 256])
@pytest.mark.parametrize("depth", [1, 4])
def test_lookup(C, d, depth):
    import vitvq_oracle as O
    _, E, _ = O.make_vq_inputs(3 + d, 64, 1024, d)
    idx = torch.randint(0, 1024, (3001, depth), generator=torch.Generator().manual_seed(depth))
    ref = O.l2norm(F.embedding(idx, E)).sum(-2)
    out, out16 = C.vq_lookup(E.cuda(), idx.cuda(), True)
    assert out.shape == (3001, d)
    assert rel(out, ref) <= 1e-7
    assert torch.equal(out16, out.to(torch.bfloat16))
    _, out16h = C.vq_lookup(E.cuda(), idx.cuda(), True, h16=torch.float16)
    assert torch.equal(out16h, out.to(torch.float16))


@pytest.mark.parametrize("d", [8, 64, 256])
@pytest.mark.parametrize("depth", [1, 4])
def test_fp16_copies_are_the_rounded_f32_results(C, d, depth):
    """the loss-scaled fp16 engine asks the quantizer for fp16 copies (h16=float16): zq16 and dz16 must be the round-to-nearest-even images of zq and dz
    bit for bit, with the codebook-loss gradient as a host scalar and as the device scalar the engine passes; the bf16 copies are unchanged"""
    import vitvq_oracle as O
    M, K = 4096, 1024
    z, E, g = O.make_vq_inputs(40 + d + depth, M, K, d)
    z, E, g = z.cuda(), E.cuda(), g.cuda()
    zq, zq16, idx, loss = C.vq_forward(z, E, 0.25, depth, True, h16=torch.float16)
    assert zq16.dtype == torch.float16 and zq16.shape == (M, d)
    assert torch.equal(zq16.view(torch.int16), zq.to(torch.float16).view(torch.int16))
    zqb, zqb16, idxb, lossb = C.vq_forward(z, E, 0.25, depth, True)
    assert torch.equal(idx, idxb) and torch.equal(zq.view(torch.int32), zqb.view(torch.int32)) and torch.equal(loss, lossb)
    assert torch.equal(zqb16, zqb.to(torch.bfloat16))
    resid = depth > 1
    gs = g * 1024.0                   # the upstream gradient carries the loss scale in the engine
    for g_loss, g_dev in ((0.7 * 1024.0, None), (1.0, torch.tensor([0.7 * 1024.0], device="cuda"))):
        dE = torch.zeros(K, d, device="cuda")
        dz, dz16 = C.vq_backward(z, E, idx, gs, g_loss, g_dev, 0.25, depth, resid, True, dE, h16=torch.float16)
        assert dz16.dtype == torch.float16 and torch.isfinite(dz16).all()
        assert torch.equal(dz16.view(torch.int16), dz.to(torch.float16).view(torch.int16)), (g_loss, g_dev)
        dEb = torch.zeros(K, d, device="cuda")
        dzb, dzb16 = C.vq_backward(z, E, idx, gs, g_loss, g_dev, 0.25, depth, resid, True, dEb)
        assert torch.equal(dzb.view(torch.int32), dz.view(torch.int32)) and torch.equal(dzb16, dzb.to(torch.bfloat16))


def _fmaf_chain_sq(x):
    """ascending fmaf chain sum x_j * x_j from 0 in float32, column by column (x [N,16] float32): the product is exact in float64"""
    s = np.zeros(x.shape[0], dtype=np.float32)
    for j in range(x.shape[1]):
        xj = x[:, j].astype(np.float64)
        s = (xj * xj + s.astype(np.float64)).astype(np.float32)
    return s


def test_lookup_width32_keeps_its_arithmetic(C):
    """the width-32 lookup is the pre-generalisation kernel's arithmetic, bit for bit: S = chain(x[0..15]) + chain(x[16..31]),
    x / max(sqrt(S), 1e-12), rows added in depth order from 0 (restated in numpy float32)."""
    import vitvq_oracle as O
    _, E, _ = O.make_vq_inputs(33, 64, 1024, 32)
    idx = torch.randint(0, 1024, (777, 4), generator=torch.Generator().manual_seed(5))
    out, _ = C.vq_lookup(E.cuda(), idx.cuda(), True)
    En = E.numpy()
    acc = np.zeros((777, 32), dtype=np.float32)
    for i in range(4):
        x = En[idx[:, i].numpy()]
        S = _fmaf_chain_sq(x[:, :16]) + _fmaf_chain_sq(x[:, 16:])
        den = np.maximum(np.sqrt(S), np.float32(1e-12)).astype(np.float32)
        acc = (acc + x / den[:, None]).astype(np.float32)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), acc.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# model (mirrors tests/test_model_gpu.py)
# ---------------------------------------------------------------------------------------------
MODEL_CASES = [(8, 0), (64, 0), (256, 0), (64, 4)]


def _cfg(d, nq):
    import vitvq_oracle as O
    cfg = copy.deepcopy(O.TINY_CFG)
    cfg["quantizer"]["embed_dim"] = d
    if nq:
        cfg["quantizer"].update(use_residual=True, num_quantizers=nq)
    return cfg


def _build(cfg, P, exact=False):
    from enhancing.modules.stage1.vitvqgan import ViTVQ
    from enhancing.utils.general import AttrDict
    loss = {"target": "enhancing.losses.vqperceptual.VQLPIPS",
            "params": dict(codebook_weight=1.0, loglaplace_weight=0.0, loggaussian_weight=1.0, perceptual_weight=0.0)}
    m = ViTVQ("image", cfg["image_size"], cfg["patch_size"], AttrDict.wrap(cfg["encoder"]), AttrDict.wrap(cfg["decoder"]),
              AttrDict.wrap(cfg["quantizer"]), AttrDict.wrap(loss))
    m.load_state_dict(P, strict=True)
    if exact:
        m.precision = "fp32"
        assert m.engine.precision == "fp32"
    m.engine
    return m


@pytest.mark.parametrize("d,nq", MODEL_CASES)
def test_state_dict_shapes(d, nq):
    import vitvq_oracle as O
    cfg = _cfg(d, nq)
    m = _build(cfg, O.make_params(cfg, seed=11))
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("loss.")}
    assert sd == {k: tuple(s) for k, s in O.param_shapes(cfg).items()}
    dim = cfg["encoder"]["dim"]
    assert sd["pre_quant.weight"] == (d, dim) and sd["post_quant.weight"] == (cfg["decoder"]["dim"], d)
    assert sd["quantizer.embedding.weight"] == (cfg["quantizer"]["n_embed"], d)


@pytest.mark.parametrize("d,nq", MODEL_CASES)
def test_train_step_vs_oracle(d, nq):
    import vitvq_oracle as O
    cfg = _cfg(d, nq)
    P = O.make_params(cfg, seed=3)
    x = O.make_images(9, 2, cfg["image_size"])
    m = _build(cfg, P)
    loss = m.training_step({"image": x}, 0, 0)
    o_loss, _, o_grads, _ = O.train_step_grads(x, P, cfg)
    assert abs(loss.item() - o_loss.item()) <= 1e-2 * abs(o_loss.item())
    m.engine.unscale_grads()
    errs = {k: rel(p.grad, o_grads[k]) for k, p in m.named_parameters() if k in o_grads}
    worst = max(errs, key=errs.get)
    print(f"d={d} nq={nq} train-step grads vs oracle: worst {worst} {errs[worst]:.2e}")
    assert set(errs) == set(o_grads)
    assert errs[worst] <= GRAD_TOL, errs


@pytest.mark.parametrize("d,nq", MODEL_CASES)
def test_exact_mode_codes_and_loss(d, nq):
    import vitvq_oracle as O
    cfg = _cfg(d, nq)
    P = O.make_params(cfg, seed=4)
    x = O.make_images(8, 2, cfg["image_size"])
    m = _build(cfg, P, exact=True)
    assert torch.equal(m.encode_codes(x).cpu(), O.encode_codes(x, P, cfg)), "indices must match end to end in exact mode"
    loss = m.training_step({"image": x}, 0, 0)
    o_loss, _, _, _ = O.train_step_grads(x, P, cfg)
    assert abs(loss.item() - o_loss.item()) <= EXACT_TOL * abs(o_loss.item())


@pytest.mark.parametrize("d,nq", MODEL_CASES)
def test_decode_codes_roundtrip(d, nq):
    import vitvq_oracle as O
    cfg = _cfg(d, nq)
    P = O.make_params(cfg, seed=11)
    x = O.make_images(5, 2, cfg["image_size"])
    m = _build(cfg, P)
    codes = m.encode_codes(x)
    assert codes.shape == ((2, 64, nq) if nq else (2, 64))
    rec = m.decode_codes(codes)
    assert rel(rec, O.decode_codes(codes.cpu(), P, cfg)) <= ACT_TOL
    # the forward's reconstruction at the same codes: decode of the straight-through tokens the quantizer returns for them
    with torch.no_grad():
        h = m.pre_quant_tokens(x, m.engine.codes_precision)
        zq, _, idx = m.quantizer(h)
        assert torch.equal(idx.reshape(codes.shape).cpu(), codes.cpu())
        rec_fwd = m.decode(zq)
    assert rel(rec, rec_fwd) <= ACT_TOL
