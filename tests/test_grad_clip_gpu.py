"""Gradient-norm clipping on the device (enh_grad_clip_coef + the clip operands of enh_adamw_step) from the kernel to the two optimizers.

Bounds.  The norm kernel adds the four squares of one 16-byte load in f32 and everything above that in f64, so the sum carries at most 4 f32 roundings of
positive summands (4 * 2^-24 = 2.4e-7 relative, half that on the root) at any size; the results are stored as f32 (6e-8).  The tests hold it to 1e-5
against numpy fp64.  The AdamW checks compare against the CPU oracle's AdamW on the SAME gradient, pre-multiplied on the host, at the tolerances of the
existing optimizer checks (tests/test_ops_gpu.py::test_colsum_cast_adamw over three steps; tests/test_fp16_gpu.py's one-step check: 1e-6).  Of that 1e-6
the second moment of a FIRST step spends 9.5e-7 before any clipping: the kernel forms 1 - beta2 in f32 (0.0099999905) where the oracle rounds 0.01; the
coefficient adds its own f32 rounding twice (<= 2.4e-7 worst case).  Measured with clipping on: v 9.4e-7 on step 1, 1.1e-7 on step 2."""
import warnings

import numpy as np
import pytest
import torch

from util import rel

pytestmark = pytest.mark.gpu

F32 = torch.float32
INF = float("inf")
GRAD_SCALE, LOSS_SCALE = 0.25, 65536.0
SIZES = [1, 3, 5, 1027, 100003, 4194309]      # 4194309 = 2 * 2048 * 256 * 4 + 5: two trips of the capped grid's stride loop and a ragged tail


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from enhancing import _C
    _C.lib()
    return _C


def _grad(n, seed=0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + n)) * 0.01


def _ref_norm(g, grad_scale=1.0, loss_scale=1.0):
    return float(np.sqrt(np.sum(np.square(g.detach().cpu().numpy().astype(np.float64)))) * grad_scale / loss_scale)


def _ref_coef(total, max_norm):
    return min(1.0, max_norm / (total + 1e-6))


def _clip(C, gd, max_norm, grad_scale=1.0, loss_scale=None, found_inf=None):
    out = torch.full((2,), -7.0, device="cuda")
    ls = None if loss_scale is None else torch.full((1,), loss_scale, device="cuda")
    C.grad_clip_coef(gd, max_norm, grad_scale, out, loss_scale=ls, found_inf=found_inf)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_norm_and_coefficient_against_fp64(C, n):
    g = _grad(n)
    gd = g.cuda()
    total = _ref_norm(g, GRAD_SCALE, LOSS_SCALE)
    max_norm = 0.5 * total
    out = _clip(C, gd, max_norm, GRAD_SCALE, LOSS_SCALE).cpu().double()
    coef = _ref_coef(total, float(np.float32(max_norm)))
    print(f"n={n}: total_norm {out[0].item():.9e} vs {total:.9e} (rel {abs(out[0].item() - total) / total:.2e}), coef {out[1].item():.9e} vs {coef:.9e}")
    assert abs(out[0].item() - total) <= 1e-5 * total
    assert coef < 1.0 and abs(out[1].item() - coef) <= 1e-5 * coef
    # a threshold above the norm, or none at all (monitor only), clips nothing: the coefficient is 1 exactly
    for loose in (2.0 * total + 1e-5, INF):
        out = _clip(C, gd, loose, GRAD_SCALE, LOSS_SCALE).cpu()
        assert out[1].item() == 1.0 and abs(out[0].item() - total) <= 1e-5 * total
    # without the device loss scale the division is by 1
    t1 = _ref_norm(g, GRAD_SCALE)
    assert abs(_clip(C, gd, INF, GRAD_SCALE)[0].item() - t1) <= 1e-5 * t1


@pytest.mark.parametrize("n", [5, 100003, 4194309])
def test_norm_is_bit_reproducible(C, n):
    gd = _grad(n, 1).cuda()
    flag = torch.zeros(1, device="cuda")
    a = _clip(C, gd, 1e-4, GRAD_SCALE, LOSS_SCALE, flag)
    b = _clip(C, gd, 1e-4, GRAD_SCALE, LOSS_SCALE, flag)
    assert torch.equal(a, b) and a[0].item() > 0.0


def test_nonfinite_flag_rides_along(C):
    n = 100003
    g = _grad(n, 2)
    flag = torch.zeros(1, device="cuda")
    _clip(C, g.cuda(), 1.0, found_inf=flag)
    assert flag.item() == 0.0, "a clean buffer leaves a zeroed flag alone"
    flag.fill_(1.0)
    _clip(C, g.cuda(), 1.0, found_inf=flag)
    assert flag.item() == 1.0, "the flag is never cleared"
    for bad, pos in ((INF, n - 1), (float("nan"), n // 2), (-INF, 0), (float("nan"), n - 2)):      # n - 1, n - 2: tail elements (n % 4 == 3)
        gb = g.clone(); gb[pos] = bad
        flag.zero_()
        _clip(C, gb.cuda(), 1.0, found_inf=flag)
        assert flag.item() == 1.0, (bad, pos)
    # without a flag operand the same buffers are simply measured
    gb = g.clone(); gb[n - 1] = INF
    assert _clip(C, gb.cuda(), 1.0)[0].item() == INF


def test_adamw_with_coefficient_and_value_clamp(C):
    import vitvq_oracle as O
    n = 100003
    gen = torch.Generator().manual_seed(4)
    p0, gr = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.01
    gd = gr.cuda()
    # (1) by norm: the coefficient comes from the norm kernel, the oracle steps on g * coef
    total = _ref_norm(gr)
    max_norm = 0.5 * total
    coef = _ref_coef(total, float(np.float32(max_norm)))
    out = _clip(C, gd, max_norm)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    pd, md, vd = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p16 = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    gc = (gr.double() * coef).float()
    for step in (1, 2, 3):
        O.adamw_step(p, gc, m, v, step, 4.5e-6)
        C.adamw_step(pd, gd, md, vd, p16, step, 4.5e-6, clip_coef=out[1:])
    assert rel(pd, p) <= 1e-6 and rel(md, m) <= 1e-5 and rel(vd, v) <= 1e-5
    assert torch.equal(p16.cpu(), pd.cpu().to(torch.bfloat16))
    assert rel(md, m * (1.0 / coef)) > 0.1, "the coefficient was applied"
    # (2) by value
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    pd, md, vd = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    gc = gr.clamp(-0.005, 0.005)
    assert 0.2 < (gc != gr).float().mean().item() < 0.9
    for step in (1, 2, 3):
        O.adamw_step(p, gc, m, v, step, 4.5e-6)
        C.adamw_step(pd, gd, md, vd, None, step, 4.5e-6, clip_value=0.005)
    assert rel(pd, p) <= 1e-6 and rel(md, m) <= 1e-5 and rel(vd, v) <= 1e-5
    assert md.abs().max().item() <= 0.005
    # (3) both operands off: the very same bits as a call that does not name them
    a = [p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.empty(n, dtype=torch.float16, device="cuda")]
    b = [t.clone() for t in a]
    ls = torch.full((1,), 4096.0, device="cuda")
    for step in (1, 2):
        C.adamw_step(a[0], gd, a[1], a[2], a[3], step, 1e-3, grad_scale=0.5, loss_scale=ls)
        C.adamw_step(b[0], gd, b[1], b[2], b[3], step, 1e-3, grad_scale=0.5, loss_scale=ls, clip_coef=None, clip_value=0.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _build(cfg, P, precision):
    from enhancing.modules.stage1.vitvqgan import ViTVQ
    from enhancing.utils.general import AttrDict
    loss = {"target": "enhancing.losses.vqperceptual.VQLPIPS",
            "params": dict(codebook_weight=1.0, loglaplace_weight=0.0, loggaussian_weight=1.0, perceptual_weight=0.0)}
    m = ViTVQ("image", cfg["image_size"], cfg["patch_size"], AttrDict.wrap(cfg["encoder"]), AttrDict.wrap(cfg["decoder"]),
              AttrDict.wrap(cfg["quantizer"]), AttrDict.wrap(loss))
    m.precision = precision
    m.load_state_dict(P, strict=True)
    assert m.engine.precision == precision
    return m


def _oracle_step(store, g64, factor, lr):
    """the CPU oracle's AdamW over the whole flat buffers on g64 * factor, from the store's current state and for its NEXT step -> (p, m, v)"""
    import vitvq_oracle as O
    p, m, v = store.p.cpu().clone(), store.m.cpu().clone(), store.v.cpu().clone()
    O.adamw_step(p, (g64 * factor).float(), m, v, store.step_count + 1, lr)
    return p, m, v


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_engine_step_clips_the_final_gradient(precision):
    """one optimizer step of the tiny model with clipping certainly active (threshold = half the norm), then a second one with grad_scale = 0.5 (an
    accumulation window of two) on non-zero moments: p, m, v follow the oracle's AdamW on g * grad_scale / loss_scale * coef, and grad_norm is the norm
    of that final gradient.  fp16: the loss-scaled engine (scale 2^16, flag pass fused into the norm pass); bf16: no scaler, no flag."""
    import vitvq_oracle as O
    cfg = O.TINY_CFG
    m = _build(cfg, O.make_params(cfg, 21), precision)
    eng, lr = m.engine, 1e-3
    s = eng.store
    S = 65536.0 if precision == "fp16" else 1.0
    assert eng.loss_scale == S and (eng.found_inf is not None) == (precision == "fp16")
    for i, grad_scale in enumerate((1.0, 0.5)):
        eng.forward_backward(O.make_images(30 + i, 2, cfg["image_size"]), w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
        g64 = s.g.cpu().double()
        total = _ref_norm(g64, grad_scale, S)
        clip_norm = 0.5 * total
        coef = _ref_coef(total, clip_norm)
        p, mm, v = _oracle_step(s, g64, grad_scale / S * coef, lr)
        eng.optimizer_step(lr, grad_scale=grad_scale, clip_norm=clip_norm)
        got = eng.grad_norm.item()
        print(f"{precision} grad_scale {grad_scale}: grad_norm {got:.6e} vs {total:.6e}, coef {coef:.4f}; p {rel(s.p, p):.1e} m {rel(s.m, mm):.1e} v {rel(s.v, v):.1e}")
        assert abs(got - total) <= 1e-5 * total and 0.49 < coef < 0.5
        assert rel(s.p, p) <= 1e-6 and rel(s.m, mm) <= 1e-6 and rel(s.v, v) <= 1e-6
        assert torch.equal(s.p16.cpu(), s.p.cpu().to(s.p16.dtype))
    if precision == "fp16":
        assert eng.skipped_steps.item() == 0.0 and eng.loss_scale == S
    # monitor only: the norm is measured and the step is the unclipped step, bit for bit
    eng.forward_backward(O.make_images(40, 2, cfg["image_size"]), w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
    total = _ref_norm(s.g, 1.0, S)
    before = [t.clone() for t in (s.p, s.m, s.v)]
    count = s.step_count
    eng.optimizer_step(lr, clip_norm=INF)
    tracked = [t.clone() for t in (s.p, s.m, s.v)]
    assert abs(eng.grad_norm.item() - total) <= 1e-5 * total
    for t, b in zip((s.p, s.m, s.v), before):
        t.copy_(b)
    s.step_count = count
    eng.optimizer_step(lr)
    assert all(torch.equal(a, b) for a, b in zip(tracked, (s.p, s.m, s.v)))


def test_overflow_under_clipping_drops_the_step():
    import vitvq_oracle as O
    cfg = O.TINY_CFG
    m = _build(cfg, O.make_params(cfg, 21), "fp16")
    eng = m.engine
    eng.forward_backward(O.make_images(30, 2, cfg["image_size"]), w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
    eng.optimizer_step(1e-3, clip_norm=1e-3)          # a clean step first: non-zero moments
    assert eng.skipped_steps.item() == 0.0
    eng.forward_backward(O.make_images(31, 2, cfg["image_size"]), w_l1=0.0, w_l2=1.0, codebook_weight=1.0)
    eng.store.g[12345 % eng.store.numel] = INF
    before = (eng.store.p.clone(), eng.store.m.clone(), eng.store.v.clone(), eng.store.p16.clone())
    eng.optimizer_step(1e-3, clip_norm=1e-3)
    torch.cuda.synchronize()
    assert eng.skipped_steps.item() == 1.0
    for t, b in zip((eng.store.p, eng.store.m, eng.store.v, eng.store.p16), before):
        assert torch.equal(t, b)
    assert eng.loss_scale == 32768.0, "GradScaler.update: an overflow halves the scale (on the device)"


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = torch.nn.Linear(37, 129), torch.nn.Linear(129, 3)


@pytest.mark.parametrize("scaled", [True, False])
def test_flat_adamw_clips_by_norm(scaled):
    from enhancing.engine.optim import FlatAdamW, LossScaler
    from enhancing.engine.stage1 import ParamStore
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    store = ParamStore(_Net(), dev, precision="fp32")
    sc = store.loss_scaler = LossScaler(dev, init_scale=4096.0)
    sc.enabled = scaled
    S = 4096.0 if scaled else 1.0
    opt = FlatAdamW(store, lr=1e-3)
    opt.grad_scale = 0.5
    gen = torch.Generator().manual_seed(7)
    for step in (1, 2):
        g = torch.randn(store.numel, generator=gen) * 0.01
        store.g.copy_(g * S)
        g64 = store.g.cpu().double()
        total = _ref_norm(g64, 0.5, S)
        opt.gradient_clip_val = 0.5 * total
        coef = _ref_coef(total, opt.gradient_clip_val)
        p, m, v = _oracle_step(store, g64, 0.5 / S * coef, 1e-3)
        opt.step()
        assert abs(opt.grad_norm.item() - total) <= 1e-5 * total
        assert rel(store.p, p) <= 1e-6 and rel(store.m, m) <= 1e-6 and rel(store.v, v) <= 1e-6
    assert store.step_count == 2 and float(sc.found_inf) == 0.0 and int(sc.tracker) == (2 if scaled else 0) and sc.scale_t.item() == 4096.0
    # by value, through the same optimizer
    opt.gradient_clip_algorithm, opt.gradient_clip_val = "value", 0.002
    g64 = store.g.cpu().double()
    p, m, v = _oracle_step(store, (g64 * (0.5 / S)).clamp(-0.002, 0.002), 1.0, 1e-3)
    opt.step()
    assert rel(store.p, p) <= 1e-6 and rel(store.m, m) <= 1e-6 and rel(store.v, v) <= 1e-6
    if scaled:      # an overflow with clipping on: dropped, the scale halves
        store.g[5] = INF
        opt.gradient_clip_algorithm, opt.gradient_clip_val = "norm", 1e-3
        before = (store.p.clone(), store.m.clone(), store.v.clone())
        opt.step()
        assert float(sc.found_inf) == 1.0 and sc.scale_t.item() == 2048.0 and all(torch.equal(a, b) for a, b in zip(before, (store.p, store.m, store.v)))


def test_graph_replay_with_clipping_equals_the_eager_sequence(lpips_random_init):
    """the two-optimizer protocol of tests/test_disc_model_gpu.py's replay test (tiny config, 2 images, four rounds: R1 on rounds 0 and 2, so each of the three
    graphs is replayed) with both optimizers clipping by norm at a threshold below their gradient norms: losses, both flat parameter buffers and both
    gradient norms are the eager sequence's, bit for bit — the norm, the coefficient and the clipped step never visit the host."""
    import vitvq_oracle as O
    from enhancing.modules.stage1.vitvqgan import ViTVQ
    from enhancing.utils.general import AttrDict
    cfg = O.TINY_CFG
    loss = {"target": "enhancing.losses.vqperceptual.VQLPIPSWithDiscriminator",
            "params": dict(loglaplace_weight=0.0, loggaussian_weight=1.0, perceptual_weight=0.1, adversarial_weight=0.1, do_r1_every=2,
                           disc_params={"size": cfg["image_size"]})}
    xs = [O.make_images(5 + i, 2, cfg["image_size"]) for i in range(2)]
    CLIP = 1e-3

    def run(graphs: bool):
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = ViTVQ("image", cfg["image_size"], cfg["patch_size"], AttrDict.wrap(cfg["encoder"]), AttrDict.wrap(cfg["decoder"]),
                      AttrDict.wrap(cfg["quantizer"]), AttrDict.wrap(loss))
        m.load_state_dict({**O.make_params(cfg, seed=11), **{"loss." + k: v for k, v in m.loss.state_dict().items()}}, strict=False)
        m.train()
        m.learning_rate = 1e-3
        opts, _ = m.configure_optimizers()
        for o in opts:
            o.gradient_clip_val = CLIP
        m.engine.use_graphs = graphs
        losses, norms = [], []
        for i in range(4):
            b = {"image": xs[i % 2]}
            l0 = m.training_step(b, i, 0); opts[0].step()
            l1 = m.training_step(b, i, 1); opts[1].step()
            m.global_step += 1
            losses.append((l0.clone(), l1.clone()))
            norms.append((opts[0].grad_norm.clone(), opts[1].grad_norm.clone()))
        torch.cuda.synchronize()
        if graphs:
            assert len(m._step_graphs) == 3          # optimizer 0; optimizer 1 with and without R1
        return losses, norms, m.engine.store.p.clone(), m.loss.disc_store(m.engine.device).p.clone()

    le, ne, pe, de = run(False)
    lg, ng, pg, dg = run(True)
    for i, (a, b) in enumerate(zip(le + ne, lg + ng)):
        assert all(torch.equal(u, v) for u, v in zip(a, b)), (i, [float(u) for u in a], [float(v) for v in b])
    assert torch.equal(pe, pg) and torch.equal(de, dg)
    assert all(float(a) > CLIP and float(d) > CLIP for a, d in ne), [(float(a), float(d)) for a, d in ne]
