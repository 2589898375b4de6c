"""GPTAdam(state="bf16") through the model: the `tiny` GPT of tests/gpt_backward_cases.py, the tiny CondTransformer of tests/test_gpt_train_gpu.py
(restated here) and the `rq_tiny` RQTransformer.  What the kernel computes is tests/test_adam16_kernel_gpu.py's subject; here: the buffers, the
switches, the first step against the f32-state optimizer, dropped steps, checkpoints in both formats and resumed training bit for bit."""
import pytest
import torch

import gpt_backward_cases as BC

pytestmark = pytest.mark.gpu

LR = 1e-3


def _model(seed=BC.PARAM_SEED):
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**BC.case_kwargs("tiny"))
    m.load_state_dict(BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed), strict=True)
    conds, codes = BC.case_inputs("tiny")
    return m.cuda(), conds.cuda(), codes.cuda()


def _bits(t):
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.int32: torch.int32}
    return t.detach().clone().contiguous().view(view[t.dtype])


def _opt_bits(opt):
    ts = [opt.p, opt.m, opt.v, opt.arena, opt.state]
    if opt.scaler is not None:
        ts += [opt.scaler.scale_t, opt.scaler.tracker]
    return [_bits(t) for t in ts]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _steps(m, opt, conds, codes, k):
    for _ in range(k):
        m.forward_backward(codes, conds, loss_scale=1.0 if opt.loss_scale is None else opt.loss_scale)
        opt.step()


def _cond_transformer():
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    torch.manual_seed(0)
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    cfg = AttrDict.wrap(dict(
        cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
        stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                    params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=tower, quantizer=dict(embed_dim=32, n_embed=64),
                                loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
        transformer=dict(target="enhancing.modules.stage2.layers.GPT",
                         params=dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, n_heads=2, n_layers=1))))
    return CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer, code_shape=[16])


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(3, 3, 32, 32, generator=g).cuda(), "class": torch.randint(0, 3, (3,), generator=g).cuda()}


def test_buffers_and_the_keyword(monkeypatch):
    from enhancing.engine.optim import GPTAdam
    monkeypatch.delenv("ENH_ADAM_STATE", raising=False)
    m, conds, codes = _model()
    opt = GPTAdam(m, lr=LR, state="bf16")
    n = m.flat_grad.numel()
    assert opt.state_format == "bf16" and opt.m.dtype == opt.v.dtype == torch.bfloat16 and opt.m.numel() == opt.v.numel() == n == opt.p.numel()
    assert opt.p.dtype == torch.float32 and not bool(opt.m.any()) and not bool(opt.v.any())
    for state in (None, "f32"):
        m2, _, _ = _model()
        o = GPTAdam(m2, lr=LR, state=state)
        assert o.state_format == "f32" and o.m.dtype == o.v.dtype == torch.float32
    with pytest.raises(ValueError, match="int8"):
        GPTAdam(m, lr=LR, state="int8")


def test_the_environment_switch_through_configure_optimizers(monkeypatch):
    for env, attr, want in ((None, None, torch.float32), ("bf16", None, torch.bfloat16), ("f32", None, torch.float32), (None, "bf16", torch.bfloat16),
                            ("bf16", "f32", torch.float32)):
        if env is None:
            monkeypatch.delenv("ENH_ADAM_STATE", raising=False)
        else:
            monkeypatch.setenv("ENH_ADAM_STATE", env)
        ct = _cond_transformer()
        ct.learning_rate = LR
        if attr is not None:
            ct.adam_state = attr
        ct.transformer.cuda()
        (opt,), _ = ct.configure_optimizers()
        assert opt.m.dtype == opt.v.dtype == want and opt.m.numel() == ct.transformer.flat_grad.numel(), (env, attr)
    monkeypatch.setenv("ENH_ADAM_STATE", "nonsense")
    del ct.adam_state                   # without the attribute the environment decides again
    with pytest.raises(ValueError, match="nonsense"):
        ct.configure_optimizers()


def test_the_first_step_has_the_bits_of_the_f32_state_optimizer():
    """from zero moments the update never reads stored state, and p never sees its own step's rounding; from the second step on it reads rounded moments"""
    from enhancing.engine.optim import GPTAdam
    (ma, conds, codes), (mb, _, _) = _model(), _model()
    oa, ob = GPTAdam(ma, lr=LR, init_scale=1024.0, state="f32"), GPTAdam(mb, lr=LR, init_scale=1024.0, state="bf16")
    _steps(ma, oa, conds, codes, 1)
    _steps(mb, ob, conds, codes, 1)
    assert torch.equal(_bits(oa.p), _bits(ob.p)) and torch.equal(_bits(oa.arena), _bits(ob.arena)) and torch.equal(_bits(oa.state), _bits(ob.state))
    # the stored moments are the f32 ones rounded to one of their two bf16 neighbours
    for a, b in ((oa.m, ob.m), (oa.v, ob.v)):
        lo = (_bits(a).to(torch.int64) & 0xFFFFFFFF) >> 16
        got = _bits(b).to(torch.int64) & 0xFFFF
        assert bool(((got == lo) | (got == lo + 1)).all()) and bool((got != lo).any())
    _steps(ma, oa, conds, codes, 1)
    _steps(mb, ob, conds, codes, 1)
    assert oa.state_dict()["step"] == ob.state_dict()["step"] == 2
    diff = (oa.p.double() - ob.p.double()).abs().max().item()
    print(f"max |p_f32state - p_bf16state| after step 2: {diff:.3e} (lr {LR})")
    assert diff <= 2 * LR, "an Adam update is bounded by ~lr: the two second steps cannot be further apart than two of them"


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_three_rounds_under_both_operand_formats(fmt, monkeypatch):
    from enhancing.modules.stage2.layers import GPT
    monkeypatch.setenv("ENH_PRECISION", fmt)
    monkeypatch.setenv("ENH_ADAM_STATE", "bf16")
    ct = _cond_transformer()
    ct.learning_rate = LR
    ct.transformer.cuda()
    (opt,), _ = ct.configure_optimizers()
    assert (opt.scaler is None) == (fmt == "bf16") and opt.arena.dtype == (torch.bfloat16 if fmt == "bf16" else torch.float16)
    if opt.scaler is not None:
        opt.scaler.scale_t.fill_(256.0)
    losses = []
    for s in range(3):
        losses.append(ct.training_step(_batch(s), s).item())
        opt.step()
    sd = opt.state_dict()
    assert sd["step"] == 3 and all(l == l and l > 0 for l in losses), "under bf16 no step is ever dropped; at scale 256 none overflows under fp16"
    assert bool(torch.isfinite(opt.m.float()).all()) and bool(torch.isfinite(opt.v.float()).all()) and bool((opt.v.float() >= 0).all())
    assert bool(opt.m.any()) and bool(opt.v.any())
    # forward, sample and forward_backward read the stepped weights without a rebuild: a fresh GPT loaded with them gives the same bits
    gpt = ct.transformer
    b = _batch(9)
    codes, conds = ct._tokenize(b)
    fresh = GPT(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, n_heads=2, n_layers=1)
    fresh.load_state_dict({k: v.cpu() for k, v in gpt.state_dict().items()})
    fresh = fresh.cuda()
    assert torch.equal(_bits(gpt(codes, conds)), _bits(fresh(codes, conds))), "the forward after three steps read a stale operand or bias copy"
    assert torch.equal(gpt.sample(conds, top_k=20, seed=3)[1], fresh.sample(conds, top_k=20, seed=3)[1])
    la, lb = gpt.forward_backward(codes, conds, loss_scale=256.0), fresh.forward_backward(codes, conds, loss_scale=256.0)
    assert torch.equal(_bits(la.view(1)), _bits(lb.view(1)))
    assert all(torch.equal(_bits(p.grad), _bits(q.grad)) for p, q in zip(gpt.parameters(), fresh.parameters()))


def test_a_forced_inf_drops_the_step_and_backs_the_scale_off():
    from enhancing.engine.optim import GPTAdam
    m, conds, codes = _model()
    opt = GPTAdam(m, lr=LR, init_scale=1024.0, state="bf16")
    _steps(m, opt, conds, codes, 1)
    before = _opt_bits(opt)[:5]
    m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
    m.flat_grad[5] = float("inf")
    opt.step()
    assert _same(before, _opt_bits(opt)[:5]), "the dropped step wrote something (p, m, v, the arena or the step count)"
    assert opt.loss_scale.item() == 512.0 and opt.scaler.tracker.item() == 0 and opt.state_dict()["step"] == 1
    _steps(m, opt, conds, codes, 1)
    assert opt.state_dict()["step"] == 2 and opt.loss_scale.item() == 512.0


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_resumed_training_has_the_bits_of_uninterrupted_training(fmt, monkeypatch):
    from enhancing.engine.optim import GPTAdam
    monkeypatch.setenv("ENH_PRECISION", fmt)
    N, seed = 2, 0x1234567890
    mb, conds, codes = _model()
    ob = GPTAdam(mb, lr=LR, init_scale=1024.0, state="bf16", state_seed=seed)
    _steps(mb, ob, conds, codes, 2 * N)                                   # run B: uninterrupted
    ma, _, _ = _model()
    oa = GPTAdam(ma, lr=LR, init_scale=1024.0, state="bf16", state_seed=seed)
    _steps(ma, oa, conds, codes, N)                                       # run A: N steps, a checkpoint ...
    sd, weights = oa.state_dict(), {k: v.clone() for k, v in ma.state_dict().items()}
    assert sd["state_format"] == "bf16" and sd["state_seed"] == seed and sd["step"] == N
    m2, _, _ = _model(seed=BC.PARAM_SEED + 1)
    o2 = GPTAdam(m2, lr=LR, state="bf16")                                 # ... a fresh optimizer (seed 0, default scale) over a model with the saved weights
    m2.load_state_dict(weights)
    o2.load_state_dict(sd)
    assert o2.state_seed == seed
    _steps(m2, o2, conds, codes, N)
    assert _same(_opt_bits(ob), _opt_bits(o2)), "resumed training differs from uninterrupted training (p, m, v, arena, step state or scaler)"
    assert o2.state_dict()["step"] == 2 * N
    m3, _, _ = _model()
    o3 = GPTAdam(m3, lr=LR, init_scale=1024.0, state="bf16", state_seed=seed + 1)
    _steps(m3, o3, conds, codes, 2 * N)
    assert not torch.equal(_bits(o3.m), _bits(ob.m)), "the seed does not reach the stored moments"


def test_checkpoints_load_across_formats():
    from enhancing.engine.optim import GPTAdam
    m16, conds, codes = _model()
    o16 = GPTAdam(m16, lr=LR, init_scale=1024.0, state="bf16", state_seed=5)
    _steps(m16, o16, conds, codes, 2)
    m32, _, _ = _model()
    o32 = GPTAdam(m32, lr=LR, init_scale=1024.0, state="f32")
    _steps(m32, o32, conds, codes, 2)
    sd16, sd32 = o16.state_dict(), o32.state_dict()
    assert sd16["m"].dtype == sd16["v"].dtype == torch.bfloat16 and sd32["m"].dtype == torch.float32 and not sd16["m"].is_cuda
    assert sd32["state_format"] == "f32" and sd16["state_format"] == "bf16"
    nbytes = lambda sd: sum(sd[k].numel() * sd[k].element_size() for k in ("m", "v"))
    assert 2 * nbytes(sd16) == nbytes(sd32)
    # bf16 checkpoint -> f32 optimizer: the widened values exactly
    a, _, _ = _model()
    oa = GPTAdam(a, lr=LR, state="f32")
    oa.load_state_dict(sd16)
    assert oa.m.dtype == torch.float32 and torch.equal(oa.m.cpu(), sd16["m"].float()) and torch.equal(oa.v.cpu(), sd16["v"].float())
    assert oa.state_seed == 5 and oa.state_dict()["step"] == 2
    # f32 checkpoint -> bf16 optimizer: the round-to-nearest-even image, once
    b, _, _ = _model()
    ob = GPTAdam(b, lr=LR, state="bf16")
    ob.load_state_dict(sd32)
    assert ob.m.dtype == torch.bfloat16 and torch.equal(_bits(ob.m.cpu()), _bits(sd32["m"].bfloat16())) and torch.equal(_bits(ob.v.cpu()), _bits(sd32["v"].bfloat16()))
    # a dict written before there was a state_format: f32, into either optimizer
    old = {k: v for k, v in sd32.items() if k not in ("state_format", "state_seed")}
    c, _, _ = _model()
    oc = GPTAdam(c, lr=LR, state="bf16", state_seed=9)
    oc.load_state_dict(old)
    assert torch.equal(_bits(oc.m.cpu()), _bits(sd32["m"].bfloat16())) and oc.state_seed == 9
    oa.load_state_dict(old)
    assert torch.equal(oa.m.cpu(), sd32["m"]) and torch.equal(oa.v.cpu(), sd32["v"])
    # and the loaded optimizers step
    for mm, oo in ((a, oa), (b, ob), (c, oc)):
        _steps(mm, oo, conds, codes, 1)
        assert oo.state_dict()["step"] == 3


def test_an_rq_prior_steps_with_bf16_state():
    import rq_backward_cases as RC
    from enhancing.engine.optim import GPTAdam
    from enhancing.modules.stage2.layers import RQTransformer
    m = RQTransformer(**RC.case_kwargs("rq_tiny"))
    m.load_state_dict(RC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=RC.PARAM_SEED), strict=True)
    conds, codes = (t.cuda() for t in RC.case_inputs("rq_tiny"))
    m = m.cuda()
    opt = GPTAdam(m, lr=LR, init_scale=1024.0, state="bf16")
    p0 = opt.p.clone()
    assert opt.m.dtype == torch.bfloat16 and opt.m.numel() == m.flat_grad.numel()
    m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
    g = m.flat_grad.clone()
    opt.step()
    assert opt.state_dict()["step"] == 1
    moved = opt.p != p0
    assert bool(moved.any()) and bool(torch.isfinite(opt.p).all())
    # the first step from zero moments: m = 0.1 g / scale, v = 0.04 (g / scale)^2 up to the rounding (no decay on the embeddings, 0.01 p elsewhere);
    # where the scaled gradient is above 1e-3 (1e-6 unscaled: v ~ 4e-14, far inside bf16's range) both moments moved
    nz = g.abs() > 1e-3
    assert bool(nz.any()) and bool((opt.m.float()[nz] != 0).all()) and bool((opt.v.float()[nz] > 0).all())
    logits = m(codes, conds)
    fresh = RQTransformer(**RC.case_kwargs("rq_tiny"))
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    assert torch.equal(_bits(logits), _bits(fresh.cuda()(codes, conds))), "the forward after the step read a stale operand copy"
