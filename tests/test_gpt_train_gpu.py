"""Stage-2 training on the device: GPTAdam over a GPT (`tiny`, and the three-head `h3` of tests/gpt_cases.py), CondTransformer.training_step /
configure_optimizers and Trainer.fit.

The step is checked by REPLAY: after every forward_backward the device's own gradients are cloned and fed to torch.optim.Adam on the CPU in fp64 with
the golden grouping (tests/golden/gpt_optim_groups.json); the parameters must agree at the kernel's limit (tests/gpt_train_util.py: 4 x the error of
the same replay in f32 + one ulp).  The limit can be that tight because the replay checks the step, not the backward."""
import json
import os

import pytest
import torch

import gpt_backward_cases as BC
import gpt_train_util as TU

pytestmark = pytest.mark.gpu

CASES = ["tiny", "h3"]
LR = 1e-3


def _model(name, seed=BC.PARAM_SEED):
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**BC.case_kwargs(name))
    m.load_state_dict(BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed), strict=True)
    conds, codes = BC.case_inputs(name)
    return m.cuda(), conds.cuda(), codes.cuda()


def _bits(ts):
    return [t.detach().clone().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64) for t in ts]


def _snapshot(m, conds, codes):
    """the bits of forward, seeded sample and forward_backward"""
    logits = m(codes, conds)
    sl, sc = m.sample(conds, top_k=20, seed=3)
    loss = m.forward_backward(codes, conds, loss_scale=256.0)
    return _bits([logits, sl, sc, loss.view(1)] + [p.grad for p in m.parameters()])


class Replay:
    """torch.optim.Adam on the CPU, in fp64 and in f32, over the GPT's parameters with the golden grouping"""

    def __init__(self, m, name):
        gold = TU.golden_groups(name)
        wd = {n: g["weight_decay"] for g in gold["groups"] for n in g["names"]}
        self.names = [n for n, _ in m.named_parameters()]
        tensors = [p.detach() for _, p in m.named_parameters()]
        self.r64 = TU.TorchAdam(tensors, [wd[n] for n in self.names], LR, torch.float64, betas=tuple(gold["betas"]), eps=gold["eps"])
        self.r32 = TU.TorchAdam(tensors, [wd[n] for n in self.names], LR, torch.float32, betas=tuple(gold["betas"]), eps=gold["eps"])

    def step(self, grads, scale=1.0, **kw):
        self.r64.step(grads, scale, **kw)
        self.r32.step(grads, scale, **kw)

    def check(self, m, what):
        worst = (0.0, 0.0)
        for (n, p), a, b in zip(m.named_parameters(), self.r32.p(), self.r64.p()):
            r = TU.check_limit(p, a, b, f"{what} {n}")
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        print(f"{what}: worst error / limit over the parameters: norm {worst[0]:.3f}, element {worst[1]:.3f}")


@pytest.mark.parametrize("name", CASES)
def test_construction_changes_no_value(name):
    from enhancing.engine.optim import GPTAdam
    m, conds, codes = _model(name)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    before = _snapshot(m, conds, codes)
    opt = GPTAdam(m, lr=LR)
    assert list(m.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    lo, hi = opt.p.data_ptr(), opt.p.data_ptr() + 4 * opt.p.numel()
    assert all(lo <= p.data_ptr() < hi for p in m.parameters()) and opt.p.numel() == m.flat_grad.numel()
    assert not m._operands, "the per-layer operand copies were kept"
    W = m._operand_copies(opt.dt)["layers"][0]
    alo, ahi = opt.arena.data_ptr(), opt.arena.data_ptr() + 2 * opt.arena.numel()
    assert all(alo <= W[k].data_ptr() < ahi for k in ("wqkv", "wproj", "w0", "w1"))
    after = _snapshot(m, conds, codes)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), "re-homing or the arena changed a result"
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0] and all(g["betas"] == (0.9, 0.96) and g["lr"] == LR for g in opt.param_groups)
    m.load_state_dict(sd)      # copies in place: the parameters stay in the flat buffer
    assert all(lo <= p.data_ptr() < hi for p in m.parameters())


@pytest.mark.parametrize("name,fmt", [("tiny", "fp16"), ("h3", "fp16"), ("tiny", "bf16")])
def test_three_steps_replayed_in_fp64_and_no_stale_copy(name, fmt, monkeypatch):
    from enhancing.engine.optim import GPTAdam
    from enhancing.modules.stage2.layers import GPT
    monkeypatch.setenv("ENH_PRECISION", fmt)
    m, conds, codes = _model(name)
    opt = GPTAdam(m, lr=LR, init_scale=1024.0)
    assert (opt.loss_scale is None) == (fmt == "bf16")
    rep = Replay(m, name)
    for t in range(3):
        S = 1.0 if opt.loss_scale is None else opt.loss_scale
        m.forward_backward(codes, conds, loss_scale=S)
        grads = [p.grad.clone() for p in m.parameters()]
        opt.step()
        rep.step(grads, 1.0 if fmt == "bf16" else 1.0 / 1024.0)
        rep.check(m, f"{name} {fmt} step {t + 1}")
    sd = opt.state_dict()
    assert sd["step"] == 3 and (fmt == "bf16" or (sd["scaler"]["scale"].item() == 1024.0 and sd["scaler"]["tracker"].item() == 3))
    # stale-copy check: every operand and bias copy the forward reads must be the stepped weights
    logits = m(codes, conds)
    fresh = GPT(**BC.case_kwargs(name))
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    fresh = fresh.cuda()
    assert torch.equal(logits.view(torch.int32), fresh(codes, conds).view(torch.int32)), "the forward after three steps read a stale operand or bias copy"
    _, c1 = m.sample(conds, top_k=20, seed=3)
    _, c2 = fresh.sample(conds, top_k=20, seed=3)
    assert torch.equal(c1, c2)


def test_an_overflow_drops_the_step_and_halves_the_scale():
    from enhancing.engine.optim import GPTAdam
    m, conds, codes = _model("tiny")
    opt = GPTAdam(m, lr=LR, init_scale=2.0 ** 24)      # dlogits up to 2^24 / (B T = 40) = 4.2e5: beyond fp16's 65504
    before = _bits([opt.p, opt.m, opt.v, opt.state]) + [opt.arena.clone().view(torch.int16)]
    m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
    assert not bool(torch.isfinite(m.flat_grad).all())
    opt.step()
    after = _bits([opt.p, opt.m, opt.v, opt.state]) + [opt.arena.clone().view(torch.int16)]
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "the dropped step wrote something"
    assert opt.loss_scale.item() == 2.0 ** 23 and opt.scaler.tracker.item() == 0
    n = 16
    for _ in range(n - 1):
        m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
        opt.step()
    applied = opt.state_dict()["step"]
    assert 1 <= applied < n, applied
    assert opt.loss_scale.item() == 2.0 ** (24 - (n - applied)), "every dropped step halves the scale once, an applied one leaves it"
    assert not torch.equal(before[0], _bits([opt.p])[0]), "later steps did not proceed"


def _cond_transformer():
    """the tiny CondTransformer of tests/test_gpt_backward_gpu.py"""
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


def test_accumulation_through_training_step():
    ct = _cond_transformer()
    ct.learning_rate = LR
    ct.transformer.cuda()
    (opt,), scheds = ct.configure_optimizers()
    assert scheds == [] and opt.loss_scale.item() == 65536.0
    opt.scaler.scale_t.fill_(256.0)
    gpt = ct.transformer
    b1, b2 = _batch(1), _batch(2)
    l1 = ct.training_step(b1, 0)
    assert ct.logged["train/total_loss"] is l1 and l1.item() == ct.validation_step(b1, 0).item(), "the returned loss is the unscaled one"
    g1 = [p.grad.clone() for p in gpt.parameters()]
    ct.training_step(b2, 1)
    g2 = [p.grad.clone() for p in gpt.parameters()]
    ct.training_step(b1, 0, zero_grad=True)
    ct.training_step(b2, 1, zero_grad=False)
    total = torch.cat([(a.double() + b.double()).reshape(-1) for a, b in zip(g1, g2)])
    got = torch.cat([p.grad.double().reshape(-1) for p in gpt.parameters()])
    assert ((got - total).norm() / total.norm()).item() < 1e-6
    # Trainer's accumulate_grad_batches = 2: grad_scale 1/2, one step on the window's sum
    names = [n for n, _ in gpt.named_parameters()]
    cfg = {k: tuple(v.shape) for k, v in gpt.state_dict().items()}
    assert sorted(cfg) == sorted(names)
    gold = TU.golden_groups("tiny")        # the names of a two-layer GPT: this one has one layer, a subset
    wd = {n: g["weight_decay"] for g in gold["groups"] for n in g["names"]}
    tensors = [p.detach() for p in gpt.parameters()]
    r64 = TU.TorchAdam(tensors, [wd[n] for n in names], LR, torch.float64)
    r32 = TU.TorchAdam(tensors, [wd[n] for n in names], LR, torch.float32)
    opt.grad_scale = 0.5
    opt.step()
    assert opt.state_dict()["step"] == 1
    summed = [a.double() + b.double() for a, b in zip(g1, g2)]
    r64.step(summed, 0.5 / 256.0)
    r32.step([s.float() for s in summed], 0.5 / 256.0)
    for (n, p), a, b in zip(gpt.named_parameters(), r32.p(), r64.p()):
        TU.check_limit(p, a, b, f"accumulated step {n}")


def test_state_dict_round_trip():
    from enhancing.engine.optim import GPTAdam
    m, conds, codes = _model("tiny")
    opt = GPTAdam(m, lr=LR, init_scale=1024.0)
    for _ in range(2):
        m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
        opt.step()
    sd, weights = opt.state_dict(), {k: v.clone() for k, v in m.state_dict().items()}
    assert sd["step"] == 2 and not sd["m"].is_cuda and sd["m"].numel() == opt.p.numel()
    m2, _, _ = _model("tiny", seed=BC.PARAM_SEED + 1)
    opt2 = GPTAdam(m2, lr=LR)
    m2.load_state_dict(weights)       # in place, with torch: the arena is recast from the masters at its next use
    opt2.load_state_dict(sd)
    for mm, oo in ((m, opt), (m2, opt2)):
        mm.forward_backward(codes, conds, loss_scale=oo.loss_scale)
        oo.step()
    for a, b in ((opt.p, opt2.p), (opt.m, opt2.m), (opt.v, opt2.v), (opt.state, opt2.state), (opt.scaler.scale_t, opt2.scaler.scale_t)):
        assert torch.equal(_bits([a])[0], _bits([b])[0])
    assert torch.equal(opt.arena.view(torch.int16), opt2.arena.view(torch.int16)) and opt2.state_dict()["step"] == 3


def test_overfitting_one_batch_follows_the_fp64_curve():
    """a coarse guard, not a measurement: 20 steps at lr 1e-3 on one fixed batch; the device's loss must fall by at least half of what the fp64
    restatement's falls under the same optimizer"""
    from enhancing.engine.optim import GPTAdam, gpt_param_groups
    m, conds, codes = _model("tiny")
    opt = GPTAdam(m, lr=LR, init_scale=1024.0)
    dev = []
    for _ in range(20):
        dev.append(m.forward_backward(codes, conds, loss_scale=opt.loss_scale))
        opt.step()
    dev = [x.item() for x in dev] + [m(codes, conds, return_loss=True)[2].item()]
    assert opt.state_dict()["step"] == 20
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    P = {k: v.double() for k, v in BC.make_params(shapes).items()}
    decay, _ = gpt_param_groups(m)
    M, V = {k: torch.zeros_like(v) for k, v in P.items()}, {k: torch.zeros_like(v) for k, v in P.items()}
    ref = []
    for t in range(1, 21):
        loss, G, _ = BC.loss_and_grads(P, BC.case_dims("tiny"), conds.cpu(), codes.cpu())
        ref.append(loss.item())
        for k in P:
            TU.adam_step64(P[k], G[k].reshape(P[k].shape), M[k], V[k], t, LR, TU.WD if k in decay else 0.0)
    ref.append(BC.loss_and_grads(P, BC.case_dims("tiny"), conds.cpu(), codes.cpu())[0].item())
    print("loss, device: " + " ".join(f"{x:.4f}" for x in dev))
    print("loss, fp64:   " + " ".join(f"{x:.4f}" for x in ref))
    assert dev[0] - dev[-1] >= 0.5 * (ref[0] - ref[-1]) > 0


class _Data:
    """a data module as Trainer.fit uses one: batches of the tiny CondTransformer's shape"""
    dataset_configs = {}

    def setup(self, rank=0, world=1):
        pass

    def train_dataloader(self):
        return [{"image": b["image"].cpu(), "class": b["class"].cpu()} for b in (_batch(s) for s in range(4))]


def test_through_the_trainer(tmp_path):
    from enhancing.engine.trainer import Trainer
    ct = _cond_transformer()
    ct.learning_rate = LR
    with pytest.raises(NotImplementedError, match="exact-f32"):
        Trainer(max_steps=1, precision=32, default_root_dir=str(tmp_path / "no")).fit(ct, _Data())
    w0 = ct.transformer.head.weight.detach().clone()
    Trainer(max_epochs=1, max_steps=3, precision=16, default_root_dir=str(tmp_path), log_every_n_steps=1).fit(ct, _Data())
    recs = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    assert len(recs) == 3 and all("train/total_loss" in r and r["train/total_loss"] > 0 for r in recs) and [r["step"] for r in recs] == [1, 2, 3]
    assert not torch.equal(ct.transformer.head.weight.detach().cpu(), w0.cpu()), "no step was applied"
    ck = torch.load(os.path.join(tmp_path, "ckpt", "epoch=00.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and ck["optimizer"]["step"] + int(round(16 - torch.log2(ck["optimizer"]["scaler"]["scale"]).item())) == 3
    ct2 = _cond_transformer()
    ct2.load_state_dict(ck["state_dict"])
    for k, v in ct.transformer.state_dict().items():
        assert torch.equal(ct2.transformer.state_dict()[k], v.cpu()), k
