"""Stage-2 RQ training on the device: GPTAdam over an RQTransformer, CondTransformer.training_step / configure_optimizers and Trainer.fit with a
residual stage 1.  The tests of tests/test_gpt_train_gpu.py of the same names, on the RQ prior: the step is checked by REPLAY (the device's own gradients
fed to torch.optim.Adam on the CPU in fp64 with the golden grouping, tests/golden/rq_optim_groups.json) at tests/gpt_train_util.py's limit."""
import json

import pytest
import torch

import gpt_train_util as TU
import rq_backward_cases as BC

pytestmark = pytest.mark.gpu

LR = 1e-3


def _model(name, seed=BC.PARAM_SEED):
    from enhancing.modules.stage2.layers import RQTransformer
    m = RQTransformer(**BC.case_kwargs(name))
    m.load_state_dict(BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed), strict=True)
    conds, codes = BC.case_inputs(name)
    return m.cuda(), conds.cuda(), codes.cuda()


def _bits(ts):
    return [t.detach().clone().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64) for t in ts]


def _snapshot(m, conds, codes):
    """the bits of forward and forward_backward"""
    logits = m(codes, conds)
    loss = m.forward_backward(codes, conds, loss_scale=256.0)
    return _bits([logits, loss.view(1)] + [p.grad for p in m.parameters()])


def _weight_decays(m):
    """per parameter in registration order: the reference's grouping (the golden file's for rq_tiny; by the same rule, GPTAdam's own, elsewhere)"""
    from enhancing.engine.optim import gpt_param_groups
    decay, _ = gpt_param_groups(m)
    return [TU.WD if n in decay else 0.0 for n, _ in m.named_parameters()]


class Replay:
    """torch.optim.Adam on the CPU, in fp64 and in f32, over the prior's parameters"""

    def __init__(self, m):
        tensors, wds = [p.detach() for p in m.parameters()], _weight_decays(m)
        self.r64 = TU.TorchAdam(tensors, wds, LR, torch.float64)
        self.r32 = TU.TorchAdam(tensors, wds, LR, torch.float32)

    def step(self, grads, scale=1.0):
        self.r64.step(grads, scale)
        self.r32.step(grads, scale)

    def check(self, m, what):
        worst = (0.0, 0.0)
        for (n, p), a, b in zip(m.named_parameters(), self.r32.p(), self.r64.p()):
            r = TU.check_limit(p, a, b, f"{what} {n}")
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        print(f"{what}: worst error / limit over the parameters: norm {worst[0]:.3f}, element {worst[1]:.3f}")


def test_golden_grouping_is_what_the_replay_uses():
    with open(TU.os.path.join(TU.GOLD, "rq_optim_groups.json")) as f:
        gold = json.load(f)["rq_tiny"]
    m, _, _ = _model("rq_tiny")
    wd = {n: g["weight_decay"] for g in gold["groups"] for n in g["names"]}
    assert [wd[n] for n, _ in m.named_parameters()] == _weight_decays(m) and (gold["betas"], gold["eps"]) == (list(TU.BETAS), TU.EPS)


def test_construction_changes_no_value():
    from enhancing.engine.optim import GPTAdam
    m, conds, codes = _model("rq_tiny")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    before = _snapshot(m, conds, codes)
    opt = GPTAdam(m, lr=LR)
    assert list(m.state_dict()) == list(sd) and all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    lo, hi = opt.p.data_ptr(), opt.p.data_ptr() + 4 * opt.p.numel()
    assert all(lo <= p.data_ptr() < hi for p in m.parameters()) and opt.p.numel() == m.flat_grad.numel()
    assert not m._operands, "the per-layer operand copies were kept"
    alo, ahi = opt.arena.data_ptr(), opt.arena.data_ptr() + 2 * opt.arena.numel()
    ops = m._operand_copies(opt.dt)
    for stack in ("spatial", "depth"):
        assert all(alo <= ops[stack][0][k].data_ptr() < ahi for k in ("wqkv", "wproj", "w0", "w1")), stack
    after = _snapshot(m, conds, codes)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), "re-homing or the arena changed a result"
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0]


@pytest.mark.parametrize("name,fmt", [("rq_tiny", "fp16"), ("rq_d3", "fp16"), ("rq_tiny", "bf16")])
def test_three_steps_replayed_in_fp64_and_no_stale_copy(name, fmt, monkeypatch):
    from enhancing.engine.optim import GPTAdam
    from enhancing.modules.stage2.layers import RQTransformer
    monkeypatch.setenv("ENH_PRECISION", fmt)
    m, conds, codes = _model(name)
    opt = GPTAdam(m, lr=LR, init_scale=1024.0)
    assert (opt.loss_scale is None) == (fmt == "bf16")
    rep = Replay(m)
    for t in range(3):
        S = 1.0 if opt.loss_scale is None else opt.loss_scale
        m.forward_backward(codes, conds, loss_scale=S)
        grads = [p.grad.clone() for p in m.parameters()]
        opt.step()
        rep.step(grads, 1.0 if fmt == "bf16" else 1.0 / 1024.0)
        rep.check(m, f"{name} {fmt} step {t + 1}")
    assert opt.state_dict()["step"] == 3
    # stale-copy check: every operand and bias copy the forward reads must be the stepped weights
    logits = m(codes, conds)
    fresh = RQTransformer(**BC.case_kwargs(name))
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    fresh = fresh.cuda()
    assert torch.equal(logits.view(torch.int32), fresh(codes, conds).view(torch.int32)), "the forward after three steps read a stale operand or bias copy"


def test_an_overflow_drops_the_step_and_halves_the_scale():
    from enhancing.engine.optim import GPTAdam
    m, conds, codes = _model("rq_tiny")
    opt = GPTAdam(m, lr=LR, init_scale=2.0 ** 24)      # dlogits up to 2^24 / (B T D = 40) = 4.2e5: beyond fp16's 65504
    before = _bits([opt.p, opt.m, opt.v, opt.state]) + [opt.arena.clone().view(torch.int16)]
    m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
    assert not bool(torch.isfinite(m.flat_grad).all())
    opt.step()
    after = _bits([opt.p, opt.m, opt.v, opt.state]) + [opt.arena.clone().view(torch.int16)]
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "the dropped step wrote something"
    assert opt.loss_scale.item() == 2.0 ** 23 and opt.scaler.tracker.item() == 0


def _cond_transformer():
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    from test_rq_forward_gpu import _tiny_cfg
    torch.manual_seed(0)
    cfg = AttrDict.wrap(_tiny_cfg())
    return CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand(3, 3, 32, 32, generator=g).cuda(), "class": torch.randint(0, 3, (3,), generator=g).cuda()}


def test_accumulation_through_training_step():
    ct = _cond_transformer()
    ct.learning_rate = LR
    ct.transformer.cuda()
    with pytest.raises(NotImplementedError, match="RQ training needs its optimizer first"):
        ct.training_step(_batch(1), 0)
    (opt,), scheds = ct.configure_optimizers()
    assert scheds == [] and opt.loss_scale.item() == 65536.0
    opt.scaler.scale_t.fill_(256.0)
    rq = ct.transformer
    b1, b2 = _batch(1), _batch(2)
    l1 = ct.training_step(b1, 0)
    assert ct.logged["train/total_loss"] is l1 and l1.item() == ct.validation_step(b1, 0).item(), "the returned loss is the unscaled one"
    g1 = [p.grad.clone() for p in rq.parameters()]
    ct.training_step(b2, 1)
    g2 = [p.grad.clone() for p in rq.parameters()]
    ct.training_step(b1, 0, zero_grad=True)
    ct.training_step(b2, 1, zero_grad=False)
    total = torch.cat([(a.double() + b.double()).reshape(-1) for a, b in zip(g1, g2)])
    got = torch.cat([p.grad.double().reshape(-1) for p in rq.parameters()])
    assert ((got - total).norm() / total.norm()).item() < 1e-6
    # Trainer's accumulate_grad_batches = 2: grad_scale 1/2, one step on the window's sum
    tensors, wds = [p.detach() for p in rq.parameters()], _weight_decays(rq)
    r64, r32 = TU.TorchAdam(tensors, wds, LR, torch.float64), TU.TorchAdam(tensors, wds, LR, torch.float32)
    opt.grad_scale = 0.5
    opt.step()
    assert opt.state_dict()["step"] == 1
    summed = [a.double() + b.double() for a, b in zip(g1, g2)]
    r64.step(summed, 0.5 / 256.0)
    r32.step([s.float() for s in summed], 0.5 / 256.0)
    for (n, p), a, b in zip(rq.named_parameters(), r32.p(), r64.p()):
        TU.check_limit(p, a, b, f"accumulated step {n}")


def test_state_dict_round_trip():
    from enhancing.engine.optim import GPTAdam
    m, conds, codes = _model("rq_tiny")
    opt = GPTAdam(m, lr=LR, init_scale=1024.0)
    for _ in range(2):
        m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
        opt.step()
    sd, weights = opt.state_dict(), {k: v.clone() for k, v in m.state_dict().items()}
    assert sd["step"] == 2 and not sd["m"].is_cuda and sd["m"].numel() == opt.p.numel()
    m2, _, _ = _model("rq_tiny", seed=BC.PARAM_SEED + 1)
    opt2 = GPTAdam(m2, lr=LR)
    m2.load_state_dict(weights)       # in place, with torch: the arena is recast from the masters at its next use
    opt2.load_state_dict(sd)
    for mm, oo in ((m, opt), (m2, opt2)):
        mm.forward_backward(codes, conds, loss_scale=oo.loss_scale)
        oo.step()
    for a, b in ((opt.p, opt2.p), (opt.m, opt2.m), (opt.v, opt2.v), (opt.state, opt2.state), (opt.scaler.scale_t, opt2.scaler.scale_t)):
        assert torch.equal(_bits([a])[0], _bits([b])[0])
    assert torch.equal(opt.arena.view(torch.int16), opt2.arena.view(torch.int16)) and opt2.state_dict()["step"] == 3


class _Data:
    """a data module as Trainer.fit uses one: the same batch of the tiny CondTransformer's shape, twenty times"""
    dataset_configs = {}

    def setup(self, rank=0, world=1):
        pass

    def train_dataloader(self):
        b = _batch(0)
        return [{"image": b["image"].cpu(), "class": b["class"].cpu()}] * 20


def test_twenty_steps_through_the_trainer_lower_the_loss(tmp_path):
    from enhancing.engine.trainer import Trainer
    ct = _cond_transformer()
    ct.learning_rate = LR
    w0 = ct.transformer.head.weight.detach().clone()
    Trainer(max_epochs=1, max_steps=20, precision=16, default_root_dir=str(tmp_path), log_every_n_steps=1).fit(ct, _Data())
    recs = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    losses = [r["train/total_loss"] for r in recs]
    print("train/total_loss: " + " ".join(f"{x:.4f}" for x in losses))
    assert len(recs) == 20 and [r["step"] for r in recs] == list(range(1, 21))
    assert not torch.equal(ct.transformer.head.weight.detach().cpu(), w0.cpu()), "no step was applied"
    assert losses[-1] < losses[0], "twenty steps on one repeated batch did not lower train/total_loss"
