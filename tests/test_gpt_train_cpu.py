"""Stage-2 training, the parts that need no device: the port's decay / no-decay partition against the reference's own configure_optimizers
(tests/golden/gpt_optim_groups.json), the step kernel's arithmetic (restated in fp64: tests/gpt_train_util.py adam_step64) on the gradients of the fp64
restatement of tests/gpt_backward_cases.py against three steps of the reference's optimizer on the reference's GPT in fp64
(tests/golden/gpt_train_tiny.npz, tools/make_golden_gpt_train.py), and the refusals.

The trajectory pins the grouping, the betas, eps and the L2 form of the decay: any of them wrong moves a parameter by a fraction of lr = 1e-3 per step,
while the two fp64 computations differ by rounding (their gradients agree to ~1e-12 relative; Adam's update lr m / (sqrt(v) + eps) changes by at most
lr x that relative error for |g| >> eps and by lr dg / eps below it).  Limits: 1e-9 absolute per element (1e-6 of one step), 1e-6 of the change's norm
for the tensors the golden keeps as projections, 1e-9 relative for the losses."""
import os

import numpy as np
import pytest
import torch

import gpt_backward_cases as BC
import gpt_train_util as TU


@pytest.mark.parametrize("case", ["tiny", "h3"])
def test_partition_is_the_references(case):
    from enhancing.engine.optim import gpt_param_groups
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**BC.case_kwargs(case))
    decay, no_decay = gpt_param_groups(m)
    gold = TU.golden_groups(case)
    assert gold["betas"] == [0.9, 0.96] and gold["eps"] == 1e-8
    by_wd = {g["weight_decay"]: g["names"] for g in gold["groups"]}
    assert sorted(by_wd) == [0.0, 0.01]
    assert decay == by_wd[0.01] and no_decay == by_wd[0.0]
    names = [n for n, _ in m.named_parameters()]
    assert sorted(decay + no_decay) == sorted(names) and not set(decay) & set(no_decay)


def test_three_steps_reproduce_the_references_trajectory():
    from enhancing.engine.optim import gpt_param_groups
    from enhancing.modules.stage2.layers import GPT
    gold = np.load(os.path.join(TU.GOLD, "gpt_train_tiny.npz"))
    m = GPT(**BC.case_kwargs("tiny"))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sorted(shapes) == list(gold["state_names"])
    P0 = BC.make_params(shapes, seed=int(gold["param_seed"]))
    P = {k: v.double().clone() for k, v in P0.items()}
    decay, _ = gpt_param_groups(m)
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    conds, codes = torch.from_numpy(gold["conds"]), torch.from_numpy(gold["codes"]).long()
    lr = float(gold["lr"])
    for t in range(1, int(gold["steps"]) + 1):
        loss, G, _ = BC.loss_and_grads(P, BC.case_dims("tiny"), conds, codes)
        ref = float(gold["loss64"][t - 1])
        assert abs(loss.item() - ref) <= 1e-9 * ref, (t, loss.item(), ref)
        for k in P:
            TU.adam_step64(P[k], G[k].reshape(P[k].shape), M[k], V[k], t, lr, TU.WD if k in decay else 0.0)
    worst = 0.0
    for i, k in enumerate(sorted(shapes)):
        if "p." + k in gold.files:
            err = (P[k] - torch.from_numpy(gold["p." + k])).abs().max().item()
            assert err <= 1e-9, (k, err)
            worst = max(worst, err / 1e-9)
        else:
            n, r, l = BC.projections(P[k] - P0[k].double(), int(gold["proj_seed"]) + i)
            gn = float(gold["n." + k])
            assert gn > 0 and abs(n.item() - gn) <= 1e-6 * gn, (k, n.item(), gn)
            er = (r - torch.from_numpy(gold["r." + k])).norm().item() / torch.from_numpy(gold["r." + k]).norm().item()
            el = (l - torch.from_numpy(gold["l." + k])).norm().item() / torch.from_numpy(gold["l." + k]).norm().item()
            assert er <= 1e-6 and el <= 1e-6, (k, er, el)
            worst = max(worst, er / 1e-6, el / 1e-6)
    print(f"worst error / limit {worst:.2e}")


def test_refusals_on_a_bare_object_and_on_a_cpu_model():
    from enhancing.engine.optim import GPTAdam
    from enhancing.modules.stage2.layers import GPT
    from enhancing.modules.stage2.transformer import CondTransformer
    ct = CondTransformer.__new__(CondTransformer)
    with pytest.raises(NotImplementedError, match="training.*configure_optimizers"):
        ct.training_step({}, 0)
    with pytest.raises(NotImplementedError, match="training.*learning_rate"):
        ct.configure_optimizers()
    m = GPT(**BC.case_kwargs("tiny"))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(RuntimeError, match="device"):
        GPTAdam(m, lr=1e-3)
    assert m._arena is None and all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


def test_segment_table_checks():
    """the table builder refuses what the kernel would trust: unsorted or overlapping segments, bounds off the 64-element grid, destinations outside
    the arena or shared"""
    from enhancing import _C
    ok = [(0, 64, -1, 0.0), (64, 192, 0, 0.01)]
    t = _C.adam_segment_table(ok, 256, 128, "cpu")
    assert t.dtype == torch.int64 and tuple(t.shape) == (2, 4) and t[1, :3].tolist() == [64, 192, 0]
    assert np.frombuffer(t[1, 3:].numpy().tobytes(), dtype=np.float32)[0] == np.float32(0.01)
    for bad in ([(64, 128, -1, 0.0), (0, 64, -1, 0.0)], [(0, 128, -1, 0.0), (64, 192, -1, 0.0)], [(0, 32, -1, 0.0)], [(0, 320, -1, 0.0)],
                [(0, 64, 96, 0.0)], [(0, 64, 4, 0.0)], [(0, 64, 0, 0.0), (64, 128, 32, 0.0)], []):
        with pytest.raises(RuntimeError, match="adam_segment_table"):
            _C.adam_segment_table(bad, 256, 128, "cpu")
