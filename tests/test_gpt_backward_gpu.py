"""GPT.forward_backward on the device against the fp64 restatement of tests/gpt_backward_cases.py (itself held to the reference's golden gradients
and to autograd by tests/test_gpt_backward_cpu.py), and the behaviour around it: the loss, chunks, repeated calls, reloaded weights, CondTransformer.

Yardstick (the rule of tests/test_gpt_forward_gpu.py): the same restatement with the device path's rounding points (the emulation).  After division by
loss_scale every parameter's gradient may be at most twice as far from the fp64 gradient as the emulation's, plus the format's rounding floor, in
relative Frobenius norm; for matrices the worst row (util.row_err) at most twice the emulation's worst row.  attn.key.bias has an analytically zero
gradient (softmax is shift-invariant): it is measured absolutely, against the norm of attn.query.bias's gradient."""
import pytest
import torch

import gpt_backward_cases as BC
from util import floor16, rel, row_err

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
_REF, _EMU = {}, {}


def _model(name):
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**BC.case_kwargs(name))
    P = BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    conds, codes = BC.case_inputs(name)
    return m.cuda(), P, conds.cuda(), codes.cuda()


def _ref(name, P, conds, codes):
    if name not in _REF:
        _REF[name] = BC.loss_and_grads(P, BC.case_dims(name), conds.cpu(), codes.cpu())
    return _REF[name]


def _emu(name, fmt, scale, P, conds, codes):
    if (name, fmt, scale) not in _EMU:
        dt = DT[fmt]
        _EMU[(name, fmt, scale)] = BC.loss_and_grads(P, BC.case_dims(name), conds.cpu(), codes.cpu(), rnd=lambda t: t.to(dt).to(torch.float64), loss_scale=scale)
    return _EMU[(name, fmt, scale)]


def _grads(m):
    return {k: p.grad for k, p in m.named_parameters()}


def _bits(m):
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()]).view(torch.int32)


CONFIGS = [(n, "fp16", 1024.0) for n in BC.CASES] + [(n, "bf16", 1.0) for n in BC.CASES] + [("tiny", "fp16", 1.0)]


@pytest.mark.parametrize("name,fmt,scale", CONFIGS, ids=[f"{n}-{f}-{int(s)}" for n, f, s in CONFIGS])
def test_gradients_against_the_emulation(name, fmt, scale, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = DT[fmt]
    m, P, conds, codes = _model(name)
    loss = m.forward_backward(codes, conds, loss_scale=scale)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    _, _, mean = m(codes, conds, return_loss=True)
    assert loss.item() == mean.item() and torch.equal(loss.view(torch.int32), mean.view(torch.int32)), "the loss is not forward()'s bits"
    loss64, G64, _ = _ref(name, P, conds, codes)
    _, GE, _ = _emu(name, fmt, scale, P, conds, codes)
    G = _grads(m)
    assert sorted(G) == sorted(G64)
    qb = {k: G64[k].norm().item() for k in G64 if k.endswith("attn.query.bias")}
    worst, worst_row = (0.0, ""), (0.0, "")
    for k in sorted(G):
        g = G[k]
        assert g.dtype == torch.float32 and g.is_cuda and g.shape == P[k].shape, k
        assert bool(torch.isfinite(g).all()), f"{k}: non-finite gradient"
        got, emu, ref = g.double().cpu() / scale, GE[k] / scale, G64[k]
        if k.endswith("attn.key.bias"):
            n = qb[k.replace("key", "query")]
            ek, ee, fl = (got - ref).norm().item() / n, (emu - ref).norm().item() / n, floor16(G64[k.replace("key", "query")], dt)
        else:
            ek, ee, fl = rel(got, ref), rel(emu, ref), floor16(ref, dt)
        worst = max(worst, (ek / (2 * ee + fl), k))
        assert ek <= 2 * ee + fl, (name, fmt, k, ek, ee, fl)
        if ref.dim() >= 2 and ref.numel() > ref.shape[-1] and not k.endswith("key.bias"):
            wk, we = row_err(got, ref, ref.shape[-1]).max().item(), row_err(emu, ref, ref.shape[-1]).max().item()
            worst_row = max(worst_row, (wk / we, k))
            assert wk <= 2 * we, (name, fmt, k, "worst row", wk, we)
    print(f"{fmt} x{scale:g} {name}: loss {loss.item():.6f} (fp64 {loss64.item():.6f}); worst kernel / (2 emulation + floor) {worst[0]:.3f} ({worst[1]}); "
          f"worst row / emulation's worst row {worst_row[0]:.3f} ({worst_row[1]})")


def test_chunks_accumulate_in_a_fixed_order():
    """two sequences per chunk (2 + 2 + 1) against one chunk of five, on the data of test_gpt_forward_gpu.test_chunks_equal_separate_calls"""
    m, P, _, _ = _model("tiny")
    C, H, L, V, T, B = BC.CASES["tiny"]
    gen = torch.Generator().manual_seed(4)
    conds5 = torch.randint(0, BC.VOCAB_COND, (5, 1), generator=gen).cuda()
    codes5 = torch.randint(0, V, (5, T), generator=gen).cuda()
    res = []
    for cap in (2 * T * m.saved_bytes_per_token(), 1 << 40):
        m.backward_saved_cap = cap
        la = m.forward_backward(codes5, conds5, loss_scale=1024.0)
        a = _bits(m)
        m.flat_grad.fill_(float("nan"))      # what a second run leaves does not depend on what was there
        lb = m.forward_backward(codes5, conds5, loss_scale=1024.0)
        assert torch.equal(a, _bits(m)) and la.item() == lb.item(), "two runs differ"
        res.append((la.item(), {k: g.clone() for k, g in _grads(m).items()}))
    assert abs(res[0][0] - res[1][0]) < 1e-3
    for k in res[0][1]:
        if not k.endswith("attn.key.bias"):
            assert rel(res[0][1][k], res[1][1][k]) < 2e-3, k


def test_a_second_call_sets_the_gradients():
    m, P, conds, codes = _model("tiny")
    V = BC.CASES["tiny"][3]
    other = (codes + 7) % V
    m.forward_backward(other, conds)
    m.forward_backward(codes, conds)
    a = _bits(m)
    m2, _, _, _ = _model("tiny")
    m2.forward_backward(codes, conds)
    assert torch.equal(a, _bits(m2)), "the first call's codes left a trace"
    g = m.tok_emb_code.weight.grad
    fed = torch.zeros(V, dtype=torch.bool, device="cuda")
    fed[codes[:, :-1].reshape(-1)] = True
    assert bool((g[~fed] == 0).all()) and bool((g[fed].abs().sum(1) > 0).all())
    assert all(p.grad.data_ptr() >= m.flat_grad.data_ptr() and p.grad.data_ptr() < m.flat_grad.data_ptr() + 4 * m.flat_grad.numel() for p in m.parameters())


def test_load_state_dict_refreshes_the_operand_copies():
    m, P, conds, codes = _model("tiny")
    m.forward_backward(codes, conds)
    a = {k: g.clone() for k, g in _grads(m).items()}
    P2 = BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=BC.PARAM_SEED + 1)
    m.load_state_dict(P2)
    m.forward_backward(codes, conds)
    assert rel(m.head.weight.grad, a["head.weight"]) > 0.5, "the second backward still ran the old weights"
    m.load_state_dict(P)
    m.forward_backward(codes, conds)
    assert all(torch.equal(g.view(torch.int32), a[k].view(torch.int32)) for k, g in _grads(m).items())


def test_refusals():
    m, P, conds, codes = _model("tiny")
    V = BC.CASES["tiny"][3]
    with pytest.raises(ValueError):
        m.forward_backward(codes[:, :-1], conds)
    bad = codes.clone()
    bad[0, 3] = V
    with pytest.raises(ValueError):
        m.forward_backward(bad, conds)
    with pytest.raises(NotImplementedError, match="exact-f32 backward is not built"):
        m.forward_backward(codes, conds, use_fp16=False)
    with pytest.raises(NotImplementedError, match="device"):
        m.forward_backward(codes.cpu(), conds.cpu())


def test_cond_transformer_loss_and_grads():
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
    ct = CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer, code_shape=[16])
    batch = {"image": torch.rand(3, 3, 32, 32).cuda(), "class": torch.tensor([0, 2, 1]).cuda()}
    loss = ct.loss_and_grads(batch, 0, loss_scale=256.0)
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and ct.logged["train/total_loss"] is loss
    assert loss.item() == ct.validation_step(batch, 0).item()
    for k, p in ct.transformer.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if not k.endswith("attn.key.bias") and not k.startswith("tok_emb"):
            assert p.grad.abs().max().item() > 0, k
    with pytest.raises(NotImplementedError, match="training"):
        ct.training_step(batch, 0)
    with pytest.raises(NotImplementedError, match="training"):
        ct.configure_optimizers()
