"""RQTransformer.forward_backward on the device against the fp64 restatement of tests/rq_backward_cases.py (itself held to the reference's golden
gradients and to autograd by tests/test_rq_backward_cpu.py), and the behaviour around it: the loss, chunks, repeated calls, the loss scale, refusals.

Yardstick and margins: those of tests/test_gpt_backward_gpu.py.  After division by loss_scale every parameter's gradient may be at most twice as far
from the fp64 gradient as the emulation's (the same restatement with the device path's rounding points), plus the format's rounding floor, in relative
Frobenius norm; for matrices the worst row at most twice the emulation's worst row.  attn.key.bias has an analytically zero gradient: it is measured
absolutely, against the norm of attn.query.bias's gradient."""
import pytest
import torch

import rq_backward_cases as BC
from util import floor16, rel, row_err

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
_REF, _EMU = {}, {}


def _model(name, code_sum="depth"):
    from enhancing.modules.stage2.layers import RQTransformer
    m = RQTransformer(**BC.case_kwargs(name), code_sum=code_sum)
    P = BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    conds, codes = BC.case_inputs(name)
    return m.cuda(), P, conds.cuda(), codes.cuda()


def _ref(name, mode, P, conds, codes):
    if (name, mode) not in _REF:
        _REF[(name, mode)] = BC.loss_and_grads(P, BC.case_dims(name), conds.cpu(), codes.cpu(), mode)
    return _REF[(name, mode)]


def _emu(name, mode, fmt, scale, P, conds, codes):
    key = (name, mode, fmt, scale)
    if key not in _EMU:
        dt = DT[fmt]
        _EMU[key] = BC.loss_and_grads(P, BC.case_dims(name), conds.cpu(), codes.cpu(), mode, rnd=lambda t: t.to(dt).to(torch.float64), loss_scale=scale)
    return _EMU[key]


def _grads(m):
    return {k: p.grad for k, p in m.named_parameters()}


def _bits(m):
    return torch.cat([p.grad.reshape(-1) for p in m.parameters()]).view(torch.int32)


CONFIGS = [(n, f, s, "depth", None) for f, s in (("fp16", 1024.0), ("bf16", 1.0)) for n in BC.CASES] + \
          [(n, "fp16", 1024.0, "channels", None) for n in ("rq_tiny", "rq_d3")] + [(n, "fp16", 1024.0, "depth", "tile") for n in ("rq_d3", "rq_d8")]


@pytest.mark.parametrize("name,fmt,scale,mode,attn", CONFIGS, ids=[f"{n}-{f}-{int(s)}-{m}" + ("-tile" if a else "") for n, f, s, m, a in CONFIGS])
def test_gradients_against_the_emulation(name, fmt, scale, mode, attn, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    if attn:
        monkeypatch.setenv("ENH_RQ_DEPTH_ATTN", attn)
    else:
        monkeypatch.delenv("ENH_RQ_DEPTH_ATTN", raising=False)
    dt = DT[fmt]
    m, P, conds, codes = _model(name, mode)
    loss = m.forward_backward(codes, conds, loss_scale=scale)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    _, _, mean = m(codes, conds, return_loss=True)
    assert loss.item() == mean.item() and torch.equal(loss.view(torch.int32), mean.view(torch.int32)), "the loss is not forward()'s bits"
    loss64, G64, _ = _ref(name, mode, P, conds, codes)
    _, GE, _ = _emu(name, mode, fmt, scale, P, conds, codes)
    G = _grads(m)
    assert sorted(G) == sorted(G64)
    qb = {k: G64[k].norm().item() for k in G64 if k.endswith("attn.query.bias")}
    worst, worst_row = (0.0, ""), (0.0, "")
    for k in sorted(G):
        g = G[k]
        assert g.dtype == torch.float32 and g.is_cuda and g.shape == P[k].shape, k
        assert bool(torch.isfinite(g).all()), f"{k}: non-finite gradient"
        got, emu, ref = g.double().cpu() / scale, GE[k].reshape(g.shape) / scale, G64[k].reshape(g.shape)
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
    print(f"{fmt} x{scale:g} {name} {mode}{' tile' if attn else ''}: loss {loss.item():.6f} (fp64 {loss64.item():.6f}); worst kernel / (2 emulation + floor) "
          f"{worst[0]:.3f} ({worst[1]}); worst row / emulation's worst row {worst_row[0]:.3f} ({worst_row[1]})")


def test_chunks_accumulate_in_a_fixed_order():
    """two images per chunk (2 + 2 + 1) against one chunk of five"""
    m, P, _, _ = _model("rq_tiny")
    C, Hs, Hd, Ls, Ld, V, T, D, B = BC.CASES["rq_tiny"]
    gen = torch.Generator().manual_seed(4)
    conds5 = torch.randint(0, BC.VOCAB_COND, (5, 1), generator=gen).cuda()
    codes5 = torch.randint(0, V, (5, T, D), generator=gen).cuda()
    res = []
    for cap in (2 * m.saved_bytes_per_image(), 1 << 40):
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


def test_a_second_call_sets_the_gradients_and_accumulate_adds():
    m, P, conds, codes = _model("rq_tiny")
    V, T, D = BC.CASES["rq_tiny"][5:8]
    other = (codes + 7) % V
    m.forward_backward(other, conds)
    m.forward_backward(codes, conds)
    a = _bits(m)
    m2, _, _, _ = _model("rq_tiny")
    m2.forward_backward(codes, conds)
    assert torch.equal(a, _bits(m2)), "the first call's codes left a trace"
    g = m.tok_emb_code.weight.grad
    fed = torch.zeros(V, dtype=torch.bool, device="cuda")
    flat = codes.reshape(codes.shape[0], -1)
    fed[flat[:, :-1].reshape(-1)] = True      # every code but the deepest of the last position
    assert bool((g[~fed] == 0).all()) and bool((g[fed].abs().sum(1) > 0).all())
    assert bool((m.pos_emb_code.grad[0, T - 1] == 0).all())
    assert all(p.grad.data_ptr() >= m.flat_grad.data_ptr() and p.grad.data_ptr() < m.flat_grad.data_ptr() + 4 * m.flat_grad.numel() for p in m.parameters())
    once = {k: v.clone() for k, v in _grads(m).items()}
    m.forward_backward(codes, conds, accumulate=True)
    for k, v in _grads(m).items():      # (a product adds its sum to what was there: the same value twice, to f32 rounding)
        if not k.endswith("attn.key.bias"):
            assert rel(v, 2 * once[k]) < 1e-5, (k, "accumulate=True did not double the gradient")


def test_a_device_loss_scale_gives_the_floats_bits():
    m, P, conds, codes = _model("rq_d3")
    la = m.forward_backward(codes, conds, loss_scale=512.0)
    a = _bits(m)
    lb = m.forward_backward(codes, conds, loss_scale=torch.full((1,), 512.0, device="cuda"))
    assert torch.equal(a, _bits(m)) and la.item() == lb.item()


def test_refusals():
    m, P, conds, codes = _model("rq_tiny")
    V = BC.CASES["rq_tiny"][5]
    with pytest.raises(ValueError):
        m.forward_backward(codes[:, :-1], conds)
    bad = codes.clone()
    bad[0, 3, 1] = V
    with pytest.raises(ValueError):
        m.forward_backward(bad, conds)
    with pytest.raises(NotImplementedError, match="exact-f32 backward is not built"):
        m.forward_backward(codes, conds, use_fp16=False)
    with pytest.raises(NotImplementedError, match="device"):
        m.forward_backward(codes.cpu(), conds.cpu())
