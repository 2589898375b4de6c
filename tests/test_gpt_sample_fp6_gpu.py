"""sample(weights="fp6") of both priors: the MXFP6 weight path against the model it claims to run, which is the case's parameters with every Block
Linear weight replaced by dequant(quant(W)) (tests/mxfp6_util.py; the head untouched).  The yardstick is the project's 16-bit rule against THAT
model: with gold_q its fp64 logits and emu the plain-torch step with every operand and cache entry rounded to the format,
rel(got, gold_q) <= 2 rel(emu, gold_q) + floor16(gold_q), per step and over the sequence.  The dequantized weights are 16-bit values in either
format (tests/test_mxfp6_cpu.py), so the emulation's rounding of W changes nothing and gpt_cases.step_logits is reused as it stands.

Worst kernel / (2 emulation + floor) over the steps, measured on MI355X, fp16 / bf16: tiny 0.432 / 0.417, hs384 0.400 / 0.402,
h3 0.433 / 0.412, rq_d3 0.450 / 0.426.  The quantization itself moves the logits by 0.036 - 0.046 against the 16-bit path's 5e-4 (fp16), so the two
orderings that show the weights really are the quantized ones are not close calls."""
import pytest
import torch

import gpt_cases as GC
import rq_sample_cases as SC
from mxfp6_util import quantized_params, row_bytes
from util import floor16, rel

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
_GOLD = {}


def _gpt(name):
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**GC.case_kwargs(name))
    P = GC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    conds, forced = GC.make_inputs(name)
    return m.cuda(), P, conds.cuda(), forced.cuda()


def _gpt_golds(name, P, conds, forced):
    """(fp64 logits of the quantized model, of the unquantized one), computed once per case on the device"""
    if name not in _GOLD:
        on = lambda D: {k: v.cuda() for k, v in D.items()}
        _GOLD[name] = (GC.step_logits(on(quantized_params(P)), name, conds, forced, work=torch.float64).cpu(),
                       GC.step_logits(on(P), name, conds, forced, work=torch.float64).cpu())
    return _GOLD[name]


def _held_to_the_rule(got, emu, gold, dt, steps, what):
    worst = 0.0
    for sl in steps + [tuple(slice(None) for _ in range(gold.dim() - 1))]:
        ek, ee, fl = rel(got[sl], gold[sl]), rel(emu[sl], gold[sl]), floor16(gold[sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        assert ek <= 2 * ee + fl, (what, sl, ek, ee, fl)
    print(f"{what}: whole-sequence error {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}; worst kernel / (2 emulation + floor) over the steps {worst:.3f}")
    return worst


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(GC.CASES))
def test_fp6_weights_against_the_dequantized_model(name, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = H16[fmt]
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    gold_q, gold = _gpt_golds(name, P, conds, forced)
    logits, codes = m.sample(conds, forced_codes=forced, seed=1, weights="fp6")
    assert tuple(logits.shape) == (B, T * V) and tuple(codes.shape) == (B, T)
    got = logits.view(B, T, V).cpu()
    Q = {k: v.cuda() for k, v in quantized_params(P).items()}
    emu = GC.step_logits(Q, name, conds, forced, rnd=lambda t: t.to(dt).to(torch.float32), prod=torch.float64).cpu()
    _held_to_the_rule(got, emu, gold_q, dt, [(slice(None), slice(t, t + 1)) for t in range(T)], f"fp6 weights, {fmt} {name}")
    # the weights really are the quantized ones: the fp6 path is the closer one to the quantized model, the 16-bit path to the unquantized one
    h16 = m.sample(conds, forced_codes=forced, seed=1, weights="h16")[0].view(B, T, V).cpu()
    a, b, c, d = rel(got, gold_q), rel(h16, gold_q), rel(h16, gold), rel(got, gold)
    print(f"{fmt} {name}: fp6 path vs quantized model {a:.3e}, 16-bit path vs quantized model {b:.3e}; 16-bit vs unquantized {c:.3e}, fp6 vs unquantized {d:.3e}")
    assert a < b and c < d, (a, b, c, d)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_rq_fp6_weights_against_the_dequantized_model(fmt, monkeypatch):
    from enhancing.modules.stage2.layers import RQTransformer
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt, name = H16[fmt], "rq_d3"
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    m = RQTransformer(**SC.case_kwargs(name))
    P = SC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    m.cuda()
    conds, forced = (t.cuda() for t in SC.case_inputs(name))
    Q = {k: v.cuda() for k, v in quantized_params(P).items()}
    assert sum(not torch.equal(Q[k].cpu(), P[k]) for k in P) == 6 * (Ls + Ld) and torch.equal(Q["head.weight"].cpu(), P["head.weight"])
    gold_q = SC.step_logits(Q, name, conds, forced, "once", work=torch.float64).view(B, T, D, V).cpu()
    emu = SC.step_logits(Q, name, conds, forced, "once", rnd=lambda t: t.to(dt).to(torch.float32), prod=torch.float64).view(B, T, D, V).cpu()
    logits, codes = m.sample(conds, forced_codes=forced, seed=1, slot0_ln="once", weights="fp6")
    assert tuple(logits.shape) == (B * T, D, V) and tuple(codes.shape) == (B, T, D)
    got = logits.view(B, T, D, V).cpu()
    _held_to_the_rule(got, emu, gold_q, dt, [(slice(None), t, d) for t in range(T) for d in range(D)], f"fp6 weights, {fmt} {name}")
    h16 = m.sample(conds, forced_codes=forced, seed=1, slot0_ln="once")[0].view(B, T, D, V).cpu()
    assert rel(got, gold_q) < rel(h16, gold_q)
    lg, cg = m.sample(conds, forced_codes=forced, seed=1, slot0_ln="once", weights="fp6", graph=True)
    assert torch.equal(lg.view(torch.int32), logits.view(torch.int32)) and torch.equal(cg, codes)


def _bits(t):
    return t.view(torch.int32)


def test_graph_replay_equals_the_loop():
    m, P, conds, forced = _gpt("tiny")
    for kw in (dict(forced_codes=forced), dict(top_k=50, top_p=0.9)):
        l0, c0 = m.sample(conds, seed=4, weights="fp6", graph=False, **kw)
        l1, c1 = m.sample(conds, seed=4, weights="fp6", graph=True, **kw)
        assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(c0, c1)


def test_composes_with_the_fp8_cache():
    """weights="fp6" with cache="fp8": the loop and the graph agree bit for bit, and the cache form is really in use (the logits differ from the
    16-bit cache's)"""
    m, P, conds, forced = _gpt("tiny")
    l0, c0 = m.sample(conds, forced_codes=forced, seed=4, weights="fp6", cache="fp8", graph=False)
    l1, c1 = m.sample(conds, forced_codes=forced, seed=4, weights="fp6", cache="fp8", graph=True)
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(c0, c1)
    l2, _ = m.sample(conds, forced_codes=forced, seed=4, weights="fp6", cache="h16")
    assert not torch.equal(_bits(l0), _bits(l2)) and bool(torch.isfinite(l0).all())


def test_seed_and_chunks(monkeypatch):
    from enhancing.modules.stage2.layers import GPT
    torch.manual_seed(0)
    m = GPT(vocab_cond_size=10, vocab_img_size=256, embed_dim=128, cond_num_tokens=1, img_num_tokens=5, n_heads=2, n_layers=1).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(6.0)
    conds = (torch.arange(70) % 10).view(70, 1).cuda()
    kw = dict(top_k=40, top_p=0.95, softmax_temperature=0.9, weights="fp6")
    l1, c1 = m.sample(conds, seed=5, **kw)
    l2, c2 = m.sample(conds, seed=5, **kw)
    assert torch.equal(c1, c2) and torch.equal(_bits(l1), _bits(l2))
    assert not torch.equal(c1, m.sample(conds, seed=6, **kw)[1])
    la, ca = m.sample(conds[:64], seed=5, **kw)
    lb, cb = m.sample(conds[64:], seed=5, row_offset=64, **kw)
    assert torch.equal(c1, torch.cat([ca, cb])) and torch.equal(_bits(l1), _bits(torch.cat([la, lb])))
    # the environment is the default of the keyword
    monkeypatch.setenv("ENH_SAMPLE_WEIGHTS", "fp6")
    l3, c3 = m.sample(conds, seed=5, top_k=40, top_p=0.95, softmax_temperature=0.9)
    assert torch.equal(_bits(l3), _bits(l1)) and torch.equal(c3, c1)
    monkeypatch.setenv("ENH_SAMPLE_WEIGHTS", "fp8")
    l4, _ = m.sample(conds, seed=5, top_k=40, top_p=0.95, softmax_temperature=0.9)
    assert not torch.equal(_bits(l4), _bits(l1))


def test_building_the_fp6_operands_builds_no_other_block_copy():
    from enhancing.modules.stage2.prior import MXFP6
    m, P, conds, forced = _gpt("tiny")
    dt = m._operand_dtype(True, "test")
    m.sample(conds, forced_codes=forced, seed=1, weights="fp6")
    assert list(m._operands) == [("fp6", dt)]
    ops = m._operands[("fp6", dt)][1]
    C = GC.CASES["tiny"][0]
    shapes = dict(wqkv=(3 * C, C), wproj=(C, C), w0=(4 * C, C), w1=(C, 4 * C))
    for W in ops["layers"]:
        for k, (N, K) in shapes.items():
            assert isinstance(W[k], MXFP6)
            codes, scales = W[k]
            assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and tuple(codes.shape) == (N, row_bytes(K)) and tuple(scales.shape) == (N, K // 32)
            assert codes.numel() * codes.element_size() + scales.numel() * scales.element_size() == N * row_bytes(K) + N * K // 32
        # nothing else of a layer is a matrix: no 16-bit, fp8 or fp4 copy of a Block weight
        assert all(v is None or v.dim() == 1 for k, v in W.items() if k not in shapes), {k: type(v) for k, v in W.items()}
    assert ops["head"].dtype == dt and set(ops) == {"layers", "head"}


def test_load_state_dict_rebuilds_the_fp6_operands():
    from enhancing.modules.stage2.layers import GPT
    m, P, conds, forced = _gpt("tiny")
    la, _ = m.sample(conds, forced_codes=forced, seed=1, weights="fp6")
    P2 = GC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=GC.PARAM_SEED + 1)
    m.load_state_dict(P2)
    lb, _ = m.sample(conds, forced_codes=forced, seed=1, weights="fp6")
    fresh = GPT(**GC.case_kwargs("tiny"))
    fresh.load_state_dict(P2)
    lf, _ = fresh.cuda().sample(conds, forced_codes=forced, seed=1, weights="fp6")
    assert torch.equal(_bits(lb), _bits(lf)) and not torch.equal(_bits(lb), _bits(la))


def _cond_transformer():
    """the tiny CondTransformer of tests/test_gpt_train_gpu.py"""
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


def test_a_sample_after_an_optimizer_step_sees_the_stepped_weights():
    from enhancing.modules.stage2.layers import GPT
    ct = _cond_transformer()
    ct.learning_rate = 1e-2
    ct.transformer.cuda()
    (opt,), _ = ct.configure_optimizers()
    gpt = ct.transformer
    conds = torch.tensor([[0], [2], [1]]).cuda()
    before, _ = gpt.sample(conds, seed=2, weights="fp6")
    g = torch.Generator().manual_seed(1)
    ct.training_step({"image": torch.rand(3, 3, 32, 32, generator=g).cuda(), "class": torch.randint(0, 3, (3,), generator=g).cuda()}, 0)
    opt.step()
    after, codes = gpt.sample(conds, seed=2, weights="fp6")
    fresh = GPT(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, n_heads=2, n_layers=1)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in gpt.state_dict().items()})
    want, want_codes = fresh.cuda().sample(conds, seed=2, weights="fp6")
    assert torch.equal(_bits(after), _bits(want)) and torch.equal(codes, want_codes)
    assert not torch.equal(_bits(after), _bits(before)), "the step changed nothing: the test shows nothing"
    # images through CondTransformer.sample, which passes the keyword on
    img = ct.sample(conds[:, 0], top_k=20, seed=3, weights="fp6")
    assert tuple(img.shape) == (3, 3, 32, 32)


def test_value_errors(monkeypatch):
    m, P, conds, forced = _gpt("tiny")
    with pytest.raises(ValueError, match="use_fp16"):
        m.sample(conds, use_fp16=False, weights="fp6")
    with pytest.raises(ValueError, match="int6"):
        m.sample(conds, weights="int6")
    monkeypatch.setenv("ENH_SAMPLE_WEIGHTS", "nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        m.sample(conds)
