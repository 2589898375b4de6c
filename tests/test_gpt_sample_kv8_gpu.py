"""GPT.sample(cache="fp8"): the MXFP8 k / v cache against the model it claims to run, which is the cached sampling loop with every step's k and v
rows replaced by their MXFP8 form before they enter the cache AND the step's own attention (tests/kv8_cases.py).  The yardstick is the project's
16-bit rule (tests/test_gpt_sample_gpu.py) against THAT model: with truth its fp64 logits and emu the same loop with every operand and cache
entry rounded to the format and fp64 products, rel(got, truth) <= 2 rel(emu, truth) + floor16(truth), over the whole tensor and over every slice
of 32 positions.  In plain torch on the CPU the emulation's own distance to the truth is 1.8 - 2.4e-3 (fp16) and 7.5 - 8.8e-3 (bf16) (a 16-bit
ulp of a k / v entry can move its e4m3 code), and an f32-product restatement sits at 0.45 - 0.48 of the limit.

Device / limit, measured on MI355X (every run prints them), fp16 / bf16: tiny 0.473 / 0.451, hs384 0.479 / 0.453, h3 0.479 / 0.457;
with weights="fp8" as well: tiny 0.483 / 0.448.
What the format costs (recorded, not gated): the fp64 truth with the hook against the fp64 loop without it is 0.93 - 1.2e-2 relative on these
random Gaussian models, below the 3.6 - 4.9e-2 of MXFP8 weights; nobody has measured it on trained weights."""
import os
import sys

import pytest
import torch

import gpt_cases as GC
import kv8_cases as KC
from mxfp8_util import quantized_params
from util import floor16, rel

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TRUTH = {}


def _gpt(name):
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**GC.case_kwargs(name))
    P = GC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    conds, forced = GC.make_inputs(name)
    return m.cuda(), P, conds.cuda(), forced.cuda()


def _truth(name, P, conds, forced, w8=False):
    """(fp64 logits of the loop with the kv8 hook, without it), computed once per case and weight form, on the CPU; w8: the Block weights are their
    MXFP8 form (mxfp8_util.quantized_params)"""
    if (name, w8) not in _TRUTH:
        Q = quantized_params(P) if w8 else P
        _TRUTH[name, w8] = (KC.step_logits(Q, name, conds.cpu(), forced.cpu(), work=torch.float64, kv=KC.kv8),
                            GC.step_logits(Q, name, conds.cpu(), forced.cpu(), work=torch.float64))
    return _TRUTH[name, w8]


def _emulation(name, P, conds, forced, dt, w8=False):
    Q = quantized_params(P) if w8 else P
    return KC.step_logits(Q, name, conds.cpu(), forced.cpu(), rnd=lambda t: t.to(dt).to(torch.float32), prod=torch.float64, kv=KC.kv8)


def _held_to_the_rule(got, emu, truth, dt, what):
    """the whole tensor and every slice of 32 positions; prints device / limit"""
    T = truth.shape[1]
    worst = 0.0
    for sl in [slice(None)] + [slice(t0, t0 + 32) for t0 in range(0, T, 32)]:
        ek, ee, fl = rel(got[:, sl], truth[:, sl]), rel(emu[:, sl], truth[:, sl]), floor16(truth[:, sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        print(f"{what} positions {sl.start or 0}..: device {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}, device / (2 emulation + floor) {ek / (2 * ee + fl):.3f}")
        assert ek <= 2 * ee + fl, (what, sl, ek, ee, fl)
    return worst


def _bits(t):
    return t.view(torch.int32)


def test_the_default_path_is_the_16_bit_cache(monkeypatch):
    monkeypatch.delenv("ENH_SAMPLE_CACHE", raising=False)
    m, P, conds, forced = _gpt("tiny")
    C, H, L, V, T, B = GC.CASES["tiny"]
    l0, c0 = m.sample(conds, forced_codes=forced, seed=1)
    l1, c1 = m.sample(conds, forced_codes=forced, seed=1, cache=None)
    l2, c2 = m.sample(conds, forced_codes=forced, seed=1, cache="h16")
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(l0), _bits(l2)) and torch.equal(c0, c1) and torch.equal(c0, c2)
    dt = m._operand_dtype(True, "test")
    for st in (m._decode_state(B, dt, "cuda"), m._decode_state(B, dt, "cuda", cache="h16")):
        assert len(st["caches"]) == L
        for kv in st["caches"]:
            assert len(kv) == 2 and all(z.dtype == dt and tuple(z.shape) == (B, H, T, C // H) for z in kv)
    st = m._decode_state(B, dt, "cuda", cache="fp8")
    assert len(st["caches"]) == L
    for kv in st["caches"]:
        assert [tuple(z.shape) for z in kv] == [(B, H, T, C // H), (B, H, T, C // H // 32)] * 2 and all(z.dtype == torch.uint8 for z in kv)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(GC.CASES))
def test_fp8_cache_against_the_quantized_cache_model(name, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = H16[fmt]
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    truth, plain = _truth(name, P, conds, forced)
    logits, codes = m.sample(conds, forced_codes=forced, seed=1, cache="fp8")
    assert tuple(logits.shape) == (B, T * V) and tuple(codes.shape) == (B, T)
    got = logits.view(B, T, V).cpu()
    emu = _emulation(name, P, conds, forced, dt)
    worst = _held_to_the_rule(got, emu, truth, dt, f"fp8 cache, {fmt} {name}")
    # the cache really is the quantized one: the fp8 path is the closer one to the quantized-cache model, the 16-bit path to the plain one (checked
    # under fp16, where the format's own rounding, 5e-4, is far below what the cache format costs, 1e-2: not a close call)
    h16 = m.sample(conds, forced_codes=forced, seed=1, cache="h16")[0].view(B, T, V).cpu()
    a, b, c, d = rel(got, truth), rel(h16, truth), rel(h16, plain), rel(got, plain)
    print(f"{fmt} {name}: device / limit {worst:.3f}; what the format costs (fp64 with the hook against fp64 without) {rel(truth, plain):.3e}; "
          f"fp8 path vs its model {a:.3e}, 16-bit path vs that model {b:.3e}; 16-bit path vs the plain model {c:.3e}, fp8 path vs the plain model {d:.3e}")
    if dt == torch.float16:
        assert a < b and c < d, (a, b, c, d)
    # graph replay: the same bits, logits and codes
    lg, cg = m.sample(conds, forced_codes=forced, seed=1, cache="fp8", graph=True)
    assert torch.equal(_bits(lg), _bits(logits)) and torch.equal(cg, codes)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_fp8_weights_and_fp8_cache_together(fmt, monkeypatch):
    """weights="fp8", cache="fp8": loop and graph run, agree bit for bit and meet the rule against the model whose Block weights AND cache entries
    are the quantized ones"""
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt, name = H16[fmt], "tiny"
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    truth, _ = _truth(name, P, conds, forced, w8=True)
    emu = _emulation(name, P, conds, forced, dt, w8=True)
    logits, codes = m.sample(conds, forced_codes=forced, seed=1, weights="fp8", cache="fp8")
    _held_to_the_rule(logits.view(B, T, V).cpu(), emu, truth, dt, f"fp8 weights + fp8 cache, {fmt} {name}")
    lg, cg = m.sample(conds, forced_codes=forced, seed=1, weights="fp8", cache="fp8", graph=True)
    assert torch.equal(_bits(lg), _bits(logits)) and torch.equal(cg, codes)
    assert not torch.equal(_bits(logits), _bits(m.sample(conds, forced_codes=forced, seed=1, cache="fp8")[0]))


def test_graph_replay_equals_the_loop_when_codes_are_drawn():
    m, P, conds, forced = _gpt("tiny")
    l0, c0 = m.sample(conds, seed=4, cache="fp8", graph=False, top_k=50, top_p=0.9)
    l1, c1 = m.sample(conds, seed=4, cache="fp8", graph=True, top_k=50, top_p=0.9)
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(c0, c1)


def test_seed_and_chunks(monkeypatch):
    from enhancing.modules.stage2.layers import GPT
    torch.manual_seed(0)
    m = GPT(vocab_cond_size=10, vocab_img_size=256, embed_dim=128, cond_num_tokens=1, img_num_tokens=5, n_heads=2, n_layers=1).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(6.0)      # logits of scale ~1 instead of the init's ~0.2
    conds = (torch.arange(66) % 10).view(66, 1).cuda()
    kw = dict(top_k=40, top_p=0.95, softmax_temperature=0.9)
    l1, c1 = m.sample(conds, seed=5, cache="fp8", **kw)
    l2, c2 = m.sample(conds, seed=5, cache="fp8", **kw)
    assert torch.equal(c1, c2) and torch.equal(_bits(l1), _bits(l2))
    assert not torch.equal(c1, m.sample(conds, seed=6, cache="fp8", **kw)[1])
    la, ca = m.sample(conds[:64], seed=5, cache="fp8", **kw)
    lb, cb = m.sample(conds[64:], seed=5, row_offset=64, cache="fp8", **kw)
    assert torch.equal(c1, torch.cat([ca, cb])) and torch.equal(_bits(l1), _bits(torch.cat([la, lb])))
    # the environment is the default of the keyword
    monkeypatch.setenv("ENH_SAMPLE_CACHE", "fp8")
    l3, c3 = m.sample(conds, seed=5, **kw)
    assert torch.equal(_bits(l3), _bits(l1)) and torch.equal(c3, c1)
    monkeypatch.setenv("ENH_SAMPLE_CACHE", "h16")
    assert not torch.equal(_bits(m.sample(conds, seed=5, **kw)[0]), _bits(l1))


def test_value_errors(monkeypatch):
    m, P, conds, forced = _gpt("tiny")
    with pytest.raises(ValueError, match="use_fp16"):
        m.sample(conds, use_fp16=False, cache="fp8")
    with pytest.raises(ValueError, match="int4"):
        m.sample(conds, cache="int4")
    monkeypatch.setenv("ENH_SAMPLE_CACHE", "nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        m.sample(conds)


def _tiny_cfg():
    """the tiny CondTransformer of tests/test_gpt_train_gpu.py, as constructor arguments"""
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    return dict(cond_key="class", code_shape=[16],
                cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
                stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                            params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=dict(tower), quantizer=dict(embed_dim=32, n_embed=64),
                                        loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
                transformer=dict(target="enhancing.modules.stage2.layers.GPT",
                                 params=dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, n_heads=2, n_layers=1)))


def test_cond_transformer_and_the_image_tool_pass_the_keyword_on(tmp_path, capsys):
    import yaml
    from PIL import Image
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    torch.manual_seed(0)
    cfg = AttrDict.wrap(_tiny_cfg())
    ct = CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer, code_shape=[16])
    conds = torch.tensor([0, 2, 1]).cuda()
    img = ct.sample(conds, top_k=20, seed=3, cache="fp8")
    assert tuple(img.shape) == (3, 3, 32, 32) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    fp8_codes = ct.last_codes.clone()
    _, want = ct.transformer.sample(conds.view(3, 1), top_k=20, seed=3, return_logits=False, cache="fp8")
    assert torch.equal(fp8_codes.view(3, 16), want)
    with pytest.raises(ValueError, match="int4"):
        ct.sample(conds, cache="int4")
    # tools/sample_images.py --cache fp8 writes an image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sample_images
    path, out = tmp_path / "tiny.yaml", tmp_path / "samples.png"
    path.write_text(yaml.safe_dump(dict(model=dict(target="enhancing.modules.stage2.transformer.CondTransformer", params=_tiny_cfg()))))
    torch.manual_seed(0)
    sample_images.main(["-c", str(path), "--classes", "0", "2", "--top_k", "20", "--seed", "1", "--nrow", "2", "--cache", "fp8", "--out", str(out)])
    assert "2 images (3, 32, 32)" in capsys.readouterr().out
    assert Image.open(out).size[0] >= 64
    with pytest.raises(SystemExit):
        sample_images.main(["-c", str(path), "--classes", "0", "--cache", "int4", "--out", str(out)])
