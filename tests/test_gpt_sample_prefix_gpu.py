"""GPT.sample(prefix_codes=): the batched prefill of given codes against the model it must reproduce, which is the SAMPLER's (the cached loop under
forced codes: tests/golden/gpt_<case>.npz holds its fp64 logits), not the teacher-forced one.  Every check is on the positions t >= P; the logits
of the given positions are NaN and codes[:, :P] is the prefix.

Exact mode: the constant and the rule of tests/test_gpt_sample_gpu.py (EXACT_RATIO x the fp32 reference's own error + 1e-6).
16-bit modes: that file's rule, rel(got, gold) <= 2 rel(emu, gold) + floor16, per step t >= P and over those steps together, with
emu = prefix_cases.prefix_step_logits(n_prefix = P, rnd = the format): the loop's emulation with the tile attention's rounding of the softmax
numerators in the prefilled steps.  `long` (a prefix of 150 rows: a 128-query block boundary and a ragged third 64-key tile) has no golden; its
gold is the same function in fp64 on the device.  With cache="fp8" the model is the one whose slots hold the MXFP8 form of the rows
(kv8_cases.kv8), with weights="fp8" | "fp6" | "fp4" the one whose Block weights are the dequantized operands.

Measured on MI355X (every test prints its figure).  Exact mode, error / fp32 reference's error, worst over P in {1, T // 2, T - 1}:
tiny 0.687, hs384 0.712, h3 0.739 (the call without a prefix: 0.687 / 0.737 / 0.665; the constant is 1.5).  16-bit modes, worst kernel /
(2 emulation + floor) over the steps: 0.405 - 0.451 on the three cases, long 0.495 (fp16) / 0.464 (bf16), cache="fp8" 0.434 - 0.484,
MX weights 0.397 - 0.440."""
import os
import sys

import numpy as np
import pytest
import torch

import gpt_cases as GC
import kv8_cases as KC
import mxfp4_util
import mxfp6_util
import mxfp8_util
import prefix_cases as PC
from test_gpt_sample_gpu import EXACT_RATIO
from util import floor16, rel

pytestmark = pytest.mark.gpu
H16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
QUANTIZED = {"fp8": mxfp8_util.quantized_params, "fp6": mxfp6_util.quantized_params, "fp4": mxfp4_util.quantized_params}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLD = {}


def _prefixes(name):
    T = PC.CASES[name][4]
    return [PC.LONG_PREFIX] if name == "long" else [1, T // 2, T - 1]


CASE_P = [(name, P) for name in GC.CASES for P in _prefixes(name)]


def _gpt(name):
    from enhancing.modules.stage2.layers import GPT
    m = GPT(**PC.case_kwargs(name))
    P = GC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    conds, forced = PC.case_inputs(name)
    return m.cuda(), P, conds.cuda(), forced.cuda()


def _on(D):
    return {k: v.cuda() for k, v in D.items()}


def _bits(t):
    return t.view(torch.int32)


def _rnd(dt):
    return lambda t: t.to(dt).to(torch.float32)


def _gold(key, make):
    """an fp64 statement of a model, computed once and left unchanged"""
    if key not in _GOLD:
        _GOLD[key] = make().cpu()
    return _GOLD[key]


def _prefix_contract(logits, codes, forced, n, B, T, V):
    """the logits of the given positions are NaN, every later one is a number, and the returned codes begin with the prefix"""
    lg = logits.view(B, T, V)
    assert bool(torch.isnan(lg[:, :n]).all()) and not bool(torch.isnan(lg[:, n:]).any())
    assert torch.equal(codes[:, :n], forced[:, :n]) and int(codes.min()) >= 0 and int(codes.max()) < V


def _held_to_the_rule(got, emu, gold, dt, n, what):
    """per step t >= n and over those steps together; prints and returns the worst device / limit"""
    T = gold.shape[1]
    worst = 0.0
    for sl in [slice(t, t + 1) for t in range(n, T)] + [slice(n, T)]:
        ek, ee, fl = rel(got[:, sl], gold[:, sl]), rel(emu[:, sl], gold[:, sl]), floor16(gold[:, sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        assert ek <= 2 * ee + fl, (what, sl, ek, ee, fl)
    print(f"{what}: steps {n}..{T - 1} error {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}; worst kernel / (2 emulation + floor) over the steps {worst:.3f}")
    return worst


@pytest.mark.parametrize("name, n", CASE_P)
def test_exact_mode_against_the_fp64_golden(golden_dir, name, n):
    """measured ratios (MI355X), P = 1 | T // 2 | T - 1: tiny 0.687 | 0.637 | 0.456, hs384 0.712 | 0.712 | 0.704, h3 0.665 | 0.739 | 0.501; the worst
    one is 0.739"""
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    g = np.load(os.path.join(golden_dir, f"gpt_{name}.npz"))
    assert torch.equal(torch.from_numpy(g["forced_codes"]).long(), forced.cpu()) and torch.equal(torch.from_numpy(g["conds"]), conds.cpu())
    logits, codes = m.sample(conds, use_fp16=False, forced_codes=forced, prefix_codes=forced[:, :n], seed=1)
    assert tuple(logits.shape) == (B, T * V) and tuple(codes.shape) == (B, T) and codes.dtype == torch.int64
    _prefix_contract(logits, codes, forced, n, B, T, V)
    err = (logits.view(B, T, V)[:, n:].cpu().double() - torch.from_numpy(g["logits64"])[:, n:]).abs().max().item()
    ref_err = float(g["ref32_err"])
    print(f"exact {name} P={n}: max err {err:.3e}, fp32 reference {ref_err:.3e}, ratio {err / ref_err:.3f}")
    assert err <= EXACT_RATIO * ref_err + 1e-6, (err, ref_err)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name, n", CASE_P)
def test_16_bit_modes_against_the_emulation(golden_dir, name, n, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = H16[fmt]
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    gold = torch.from_numpy(np.load(os.path.join(golden_dir, f"gpt_{name}.npz"))["logits64"])
    logits, codes = m.sample(conds, forced_codes=forced, prefix_codes=forced[:, :n], seed=1)
    _prefix_contract(logits, codes, forced, n, B, T, V)
    emu = PC.prefix_step_logits(_on(P), name, conds, forced, n, rnd=_rnd(dt), prod=torch.float64).cpu()
    _held_to_the_rule(logits.view(B, T, V).cpu(), emu, gold, dt, n, f"{fmt} {name} P={n}")


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_the_long_prefix_against_the_emulation(fmt, monkeypatch):
    """a prefix of 150 rows: more than one query block and a ragged last key tile in the prefill's attention, the decode attention's split plan behind it"""
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt, name, n = H16[fmt], "long", PC.LONG_PREFIX
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = PC.CASES[name]
    gold = _gold(name, lambda: PC.prefix_step_logits(_on(P), name, conds, forced, n, rnd=None, prod=torch.float64, work=torch.float64))
    logits, codes = m.sample(conds, forced_codes=forced, prefix_codes=forced[:, :n], seed=1)
    _prefix_contract(logits, codes, forced, n, B, T, V)
    emu = PC.prefix_step_logits(_on(P), name, conds, forced, n, rnd=_rnd(dt), prod=torch.float64).cpu()
    _held_to_the_rule(logits.view(B, T, V).cpu(), emu, gold, dt, n, f"{fmt} {name} P={n}")
    # the prefill is what the forced loop computes up to the roundings the rule allows: the two paths are close, and not the same launches
    loop = m.sample(conds, forced_codes=forced, seed=1)[0].view(B, T, V)[:, n:]
    print(f"{fmt} long: prefill against the forced loop on the same codes {rel(logits.view(B, T, V)[:, n:], loop):.3e}")


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("n", _prefixes("tiny"))
def test_fp8_cache_against_the_quantized_cache_model(n, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt, name = H16[fmt], "tiny"
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    truth = _gold("tiny kv8", lambda: PC.prefix_step_logits(P, name, conds.cpu(), forced.cpu(), 0, work=torch.float64, kv=KC.kv8))
    logits, codes = m.sample(conds, forced_codes=forced, prefix_codes=forced[:, :n], seed=1, cache="fp8")
    _prefix_contract(logits, codes, forced, n, B, T, V)
    emu = PC.prefix_step_logits(P, name, conds.cpu(), forced.cpu(), n, rnd=_rnd(dt), prod=torch.float64, kv=KC.kv8)
    _held_to_the_rule(logits.view(B, T, V).cpu(), emu, truth, dt, n, f"fp8 cache, {fmt} {name} P={n}")


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("n", _prefixes("tiny"))
@pytest.mark.parametrize("weights", list(QUANTIZED))
def test_mx_weights_against_the_dequantized_model(weights, n, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt, name = H16[fmt], "tiny"
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    Q = _on(QUANTIZED[weights](P))
    gold_q = _gold(("tiny", weights), lambda: GC.step_logits(Q, name, conds, forced, work=torch.float64))
    logits, codes = m.sample(conds, forced_codes=forced, prefix_codes=forced[:, :n], seed=1, weights=weights)
    _prefix_contract(logits, codes, forced, n, B, T, V)
    emu = PC.prefix_step_logits(Q, name, conds, forced, n, rnd=_rnd(dt), prod=torch.float64).cpu()
    _held_to_the_rule(logits.view(B, T, V).cpu(), emu, gold_q, dt, n, f"{weights} weights, {fmt} {name} P={n}")
    assert dt not in m._operands and (weights, dt) in m._operands, "the prefill built 16-bit copies of the Block weights"


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------
KW = dict(top_k=40, top_p=0.95, softmax_temperature=0.9)


def _scaled_model(T=5):
    from enhancing.modules.stage2.layers import GPT
    torch.manual_seed(0)
    m = GPT(vocab_cond_size=10, vocab_img_size=256, embed_dim=128, cond_num_tokens=1, img_num_tokens=T, n_heads=2, n_layers=2).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(6.0)      # logits of scale ~1 instead of the init's ~0.2
    return m


def test_no_prefix_and_an_empty_prefix_are_the_call_without_the_keyword(monkeypatch):
    from enhancing import _C
    m = _scaled_model()
    conds = (torch.arange(6) % 10).view(6, 1).cuda()
    l0, c0 = m.sample(conds, seed=5, **KW)
    new = []
    for fn in ("kv_cache_fill", "kv_cache_fill_kv8", "causal_attention", "gpt_embed_seq", "ln_timeshift", "gemm"):
        monkeypatch.setattr(_C, fn, lambda *a, _fn=fn, **k: new.append(_fn))
    for prefix in (None, torch.empty(6, 0, dtype=torch.int64), torch.empty(6, 0, dtype=torch.int64).cuda()):
        l1, c1 = m.sample(conds, seed=5, prefix_codes=prefix, **KW)
        assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(c0, c1)
    assert not new, f"a call without given codes ran launches of the prefill: {new}"


def test_a_seed_gives_the_same_bits_twice_and_the_draws_of_a_full_run():
    m = _scaled_model(T=9)
    conds = (torch.arange(6) % 10).view(6, 1).cuda()
    _, full = m.sample(conds, seed=5, **KW)
    l1, c1 = m.sample(conds, seed=5, prefix_codes=full[:, :4], **KW)
    l2, c2 = m.sample(conds, seed=5, prefix_codes=full[:, :4].cpu(), **KW)
    assert torch.equal(_bits(l1), _bits(l2)) and torch.equal(c1, c2) and torch.equal(c1[:, :4], full[:, :4])
    assert not torch.equal(c1, m.sample(conds, seed=6, prefix_codes=full[:, :4], **KW)[1])
    # positions >= P keep their step numbers, so their uniforms.  Under forced codes (no draw feeds a later step) the continued run and the full
    # run draw from logits that differ by the prefill's roundings, ~1e-3 relative, with the SAME uniform: a draw differs only where its uniform
    # lies that close to a boundary of the CDF.  With the uniforms of other steps the draws would be independent and agree at a rate of
    # sum p^2 over 40 kept entries: far below a half.  So: at least half of the 30 draws agree (in practice all of them).
    _, cf = m.sample(conds, seed=5, forced_codes=full, **KW)
    _, cp = m.sample(conds, seed=5, forced_codes=full, prefix_codes=full[:, :4], **KW)
    same = (cp[:, 4:] == cf[:, 4:]).float().mean().item()
    print(f"draws of the continued run equal to the full run's under the same forced codes: {same:.3f}")
    assert same >= 0.5
    # forcing the continued run's codes reproduces its logits: the drawn codes are what is fed forward
    lf, _ = m.sample(conds, seed=9, prefix_codes=c1[:, :4], forced_codes=c1, **KW)
    assert torch.equal(_bits(lf), _bits(l1))


@pytest.mark.parametrize("kw", [dict(), dict(cache="fp8", weights="fp4")], ids=["h16", "fp8cache_fp4weights"])
def test_graph_replay_equals_the_loop_with_a_prefix(kw):
    name, n = "tiny", 7
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    for more in (dict(forced_codes=forced), dict(top_k=50, top_p=0.9)):
        l0, c0 = m.sample(conds, seed=4, prefix_codes=forced[:, :n], graph=False, **kw, **more)
        l1, c1 = m.sample(conds, seed=4, prefix_codes=forced[:, :n], graph=True, **kw, **more)
        assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(c0, c1)
        _prefix_contract(l1, c1, forced, n, B, T, V)
    lt, ct = m.sample(conds, seed=4, prefix_codes=forced[:, :T - 1], graph=True, **kw)      # nothing is left to replay
    l2, c2 = m.sample(conds, seed=4, prefix_codes=forced[:, :T - 1], graph=False, **kw)
    assert torch.equal(_bits(lt), _bits(l2)) and torch.equal(ct, c2)


@pytest.mark.parametrize("kw", [dict(), dict(cache="fp8")], ids=["h16", "fp8cache"])
def test_chunks_equal_separate_calls_with_a_prefix(kw):
    m = _scaled_model()
    conds = (torch.arange(70) % 10).view(70, 1).cuda()
    prefix = torch.randint(0, 256, (70, 2), generator=torch.Generator().manual_seed(2)).cuda()
    l1, c1 = m.sample(conds, seed=5, prefix_codes=prefix, **kw, **KW)
    la, ca = m.sample(conds[:64], seed=5, prefix_codes=prefix[:64], **kw, **KW)
    lb, cb = m.sample(conds[64:], seed=5, prefix_codes=prefix[64:], row_offset=64, **kw, **KW)
    assert torch.equal(c1, torch.cat([ca, cb])) and torch.equal(_bits(l1), _bits(torch.cat([la, lb])))
    assert torch.equal(c1[:, :2], prefix) and len(torch.unique(c1[:, 2:])) > 20
    # groups of whole sequences under the hidden-activation cap: the same bits whatever the group size
    m.forward_hidden_cap = 3 * 2 * 4 * 128 * 6      # three sequences of two rows per group
    l2, c2 = m.sample(conds, seed=5, prefix_codes=prefix, **kw, **KW)
    assert torch.equal(c1, c2) and torch.equal(_bits(l1), _bits(l2))


def test_the_given_codes_reach_the_caches():
    """two prefixes that differ in one code give different logits at t = P, wherever the code sits (the first one is seen only through the caches)"""
    name, n = "tiny", 7
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    l0, _ = m.sample(conds, seed=1, prefix_codes=forced[:, :n])
    for pos in (0, n - 1):
        other = forced[:, :n].clone()
        other[:, pos] = (other[:, pos] + 1) % V
        l1, c1 = m.sample(conds, seed=1, prefix_codes=other)
        a, b = l0.view(B, T, V)[:, n], l1.view(B, T, V)[:, n]
        assert rel(a, b) > 1e-3, (pos, rel(a, b))
        assert torch.equal(c1[:, :n], other)


def test_refusals():
    name = "tiny"
    m, P, conds, forced = _gpt(name)
    C, H, L, V, T, B = GC.CASES[name]
    with pytest.raises(ValueError, match="left to draw"):
        m.sample(conds, prefix_codes=forced)      # P = T
    for bad in (forced[:, :3] + V, forced[:, :3] - V):
        with pytest.raises(ValueError, match="prefix_codes outside"):
            m.sample(conds, prefix_codes=bad)
    with pytest.raises(ValueError, match="one row per row"):
        m.sample(conds, prefix_codes=forced[:1, :3])
    other = forced.clone()
    other[-1, 2] = (other[-1, 2] + 1) % V
    with pytest.raises(ValueError, match="disagree"):
        m.sample(conds, forced_codes=other, prefix_codes=forced[:, :3])
    m.sample(conds, forced_codes=other, prefix_codes=forced[:, :2])      # they agree in the first two positions
    with pytest.raises(ValueError, match="use_fp16"):
        m.sample(conds, use_fp16=False, cache="fp8", prefix_codes=forced[:, :3])      # the refusals that were there stay
    with pytest.raises(ValueError, match="int4"):
        m.sample(conds, cache="int4", prefix_codes=forced[:, :3])


# ---- the public surface -------------------------------------------------------------------------------------------------------------------
def _tiny_cfg():
    """the tiny CondTransformer of tests/test_gpt_sample_gpu.py: 32 x 32 images, 16 tokens"""
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    return dict(cond_key="class", code_shape=[4, 4],
                cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
                stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                            params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=dict(tower), quantizer=dict(embed_dim=32, n_embed=64),
                                        loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
                transformer=dict(target="enhancing.modules.stage2.layers.GPT",
                                 params=dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, n_heads=2, n_layers=1)))


def test_cond_transformer_continues_and_completes(tmp_path, capsys):
    import yaml
    from PIL import Image
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    torch.manual_seed(0)
    cfg = AttrDict.wrap(_tiny_cfg())
    ct = CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer, code_shape=[16])
    conds = torch.tensor([0, 2, 1]).cuda()
    codes = torch.randint(0, 64, (3, 16), generator=torch.Generator().manual_seed(1)).cuda()
    img = ct.sample(conds, prefix_codes=codes[:, :8].view(3, 2, 4), seed=3)
    assert tuple(img.shape) == (3, 3, 32, 32) and tuple(ct.last_codes.shape) == (3, 16)
    assert torch.equal(ct.last_codes[:, :8], codes[:, :8])
    _, want = ct.transformer.sample(conds.view(3, 1), prefix_codes=codes[:, :8], seed=3, return_logits=False)
    assert torch.equal(ct.last_codes, want)
    # complete: the kept rows are the tokenizer's codes of the images, the rest is drawn; under a [h, w] code_shape too
    images = torch.rand(3, 3, 32, 32, generator=torch.Generator().manual_seed(4)).cuda()
    tokens = ct.stage1_model.encode_codes(images).view(3, 16)
    for shape in ([16], [4, 4]):
        ct.code_shape = shape
        out = ct.complete(images, conds, keep=0.5, seed=3)
        assert tuple(out.shape) == (3, 3, 32, 32) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
        assert tuple(ct.last_codes.shape) == (3, *shape)
        last = ct.last_codes.view(3, 16)
        assert torch.equal(last[:, :8], tokens[:, :8])
        assert torch.equal(out, ct.stage1_model.decode_codes(ct.last_codes).clamp(0, 1))
        assert torch.equal(last, ct.transformer.sample(conds.view(3, 1), prefix_codes=tokens[:, :8], seed=3, return_logits=False)[1])
    ct.complete(images, conds, keep=0.1, seed=3)      # under one row of a 4 x 4 grid: nothing is kept, a plain sample
    assert torch.equal(ct.last_codes.view(3, 16), ct.transformer.sample(conds.view(3, 1), seed=3, return_logits=False)[1])
    with pytest.raises(ValueError, match="left to draw"):
        ct.complete(images, conds, keep=1.0)
    with pytest.raises(ValueError, match="keep"):
        ct.complete(images, conds, keep=-0.5)
    # tools/sample_images.py --complete: one row per image (the original, the kept part, a completion per class)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sample_images
    path, out_png = tmp_path / "tiny.yaml", tmp_path / "completed.png"
    path.write_text(yaml.safe_dump(dict(model=dict(target="enhancing.modules.stage2.transformer.CondTransformer", params=_tiny_cfg()))))
    files = []
    for i in range(2):
        files.append(str(tmp_path / f"in{i}.png"))
        Image.fromarray((images[i].permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)).save(files[-1])
    torch.manual_seed(0)
    sample_images.main(["-c", str(path), "--classes", "0", "2", "1", "--top_k", "20", "--seed", "1", "--complete", *files, "--keep", "0.5", "--out", str(out_png)])
    assert "2 images (3, 32, 32) completed for 3 classes, 2 of 4 token rows kept" in capsys.readouterr().out
    w, h = Image.open(out_png).size
    assert w >= 5 * 32 and h >= 2 * 32 and w > 2 * h
    with pytest.raises(SystemExit):
        sample_images.main(["-c", str(path), "--classes", "0", "--complete", files[0], "--keep", "1.0", "--out", str(out_png)])
