"""GPT.sample on the device against the reference's golden logits (tests/golden/gpt_<case>.npz: the reference's cached sample() in fp64, fed with forced
codes), in the exact mode and in both 16-bit modes, and the behaviour around it: seeds, chunked batches, CondTransformer, reloaded weights."""
import os

import numpy as np
import pytest
import torch

import gpt_cases as GC
from util import floor16, rel

pytestmark = pytest.mark.gpu

# Exact mode: max |logits - fp64 golden| <= EXACT_RATIO x (the fp32 reference module's own max error against the same golden) + 1e-6.
# Measured on MI355X: tiny 0.687, hs384 0.737, h3 0.665 (max errors 9.9e-7 / 7.6e-7 / 7.7e-7).  The constant is twice the worst ratio, the margin for
# summation-order differences across tile choices.  (With the exact GEMM's ascending-k sums in place of the tree-ordered enh_skinny_gemm_f32 the ratios
# were 1.77 / 4.05 / 2.13: the error of a sequential f32 sum over K = 3072.)
EXACT_RATIO = 1.5


def _case(golden_dir, name):
    from enhancing.modules.stage2.layers import GPT
    g = np.load(os.path.join(golden_dir, f"gpt_{name}.npz"))
    m = GPT(**GC.case_kwargs(name))
    P = GC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    C, H, L, V, T, B = GC.CASES[name]
    gold = torch.from_numpy(g["logits64"])
    return m.cuda(), P, torch.from_numpy(g["conds"]).cuda(), torch.from_numpy(g["forced_codes"]).long().cuda(), gold, g


@pytest.mark.parametrize("name", list(GC.CASES))
def test_exact_mode_against_the_fp64_golden(golden_dir, name):
    m, P, conds, forced, gold, g = _case(golden_dir, name)
    C, H, L, V, T, B = GC.CASES[name]
    logits, codes = m.sample(conds, use_fp16=False, forced_codes=forced, seed=1)
    assert tuple(logits.shape) == (B, T * V) and tuple(codes.shape) == (B, T) and codes.dtype == torch.int64
    assert int(codes.min()) >= 0 and int(codes.max()) < V
    err = (logits.view(B, T, V).cpu().double() - gold).abs()
    ref_err = float(g["ref32_err"])
    print(f"exact {name}: max err {err.max().item():.3e}, fp32 reference {ref_err:.3e}, ratio {err.max().item() / ref_err:.3f}")
    assert err.max().item() <= EXACT_RATIO * ref_err + 1e-6, (err.max().item(), ref_err)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(GC.CASES))
def test_16_bit_modes_against_the_emulation(golden_dir, name, fmt, monkeypatch):
    """yardstick: the same step in plain torch on the device with every GEMM operand and cache entry rounded to the format, products in fp64, the rest in f32.
    The kernel path may be at most twice as far from the golden as the emulation, plus the format's rounding floor: per step and over the sequence."""
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[fmt]
    m, P, conds, forced, gold, g = _case(golden_dir, name)
    C, H, L, V, T, B = GC.CASES[name]
    logits, _ = m.sample(conds, use_fp16=True, forced_codes=forced, seed=1)
    got = logits.view(B, T, V).cpu()
    emu = GC.step_logits({k: v.cuda() for k, v in P.items()}, name, conds, forced, rnd=lambda t: t.to(dt).to(torch.float32), prod=torch.float64).cpu()
    worst = 0.0
    for t in list(range(T)) + [None]:
        sl = slice(None) if t is None else slice(t, t + 1)
        ek, ee, fl = rel(got[:, sl], gold[:, sl]), rel(emu[:, sl], gold[:, sl]), floor16(gold[:, sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        assert ek <= 2 * ee + fl, (name, fmt, t, ek, ee, fl)
    print(f"{fmt} {name}: whole-sequence error {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}; worst kernel / (2 emulation + floor) over the steps {worst:.3f}")


def test_seed_gives_the_same_codes_and_chunks_equal_separate_calls(golden_dir):
    from enhancing.modules.stage2.layers import GPT
    torch.manual_seed(0)
    m = GPT(vocab_cond_size=10, vocab_img_size=256, embed_dim=128, cond_num_tokens=1, img_num_tokens=5, n_heads=2, n_layers=1).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(6.0)      # logits of scale ~1 instead of the init's ~0.2
    conds = (torch.arange(70) % 10).view(70, 1).cuda()
    kw = dict(top_k=40, top_p=0.95, softmax_temperature=0.9)
    l1, c1 = m.sample(conds, seed=5, **kw)
    l2, c2 = m.sample(conds, seed=5, **kw)
    assert torch.equal(c1, c2) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    _, c3 = m.sample(conds, seed=6, **kw)
    assert not torch.equal(c1, c3)
    # 70 rows = a chunk of 64 and one of 6: the same as two calls on those rows with the same seed and row numbers
    la, ca = m.sample(conds[:64], seed=5, **kw)
    lb, cb = m.sample(conds[64:], seed=5, row_offset=64, **kw)
    assert torch.equal(c1, torch.cat([ca, cb])) and torch.equal(l1.view(torch.int32), torch.cat([la, lb]).view(torch.int32))
    assert len(torch.unique(c1)) > 20
    _, cn = m.sample(conds[:2], return_logits=False)
    assert _ is None and tuple(cn.shape) == (2, 5)


def test_load_state_dict_refreshes_the_operand_copies(golden_dir):
    m, P, conds, forced, gold, g = _case(golden_dir, "tiny")
    la, _ = m.sample(conds, forced_codes=forced, seed=1)
    P2 = GC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=GC.PARAM_SEED + 1)
    m.load_state_dict(P2)
    lb, _ = m.sample(conds, forced_codes=forced, seed=1)
    assert rel(lb, la) > 0.5, "the second sample still ran the old weights"
    m.load_state_dict(P)
    lc, _ = m.sample(conds, forced_codes=forced, seed=1)
    assert torch.equal(lc.view(torch.int32), la.view(torch.int32))
    with torch.no_grad():
        m.head.weight.mul_(2.0)      # an in-place change of a master
    ld, _ = m.sample(conds, forced_codes=forced, seed=1)
    assert rel(ld, 2 * la) < 1e-3


def test_cond_transformer_samples_images():
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
    conds = torch.tensor([0, 2, 1]).cuda()
    img = ct.sample(conds, top_k=20, seed=3)
    assert tuple(img.shape) == (3, 3, 32, 32) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    assert tuple(ct.last_codes.shape) == (3, 16)
    assert torch.equal(img, ct.stage1_model.decode_codes(ct.last_codes).clamp(0, 1))
    with pytest.raises(NotImplementedError):
        ct.training_step({}, 0)
