"""GPT.forward on the device against the reference's golden logits (tests/golden/gpt_fwd_<case>.npz: the reference's GPT.forward in fp64), in the
exact mode and in both 16-bit modes, and the behaviour around it: the loss, chunked batches, reloaded weights, refusals, CondTransformer.

Exact mode: max |logits - fp64 golden| <= 4 x (the fp32 reference module's own max error against the same golden) + 1e-6: the reference's own
fp32 error is the yardstick, 4 x the project's margin for another summation order of the same arithmetic (tests/test_gpt_sample_cpu.py).  The
products run as enh_skinny_gemm_f32 in 64-row pieces (tree-ordered sums), not enh_gemm_f32, whose ascending-k sums DESIGN §3.5 recorded at
4.05 x the reference's error at K = 3072.  Measured on MI355X: tiny 0.421, hs384 0.368, h3 0.393, long 0.332, long3 0.388 (max errors 9.5e-7,
1.2e-6, 1.0e-6, 7.6e-7, 9.0e-7); 16-bit modes: kernel / (2 x emulation + floor) 0.41 - 0.45 over all cases and slices."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpt_forward_cases as FC
from util import floor16, rel

pytestmark = pytest.mark.gpu

EXACT_RATIO = 4.0
_EMU = {}


def _case(golden_dir, name):
    from enhancing.modules.stage2.layers import GPT
    g = np.load(os.path.join(golden_dir, f"gpt_fwd_{name}.npz"))
    m = GPT(**FC.case_kwargs(name))
    P = FC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    return m.cuda(), P, torch.from_numpy(g["conds"]).cuda(), torch.from_numpy(g["codes"]).long().cuda(), torch.from_numpy(g["logits64"]), g


@pytest.mark.parametrize("name", list(FC.CASES))
def test_exact_mode_against_the_fp64_golden(golden_dir, name):
    m, P, conds, codes, gold, g = _case(golden_dir, name)
    C, H, L, V, T, B = FC.CASES[name]
    logits = m(codes, conds, use_fp16=False)
    assert tuple(logits.shape) == (B, T, V) and logits.dtype == torch.float32 and not logits.requires_grad
    err = (logits.cpu().double() - gold).abs().max().item()
    ref_err = float(g["ref32_err"])
    print(f"exact {name}: max err {err:.3e}, fp32 reference {ref_err:.3e}, ratio {err / ref_err:.3f}")
    assert err <= EXACT_RATIO * ref_err + 1e-6, (err, ref_err)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(FC.CASES))
def test_16_bit_modes_against_the_emulation(golden_dir, name, fmt, monkeypatch):
    """yardstick: the same forward in plain torch on the device with every GEMM operand, q / k / v and the softmax numerators rounded to the format,
    products in fp64, the rest in f32.  The kernel path may be at most twice as far from the golden as the emulation, plus the format's rounding
    floor: over the whole tensor and over every slice of 32 positions (the rule of tests/test_gpt_sample_gpu.py)."""
    monkeypatch.setenv("ENH_PRECISION", fmt)
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[fmt]
    m, P, conds, codes, gold, g = _case(golden_dir, name)
    C, H, L, V, T, B = FC.CASES[name]
    got = m(codes, conds, use_fp16=True).cpu()
    if (name, fmt) not in _EMU:
        _EMU[(name, fmt)] = FC.forward_logits({k: v.cuda() for k, v in P.items()}, name, conds, codes, rnd=lambda t: t.to(dt).to(torch.float32),
                                              prod=torch.float64).cpu()
    emu = _EMU[(name, fmt)]
    worst = 0.0
    for sl in [slice(t, t + 32) for t in range(0, T, 32)] + [slice(None)]:
        ek, ee, fl = rel(got[:, sl], gold[:, sl]), rel(emu[:, sl], gold[:, sl]), floor16(gold[:, sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        assert ek <= 2 * ee + fl, (name, fmt, sl, ek, ee, fl)
    print(f"{fmt} {name}: whole-tensor error {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}; worst kernel / (2 emulation + floor) over the slices {worst:.3f}")


@pytest.mark.parametrize("use_fp16", [False, True])
def test_loss_is_the_cross_entropy_of_the_returned_logits(golden_dir, use_fp16):
    for name in ("tiny", "long3"):
        m, P, conds, codes, gold, g = _case(golden_dir, name)
        C, H, L, V, T, B = FC.CASES[name]
        logits, nll, mean = m(codes, conds, use_fp16=use_fp16, return_loss=True)
        assert tuple(nll.shape) == (B, T) and mean.dim() == 0
        ref = F.cross_entropy(logits.double().view(-1, V), codes.view(-1), reduction="none").view(B, T)
        nll64 = torch.from_numpy(g["nll64"])
        assert bool(((nll.double() - ref).abs().cpu() <= 2e-6 + 1e-6 * nll64.abs()).all())
        # the mean moves with the logits: |d nll| <= 2 max|d logits| per position; the logits' tolerance is the exact mode's / the 16-bit whole-tensor error
        tol = 2 * (EXACT_RATIO * float(g["ref32_err"]) + 1e-6) if not use_fp16 else 2 * (logits.cpu().double() - gold).abs().max().item() + 2e-6
        assert abs(mean.item() - float(nll64.mean())) <= tol, (mean.item(), float(nll64.mean()), tol)
        assert abs(mean.item() - ref.mean().item()) <= 3e-6 + 1e-6 * ref.mean().item()


def test_chunks_equal_separate_calls(golden_dir):
    m, P, conds, codes, gold, g = _case(golden_dir, "tiny")
    C, H, L, V, T, B = FC.CASES["tiny"]
    gen = torch.Generator().manual_seed(4)
    conds5 = torch.randint(0, FC.VOCAB_COND, (5, 1), generator=gen).cuda()
    codes5 = torch.randint(0, V, (5, T), generator=gen).cuda()
    for use_fp16 in (True, False):
        m.forward_hidden_cap = 2 * T * 4 * C * (6 if use_fp16 else 4)      # two sequences per chunk: 2 + 2 + 1
        la, na, ma = m(codes5, conds5, use_fp16=use_fp16, return_loss=True)
        parts = [m(codes5[s:s + 2], conds5[s:s + 2], use_fp16=use_fp16, return_loss=True) for s in (0, 2, 4)]
        assert torch.equal(la.view(torch.int32), torch.cat([p[0] for p in parts]).view(torch.int32))
        assert torch.equal(na.view(torch.int32), torch.cat([p[1] for p in parts]).view(torch.int32))
        m.forward_hidden_cap = 1 << 40
        lb, nb, mb = m(codes5, conds5, use_fp16=use_fp16, return_loss=True)      # one chunk of five: other GEMM plans, the same model
        assert rel(lb, la) < (2e-3 if use_fp16 else 1e-5) and abs(mb.item() - ma.item()) < 1e-3
        l2, n2, m2 = m(codes5, conds5, use_fp16=use_fp16, return_loss=True)
        assert torch.equal(lb.view(torch.int32), l2.view(torch.int32)) and mb.item() == m2.item()      # the same bits on every run


def test_load_state_dict_refreshes_the_operand_copies(golden_dir):
    m, P, conds, codes, gold, g = _case(golden_dir, "tiny")
    la = m(codes, conds)
    P2 = FC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=FC.PARAM_SEED + 1)
    m.load_state_dict(P2)
    lb = m(codes, conds)
    assert rel(lb, la) > 0.5, "the second forward still ran the old weights"
    m.load_state_dict(P)
    assert torch.equal(m(codes, conds).view(torch.int32), la.view(torch.int32))
    with torch.no_grad():
        m.head.weight.mul_(2.0)      # an in-place change of a master
    assert rel(m(codes, conds), 2 * la) < 1e-3


def test_refusals(golden_dir):
    m, P, conds, codes, gold, g = _case(golden_dir, "tiny")
    V = FC.CASES["tiny"][3]
    with pytest.raises(ValueError):
        m(codes[:, :-1], conds)
    bad = codes.clone()
    bad[0, 3] = V
    with pytest.raises(ValueError):
        m(bad, conds)
    with pytest.raises(NotImplementedError, match="forward"):
        m(codes.cpu(), conds.cpu())


def test_cond_transformer_validation_loss():
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
    images = torch.rand(3, 3, 32, 32).cuda()
    batch = {"image": images, "class": torch.tensor([0, 2, 1]).cuda()}
    loss = ct.validation_step(batch, 0)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    assert ct.logged["val/total_loss"] is loss
    codes = ct.stage1_model.encode_codes(images)
    logits, flat = ct(codes, batch["class"])
    assert tuple(logits.shape) == (3, 16, 64) and torch.equal(flat, codes.view(-1, codes.shape[-1]))
    ref = F.cross_entropy(logits.double().view(-1, 64), flat.reshape(-1))
    assert abs(loss.item() - ref.item()) <= 3e-6 + 1e-6 * ref.item()
    assert abs(ct.shared_step(batch, 0).item() - loss.item()) == 0.0
    with pytest.raises(NotImplementedError, match="training"):
        ct.training_step(batch, 0)
    with pytest.raises(NotImplementedError, match="training"):
        ct.configure_optimizers()


def test_eval_gpt_nll_tool_prints_one_json_line(tmp_path, capsys):
    import json
    import math
    import sys
    import yaml
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import eval_gpt_nll
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    cfg = dict(model=dict(target="enhancing.modules.stage2.transformer.CondTransformer", params=dict(
        cond_key="class", code_shape=[16],
        cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
        stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                    params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=tower, quantizer=dict(embed_dim=32, n_embed=64),
                                loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
        transformer=dict(target="enhancing.modules.stage2.layers.GPT",
                         params=dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, n_heads=2, n_layers=1)))))
    path = tmp_path / "tiny_gpt.yaml"
    path.write_text(yaml.safe_dump(cfg))
    torch.manual_seed(0)
    eval_gpt_nll.main(["-c", str(path), "--synthetic", "3", "--batch_size", "2"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    r = json.loads(line[0])
    assert r["images"] == 3 and r["codes"] == 48 and math.isfinite(r["val/total_loss"])
    assert abs(r["bits_per_code"] - r["val/total_loss"] / math.log(2)) < 1e-12
    assert 0.5 * math.log(64) < r["val/total_loss"] < 2 * math.log(64)      # an untrained prior: about log V
