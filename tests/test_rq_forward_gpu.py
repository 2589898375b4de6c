"""RQTransformer.forward on the device against the reference's golden logits (tests/golden/rq_fwd_<case>.npz, fp64), for both `code_sum` modes, in
the exact mode and in both 16-bit modes, and the behaviour around it: the loss, chunked batches, reloaded weights, the tile-kernel A/B switch,
CondTransformer over a residual stage 1, tools/eval_gpt_nll.py.  The bounds are the rules of tests/test_gpt_forward_gpu.py.

Exact mode: max |logits - fp64 golden| <= 4 x (the fp32 reference module's own max error against the same golden) + 1e-6.
16-bit modes: error <= 2 x the emulation's + the format's rounding floor, over the whole tensor and over every slice of 32 rows of the B T D axis;
the emulation is tests/rq_cases.py forward_logits with every GEMM operand, q / k / v and the softmax numerators rounded, products in fp64.

Measured on MI355X (the figures each test prints).  Exact mode, error / fp32 reference's error, depth | channels: rq_tiny 0.386 |
0.721, rq_d3 0.317 | 0.393, rq_hs384 0.841 | 0.800, rq_d8 0.424 | 0.600, rq_long 0.444 | 0.661 (max errors 6.8e-7 .. 1.3e-6).  16-bit modes, worst
kernel / (2 x emulation + floor) over all slices: 0.400 - 0.435 over the five cases, both modes and both formats; with ENH_RQ_DEPTH_ATTN=tile
0.405 - 0.432."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rq_cases as RC
from util import floor16, rel

pytestmark = pytest.mark.gpu

EXACT_RATIO = 4.0
MODES = ["depth", "channels"]
_EMU = {}


def _case(golden_dir, name, mode):
    from enhancing.modules.stage2.layers import RQTransformer
    g = np.load(os.path.join(golden_dir, f"rq_fwd_{name}.npz"))
    m = RQTransformer(**RC.case_kwargs(name), code_sum=mode)
    P = RC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    return (m.cuda(), P, torch.from_numpy(g["conds"]).cuda(), torch.from_numpy(g["codes"]).long().cuda(), torch.from_numpy(g[f"logits64_{mode}"]), g)


def _within_emulation(got, gold, emu, dt, what):
    """the rule of test_gpt_forward_gpu.py over [B T D, V] rows: whole tensor and every slice of 32 rows; returns the worst kernel / limit"""
    V = gold.shape[-1]
    got, gold, emu = got.reshape(-1, V), gold.reshape(-1, V), emu.reshape(-1, V)
    worst = 0.0
    for sl in [slice(t, t + 32) for t in range(0, gold.shape[0], 32)] + [slice(None)]:
        ek, ee, fl = rel(got[sl], gold[sl]), rel(emu[sl], gold[sl]), floor16(gold[sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        assert ek <= 2 * ee + fl, (what, sl, ek, ee, fl)
    print(f"{what}: whole-tensor error {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}; worst kernel / (2 emulation + floor) over the slices {worst:.3f}")
    return worst


def _emulation(name, mode, fmt, P, conds, codes):
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[fmt]
    if (name, mode, fmt) not in _EMU:
        _EMU[(name, mode, fmt)] = RC.forward_logits({k: v.cuda() for k, v in P.items()}, name, conds, codes, mode,
                                                    rnd=lambda t: t.to(dt).to(torch.float32), prod=torch.float64).cpu()
    return _EMU[(name, mode, fmt)], dt


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RC.CASES))
def test_exact_mode_against_the_fp64_golden(golden_dir, name, mode):
    m, P, conds, codes, gold, g = _case(golden_dir, name, mode)
    C, Hs, Hd, Ls, Ld, V, T, D, B = RC.CASES[name]
    logits = m(codes, conds, use_fp16=False)
    assert tuple(logits.shape) == (B * T, D, V) and logits.dtype == torch.float32 and not logits.requires_grad
    err = (logits.cpu().double() - gold).abs().max().item()
    ref_err = float(g[f"ref32_err_{mode}"])
    print(f"exact {name} {mode}: max err {err:.3e}, fp32 reference {ref_err:.3e}, ratio {err / ref_err:.3f}")
    assert err <= EXACT_RATIO * ref_err + 1e-6, (err, ref_err)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RC.CASES))
def test_16_bit_modes_against_the_emulation(golden_dir, name, mode, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    monkeypatch.delenv("ENH_RQ_DEPTH_ATTN", raising=False)
    m, P, conds, codes, gold, g = _case(golden_dir, name, mode)
    got = m(codes, conds, use_fp16=True).cpu()
    emu, dt = _emulation(name, mode, fmt, P, conds, codes)
    _within_emulation(got, gold, emu, dt, f"{fmt} {name} {mode}")


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["rq_d3", "rq_d8"])
def test_tile_kernel_switch_stays_within_the_bound(golden_dir, name, fmt, monkeypatch):
    """ENH_RQ_DEPTH_ATTN=tile runs the depth attention on gpt_prefill_causal_kernel at N = D: another kernel, the same bound"""
    from enhancing import _C
    monkeypatch.setenv("ENH_PRECISION", fmt)
    monkeypatch.setenv("ENH_RQ_DEPTH_ATTN", "tile")
    m, P, conds, codes, gold, g = _case(golden_dir, name, "depth")
    calls = []
    monkeypatch.setattr(_C, "short_causal_attention", lambda *a, **k: calls.append(a))
    got = m(codes, conds, use_fp16=True).cpu()
    assert not calls, "the switch still ran the short-sequence kernel"
    emu, dt = _emulation(name, "depth", fmt, P, conds, codes)
    _within_emulation(got, gold, emu, dt, f"tile {fmt} {name}")


@pytest.mark.parametrize("use_fp16", [False, True])
def test_loss_is_the_cross_entropy_of_the_returned_logits(golden_dir, use_fp16):
    for name, mode in (("rq_tiny", "depth"), ("rq_d3", "channels"), ("rq_long", "depth")):
        m, P, conds, codes, gold, g = _case(golden_dir, name, mode)
        C, Hs, Hd, Ls, Ld, V, T, D, B = RC.CASES[name]
        logits, nll, mean = m(codes, conds, use_fp16=use_fp16, return_loss=True)
        assert tuple(nll.shape) == (B * T, D) and mean.dim() == 0
        ref = F.cross_entropy(logits.double().view(-1, V), codes.view(-1), reduction="none").view(B * T, D)
        nll64 = torch.from_numpy(g[f"nll64_{mode}"])
        assert bool(((nll.double() - ref).abs().cpu() <= 2e-6 + 1e-6 * nll64.abs()).all())
        # the mean moves with the logits: |d nll| <= 2 max|d logits| per position; the logits' tolerance is the exact mode's / the 16-bit whole-tensor error
        tol = 2 * (EXACT_RATIO * float(g[f"ref32_err_{mode}"]) + 1e-6) if not use_fp16 else 2 * (logits.cpu().double() - gold).abs().max().item() + 2e-6
        assert abs(mean.item() - float(nll64.mean())) <= tol, (mean.item(), float(nll64.mean()), tol)
        assert abs(mean.item() - ref.mean().item()) <= 3e-6 + 1e-6 * ref.mean().item()


def test_chunks_equal_separate_calls(golden_dir):
    m, P, conds, codes, gold, g = _case(golden_dir, "rq_tiny", "depth")
    C, Hs, Hd, Ls, Ld, V, T, D, B = RC.CASES["rq_tiny"]
    gen = torch.Generator().manual_seed(4)
    conds5 = torch.randint(0, RC.VOCAB_COND, (5, 1), generator=gen).cuda()
    codes5 = torch.randint(0, V, (5, T, D), generator=gen).cuda()
    for use_fp16 in (True, False):
        m.forward_hidden_cap = 2 * T * D * 4 * C * (6 if use_fp16 else 4)      # two images per chunk (the cap counts the depth activation): 2 + 2 + 1
        la, na, ma = m(codes5, conds5, use_fp16=use_fp16, return_loss=True)
        assert next(iter(m._fwd_states))[0] == 2 and tuple(la.shape) == (5 * T, D, V) and tuple(na.shape) == (5 * T, D)
        parts = [m(codes5[s:s + 2], conds5[s:s + 2], use_fp16=use_fp16, return_loss=True) for s in (0, 2, 4)]
        assert torch.equal(la.view(torch.int32), torch.cat([p[0] for p in parts]).view(torch.int32))
        assert torch.equal(na.view(torch.int32), torch.cat([p[1] for p in parts]).view(torch.int32))
        m.forward_hidden_cap = 1 << 40
        lb, nb, mb = m(codes5, conds5, use_fp16=use_fp16, return_loss=True)      # one chunk of five: other GEMM plans, the same model
        assert rel(lb, la) < (2e-3 if use_fp16 else 1e-5) and abs(mb.item() - ma.item()) < 1e-3
        l2, n2, m2 = m(codes5, conds5, use_fp16=use_fp16, return_loss=True)
        assert torch.equal(lb.view(torch.int32), l2.view(torch.int32)) and mb.item() == m2.item()      # the same bits on every run


def test_load_state_dict_refreshes_the_operand_copies(golden_dir):
    m, P, conds, codes, gold, g = _case(golden_dir, "rq_tiny", "depth")
    la = m(codes, conds)
    P2 = RC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=RC.PARAM_SEED + 1)
    m.load_state_dict(P2)
    lb = m(codes, conds)
    assert rel(lb, la) > 0.5, "the second forward still ran the old weights"
    m.load_state_dict(P)
    assert torch.equal(m(codes, conds).view(torch.int32), la.view(torch.int32))
    with torch.no_grad():
        m.head.weight.mul_(2.0)      # an in-place change of a master
    assert rel(m(codes, conds), 2 * la) < 1e-3


def test_refusals(golden_dir):
    m, P, conds, codes, gold, g = _case(golden_dir, "rq_tiny", "depth")
    V = RC.CASES["rq_tiny"][5]
    with pytest.raises(ValueError):
        m(codes[:, :-1], conds)
    with pytest.raises(ValueError):
        m(codes[:, :, :-1], conds)
    bad = codes.clone()
    bad[0, 3, 1] = V
    with pytest.raises(ValueError):
        m(bad, conds)
    with pytest.raises(NotImplementedError, match="forward"):
        m(codes.cpu(), conds.cpu())


TINY_RQ = dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, depth_num_tokens=4, spatial_n_heads=2,
               depth_n_heads=2, spatial_n_layers=1, depth_n_layers=1)


def _tiny_cfg():
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    return dict(cond_key="class",
                cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
                stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                            params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=tower,
                                        quantizer=dict(embed_dim=32, n_embed=64, use_residual=True, num_quantizers=4),
                                        loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
                transformer=dict(target="enhancing.modules.stage2.layers.RQTransformer", params=TINY_RQ))


def test_cond_transformer_validation_loss_over_a_residual_stage1():
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    torch.manual_seed(0)
    cfg = AttrDict.wrap(_tiny_cfg())
    ct = CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer)
    images = torch.rand(3, 3, 32, 32).cuda()
    batch = {"image": images, "class": torch.tensor([0, 2, 1]).cuda()}
    loss = ct.validation_step(batch, 0)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    assert ct.logged["val/total_loss"] is loss
    codes = ct.stage1_model.encode_codes(images)
    assert tuple(codes.shape) == (3, 16, 4)
    logits, flat = ct(codes, batch["class"])
    assert tuple(logits.shape) == (3 * 16, 4, 64) and torch.equal(flat, codes.view(-1, 4))
    assert loss.item() == ct.transformer(codes, batch["class"], return_loss=True)[2].item()
    ref = F.cross_entropy(logits.double().view(-1, 64), flat.reshape(-1))
    assert abs(loss.item() - ref.item()) <= 3e-6 + 1e-6 * ref.item()
    assert abs(ct.shared_step(batch, 0).item() - loss.item()) == 0.0
    with pytest.raises(NotImplementedError, match="RQ training"):
        ct.training_step(batch, 0)


def test_eval_gpt_nll_tool_prints_one_json_line(tmp_path, capsys):
    import json
    import math
    import sys
    import yaml
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import eval_gpt_nll
    cfg = dict(model=dict(target="enhancing.modules.stage2.transformer.CondTransformer", params=_tiny_cfg()))
    path = tmp_path / "tiny_rq.yaml"
    path.write_text(yaml.safe_dump(cfg))
    torch.manual_seed(0)
    eval_gpt_nll.main(["-c", str(path), "--synthetic", "2", "--batch_size", "2"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    r = json.loads(line[0])
    assert r["images"] == 2 and r["codes"] == 2 * 16 * 4 and math.isfinite(r["val/total_loss"])
    assert abs(r["bits_per_code"] - r["val/total_loss"] / math.log(2)) < 1e-12
    assert 0.5 * math.log(64) < r["val/total_loss"] < 2 * math.log(64)      # an untrained prior: about log V
