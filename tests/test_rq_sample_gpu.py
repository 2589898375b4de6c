"""RQTransformer.sample on the device against the reference's golden logits (tests/golden/rq_sample_<case>.npz: the reference's cached spatial /
depth loop in fp64, fed with forced codes; `twice` its sample_depth_step line for line, `once` with one ln_depth at slot 0), in the exact mode and
in both 16-bit modes, and the behaviour around it: seeds, chunked batches, reloaded weights, refusals, the depth-attention A/B switch,
CondTransformer over a residual stage 1, tools/sample_images.py.

Exact mode: max |logits - fp64 golden| <= 4 x (the fp32 reference module's own max error against the same golden) + 1e-6: the RQ forward's constant
(tests/test_rq_forward_gpu.py).
16-bit modes: the rule of tests/test_gpt_sample_gpu.py: error <= 2 x the emulation's + the format's rounding floor, per (t, d) step and over the
whole tensor; the emulation is tests/rq_sample_cases.py step_logits on the device with every GEMM operand and cache entry rounded, products in fp64.

Measured on MI355X (the figures each test prints).  Exact mode, error / fp32 reference's error, once | twice: rq_tiny 1.049 | 0.981,
rq_d3 0.989 | 1.137, rq_hs384 0.685 | 0.667, rq_d8 0.949 | 1.003, rq_t70 0.879 | 0.819 (max errors 7.3e-7 .. 1.06e-6).  16-bit modes, worst kernel /
(2 x emulation + floor) over the steps: 0.43 - 0.57 over the five cases and both formats; with ENH_RQ_DEPTH_DECODE=cache the default's figures."""
import os

import numpy as np
import pytest
import torch

import rq_sample_cases as SC
from util import floor16, rel

pytestmark = pytest.mark.gpu

EXACT_RATIO = 4.0
_EMU = {}


def _case(golden_dir, name, **kw):
    from enhancing.modules.stage2.layers import RQTransformer
    g = np.load(os.path.join(golden_dir, f"rq_sample_{name}.npz"))
    m = RQTransformer(**SC.case_kwargs(name), **kw)
    P = SC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict(P, strict=True)
    return m.cuda(), P, torch.from_numpy(g["conds"]).cuda(), torch.from_numpy(g["forced_codes"]).long().cuda(), g


def _exact(golden_dir, name, mode, what):
    m, P, conds, forced, g = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    logits, codes = m.sample(conds, use_fp16=False, forced_codes=forced, seed=1, slot0_ln=mode)
    assert tuple(logits.shape) == (B * T, D, V) and logits.dtype == torch.float32
    assert tuple(codes.shape) == (B, T, D) and codes.dtype == torch.int64 and int(codes.min()) >= 0 and int(codes.max()) < V
    err = (logits.cpu().double() - torch.from_numpy(g[f"logits64_{mode}"])).abs().max().item()
    ref_err = float(g[f"ref32_err_{mode}"])
    print(f"{what} {name} slot0_ln={mode}: max err {err:.3e}, fp32 reference {ref_err:.3e}, ratio {err / ref_err:.3f}")
    assert err <= EXACT_RATIO * ref_err + 1e-6, (name, mode, err, ref_err)


def _sixteen(golden_dir, name, fmt, mode, what):
    """(ENH_PRECISION is already set) kernel error <= 2 x emulation error + floor16, per (t, d) step and over the whole tensor"""
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[fmt]
    m, P, conds, forced, g = _case(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = SC.CASES[name]
    logits, _ = m.sample(conds, use_fp16=True, forced_codes=forced, seed=1, slot0_ln=mode)
    got = logits.view(B, T, D, V).cpu()
    gold = torch.from_numpy(g[f"logits64_{mode}"]).view(B, T, D, V)
    if (name, fmt, mode) not in _EMU:
        _EMU[(name, fmt, mode)] = SC.step_logits({k: v.cuda() for k, v in P.items()}, name, conds, forced, mode,
                                                 rnd=lambda t: t.to(dt).to(torch.float32), prod=torch.float64).view(B, T, D, V).cpu()
    emu = _EMU[(name, fmt, mode)]
    worst = 0.0
    for t, d in [(t, d) for t in range(T) for d in range(D)] + [(None, None)]:
        sl = (slice(None), slice(None), slice(None)) if t is None else (slice(None), t, d)
        ek, ee, fl = rel(got[sl], gold[sl]), rel(emu[sl], gold[sl]), floor16(gold[sl], dt)
        worst = max(worst, ek / (2 * ee + fl))
        assert ek <= 2 * ee + fl, (name, fmt, mode, t, d, ek, ee, fl)
    print(f"{what} {fmt} {name} slot0_ln={mode}: whole-tensor error {ek:.3e}, emulation {ee:.3e}, floor {fl:.3e}; worst kernel / (2 emulation + "
          f"floor) over the steps {worst:.3f}")


@pytest.mark.parametrize("mode", ["once", "twice"])
@pytest.mark.parametrize("name", list(SC.CASES))
def test_exact_mode_against_the_fp64_golden(golden_dir, name, mode):
    _exact(golden_dir, name, mode, "exact")


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(SC.CASES))
def test_16_bit_modes_against_the_emulation(golden_dir, name, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    _sixteen(golden_dir, name, fmt, "once", "16-bit")


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_16_bit_modes_with_the_reference_s_second_ln_depth(golden_dir, fmt, monkeypatch):
    monkeypatch.setenv("ENH_PRECISION", fmt)
    _sixteen(golden_dir, "rq_tiny", fmt, "twice", "16-bit")


@pytest.mark.parametrize("name", ["rq_d3", "rq_d8"])
def test_depth_decode_switch_meets_the_same_bounds(golden_dir, name, monkeypatch):
    """ENH_RQ_DEPTH_DECODE=cache: enh_decode_attention at Tmax = D in the depth transformer (the A/B of DESIGN.md §3.11)"""
    from enhancing import _C
    monkeypatch.setenv("ENH_RQ_DEPTH_DECODE", "cache")
    calls = []
    monkeypatch.setattr(_C, "short_decode_attention", lambda *a, **k: calls.append(1))
    _exact(golden_dir, name, "once", "exact, depth decode = cache")
    monkeypatch.setenv("ENH_PRECISION", "fp16")
    _sixteen(golden_dir, name, "fp16", "once", "depth decode = cache")
    assert not calls, "the switch did not take the short kernel out"
    monkeypatch.setenv("ENH_RQ_DEPTH_DECODE", "tile")
    m, P, conds, forced, g = _case(golden_dir, name)
    with pytest.raises(ValueError, match="ENH_RQ_DEPTH_DECODE"):
        m.sample(conds)


def _scaled_model(**kw):
    from enhancing.modules.stage2.layers import RQTransformer
    torch.manual_seed(0)
    m = RQTransformer(vocab_cond_size=10, vocab_img_size=256, embed_dim=128, cond_num_tokens=1, img_num_tokens=3, depth_num_tokens=2, spatial_n_heads=2,
                      depth_n_heads=2, spatial_n_layers=1, depth_n_layers=1, **kw).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(6.0)      # logits of scale ~1 instead of the init's ~0.2
    return m


def test_seed_gives_the_same_codes_and_chunks_equal_separate_calls():
    m = _scaled_model()
    conds = (torch.arange(70) % 10).view(70, 1).cuda()
    kw = dict(top_k=40, top_p=0.95, softmax_temperature=0.9)
    l1, c1 = m.sample(conds, seed=5, **kw)
    l2, c2 = m.sample(conds, seed=5, **kw)
    assert tuple(l1.shape) == (70 * 3, 2, 256) and tuple(c1.shape) == (70, 3, 2)
    assert torch.equal(c1, c2) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    _, c3 = m.sample(conds, seed=6, **kw)
    assert not torch.equal(c1, c3)
    _, c4 = m.sample(conds, seed=5, call=1, **kw)
    assert not torch.equal(c1, c4)
    # 70 rows = a chunk of 64 and one of 6: the same as two calls on those rows with the same seed and row numbers
    la, ca = m.sample(conds[:64], seed=5, **kw)
    lb, cb = m.sample(conds[64:], seed=5, row_offset=64, **kw)
    assert torch.equal(c1, torch.cat([ca, cb])) and torch.equal(l1.view(torch.int32), torch.cat([la, lb]).view(torch.int32))
    assert len(torch.unique(c1)) > 20
    # the logits are after the temperature and the top-k mask: 40 finite entries per row
    assert bool((torch.isfinite(l1).sum(-1) == 40).all())
    # the drawn codes are fed forward: forcing them reproduces the logits
    lf, _ = m.sample(conds, seed=9, forced_codes=c1, **kw)
    assert torch.equal(lf.view(torch.int32), l1.view(torch.int32))
    none, cn = m.sample(conds[:2], return_logits=False)
    assert none is None and tuple(cn.shape) == (2, 3, 2) and cn.dtype == torch.int64


def test_load_state_dict_refreshes_the_operand_copies(golden_dir):
    m, P, conds, forced, g = _case(golden_dir, "rq_tiny")
    la, _ = m.sample(conds, forced_codes=forced, seed=1)
    P2 = SC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=SC.PARAM_SEED + 1)
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


def test_refusals(golden_dir):
    m, P, conds, forced, g = _case(golden_dir, "rq_tiny")
    V = SC.CASES["rq_tiny"][5]
    with pytest.raises(ValueError, match="top_k"):
        m.sample(conds, top_k=V + 1)
    with pytest.raises(ValueError, match="top_k"):
        m.sample(conds, top_k=0)
    with pytest.raises(ValueError, match="forced_codes outside"):
        m.sample(conds, forced_codes=forced + V)
    with pytest.raises(ValueError, match="forced_codes must be"):
        m.sample(conds, forced_codes=forced[:, :-1])
    with pytest.raises(ValueError, match="slot0_ln"):
        m.sample(conds, slot0_ln="thrice")
    with pytest.raises(NotImplementedError, match="sampling runs on a ROCm device only"):
        m.sample(conds.cpu())
    mc, *_ = _case(golden_dir, "rq_tiny", code_sum="channels")
    with pytest.raises(ValueError, match="sums the code embeddings over depth"):
        mc.sample(conds)


TINY_RQ = dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, depth_num_tokens=2, spatial_n_heads=2,
               depth_n_heads=2, spatial_n_layers=1, depth_n_layers=1)


def _tiny_cfg():
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    return dict(cond_key="class", code_shape=[16, 2],
                cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
                stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                            params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=tower,
                                        quantizer=dict(embed_dim=32, n_embed=64, use_residual=True, num_quantizers=2),
                                        loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
                transformer=dict(target="enhancing.modules.stage2.layers.RQTransformer", params=TINY_RQ))


def test_cond_transformer_samples_images_over_a_residual_stage1():
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    torch.manual_seed(0)
    cfg = AttrDict.wrap(_tiny_cfg())
    ct = CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer, code_shape=[16, 2])
    conds = torch.tensor([0, 2, 1]).cuda()
    img = ct.sample(conds, top_k=20, seed=3)
    assert tuple(img.shape) == (3, 3, 32, 32) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    assert tuple(ct.last_codes.shape) == (3, 16, 2) and ct.last_codes.dtype == torch.int64
    assert torch.equal(img, ct.stage1_model.decode_codes(ct.last_codes).clamp(0, 1))
    img2 = ct.sample(conds, top_k=20, seed=3)
    assert torch.equal(img, img2)
    _, codes = ct.transformer.sample(conds.view(3, 1), top_k=20, seed=3, return_logits=False)
    assert torch.equal(codes, ct.last_codes)


def test_sample_images_tool_accepts_the_rq_config(tmp_path, capsys):
    import sys
    import yaml
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import sample_images
    cfg = dict(model=dict(target="enhancing.modules.stage2.transformer.CondTransformer", params=_tiny_cfg()))
    path, out = tmp_path / "tiny_rq.yaml", tmp_path / "samples.png"
    path.write_text(yaml.safe_dump(cfg))
    torch.manual_seed(0)
    sample_images.main(["-c", str(path), "--classes", "0", "2", "--top_k", "20", "--seed", "1", "--nrow", "2", "--out", str(out)])
    assert "2 images (3, 32, 32)" in capsys.readouterr().out
    assert Image.open(out).size[0] >= 64
