"""The contract of the stage-2 RQTransformer's teacher-forced forward on the CPU: the module's parameters, init and refusals, and
tests/golden/rq_fwd_<case>.npz (the reference's RQTransformer in fp64, tools/make_golden_rq_forward.py) against the plain-torch restatement of
tests/rq_cases.py that the device tests use as their yardstick."""
import os

import numpy as np
import pytest
import torch

import rq_cases as RC

torch.set_num_threads(4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["depth", "channels"]


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"rq_fwd_{name}.npz"))
    shapes = {str(k): tuple(int(d) for d in s if d) for k, s in zip(g["state_names"], g["state_shapes"])}
    return g, shapes, torch.from_numpy(g["conds"]), torch.from_numpy(g["codes"]).long()


def _rq(**over):
    from enhancing.modules.stage2.layers import RQTransformer
    return RQTransformer(**dict(RC.case_kwargs("rq_tiny"), **over))


@pytest.mark.parametrize("name", list(RC.CASES))
def test_state_dict_names_and_shapes_are_the_references(golden_dir, name):
    from enhancing.modules.stage2.layers import RQTransformer
    g, shapes, conds, codes = _load(golden_dir, name)
    m = RQTransformer(**RC.case_kwargs(name))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes
    C, Hs, Hd, Ls, Ld, V, T, D, B = RC.CASES[name]
    assert len(shapes) == 10 + 17 * (Ls + Ld)      # 44 at one spatial and one depth layer
    assert shapes["pos_emb_depth"] == (1, D - 1, C) and shapes["ln_spatial.weight"] == (C,) and shapes["head.weight"] == (V, C)
    assert tuple(codes.shape) == (B, T, D) and torch.equal(codes, RC.case_inputs(name)[1])
    m.load_state_dict(RC.make_params(shapes), strict=True)


def test_init_is_the_references():
    torch.manual_seed(0)
    m = _rq(embed_dim=256, vocab_img_size=512, img_num_tokens=64)
    for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):      # torch.rand
        assert 0.0 <= p.min().item() and p.max().item() < 1.0
    assert abs(m.pos_emb_code.mean().item() - 0.5) < 0.02
    for w in (m.head.weight, m.tok_emb_code.weight, m.spatial_transformer[0].mlp.p0.weight, m.depth_transformer[0].attn.query.weight):
        assert abs(w.std().item() - 0.02) < 0.002 and abs(w.mean().item()) < 0.002
    assert m.depth_transformer[0].mlp.p1.bias.detach().abs().max().item() == 0.0
    assert bool((m.ln_depth.weight == 1).all()) and bool((m.ln_spatial.bias == 0).all())
    tm = m.depth_transformer[0].attn.time_mix
    assert tuple(tm.shape) == (1, 1, 256) and tm[0, 0, 0].item() == 0.0 and tm[0, 0, -1].item() == 1.0
    assert m.code_sum == "depth" and _rq(code_sum="channels").code_sum == "channels"


@pytest.mark.parametrize("over,match", [
    (dict(cond_num_tokens=2), "cond_num_tokens"),
    (dict(depth_num_tokens=1), "use GPT"),
    (dict(depth_num_tokens=9), "depth_num_tokens"),
    (dict(depth_num_tokens=0), "depth_num_tokens"),
    (dict(spatial_n_heads=4), "spatial_n_heads"),                         # head size 32
    (dict(depth_n_heads=4), "depth_n_heads"),
    (dict(embed_dim=512, spatial_n_heads=1, depth_n_heads=2), "spatial_n_heads"),      # head size 512 > 384
    (dict(embed_dim=512, spatial_n_heads=2, depth_n_heads=1), "depth_n_heads"),
    (dict(spatial_n_heads=3), "multiple"),
    (dict(embed_dim=8192 + 128, spatial_n_heads=65, depth_n_heads=65), "embed_dim"),
    (dict(vocab_img_size=16384 + 8), "vocab_img_size"),
    (dict(vocab_img_size=60), "multiple of 8"),
    (dict(img_num_tokens=8193), "img_num_tokens"),
    (dict(code_sum="rows"), "code_sum"),
])
def test_constructor_refusals(over, match):
    with pytest.raises(ValueError, match=match):
        _rq(**over)


def test_code_sum_is_keyword_only():
    with pytest.raises(TypeError):
        from enhancing.modules.stage2.layers import RQTransformer
        RQTransformer(10, 64, 128, 1, 5, 4, 2, 2, 1, 1, True, True, "depth")


def test_the_config_loads():
    from enhancing.utils.general import get_config_from_file
    cfg = get_config_from_file(os.path.join(ROOT, "configs", "imagenet_rqtransformer_rqvae_base.yaml"))
    stage1 = get_config_from_file(os.path.join(ROOT, "configs", "imagenet_rqvae_base.yaml"))
    p = cfg.model.params
    assert p.transformer.target == "enhancing.modules.stage2.layers.RQTransformer"
    t = dict(p.transformer.params)
    assert t == dict(vocab_cond_size=1000, vocab_img_size=8192, embed_dim=1536, cond_num_tokens=1, img_num_tokens=1024, depth_num_tokens=4,
                     spatial_n_heads=12, depth_n_heads=12, spatial_n_layers=24, depth_n_layers=4)
    for k in ("image_size", "patch_size", "encoder", "decoder", "quantizer"):      # its stage 1 is the rqvae_base model
        assert p.stage1.params[k] == stage1.model.params[k], k
    assert p.stage1.params.quantizer.num_quantizers == t["depth_num_tokens"]
    assert (p.stage1.params.image_size // p.stage1.params.patch_size) ** 2 == t["img_num_tokens"]
    from enhancing.modules.stage2.layers import RQTransformer
    with torch.device("meta"):
        m = RQTransformer(**t)
    assert sum(v.numel() for v in m.parameters()) > 7e8


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RC.CASES))
def test_fp64_restatement_is_the_reference(golden_dir, name, mode):
    """pins the yardstick to the reference: "channels" against the reference's own forward, "depth" against its own submodules composed with the
    sum over depth; S = T spatial rows suffice"""
    g, shapes, conds, codes = _load(golden_dir, name)
    C, Hs, Hd, Ls, Ld, V, T, D, B = RC.CASES[name]
    gold = torch.from_numpy(g[f"logits64_{mode}"])
    assert tuple(gold.shape) == (B * T, D, V)
    got = RC.forward_logits(RC.make_params(shapes), name, conds, codes, mode, rnd=None, prod=torch.float64, work=torch.float64)
    assert (got - gold).abs().max().item() <= 1e-9
    nll = torch.nn.functional.cross_entropy(gold.reshape(-1, V), codes.reshape(-1), reduction="none").view(B * T, D)
    assert (nll - torch.from_numpy(g[f"nll64_{mode}"])).abs().max().item() <= 1e-12
    assert float(g[f"ref32_err_{mode}"]) < 1e-4


def test_the_two_code_sums_are_different_models(golden_dir):
    """the quirk: the reference's forward (cumsum along the channels) is not the model its sampler draws from (sum over depth)"""
    g = np.load(os.path.join(golden_dir, "rq_fwd_rq_tiny.npz"))
    a, b = torch.from_numpy(g["logits64_channels"]), torch.from_numpy(g["logits64_depth"])
    assert ((a - b).norm() / b.norm()).item() > 0.1


def _cond_transformer(transformer_params):
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    cfg = AttrDict.wrap(dict(
        cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
        stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                    params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=tower,
                                quantizer=dict(embed_dim=32, n_embed=64, use_residual=True, num_quantizers=4),
                                loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
        transformer=dict(target="enhancing.modules.stage2.layers.RQTransformer", params=transformer_params)))
    return CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer)


def test_cond_transformer_names_what_is_not_built():
    ct = _cond_transformer(dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, depth_num_tokens=4,
                                spatial_n_heads=2, depth_n_heads=2, spatial_n_layers=1, depth_n_layers=1))
    batch = {"image": torch.rand(2, 3, 32, 32), "class": torch.tensor([0, 2])}
    with pytest.raises(NotImplementedError, match="sampling"):
        ct.sample(torch.tensor([0, 2]))
    with pytest.raises(NotImplementedError, match="backward"):
        ct.loss_and_grads(batch)
    with pytest.raises(NotImplementedError, match="RQ training"):
        ct.training_step(batch, 0)
    ct.learning_rate = 1e-4
    with pytest.raises(NotImplementedError, match="RQ training"):
        ct.configure_optimizers()


def test_forward_refuses_cpu_tensors():
    m = _rq()
    conds, codes = RC.case_inputs("rq_tiny")
    with pytest.raises(NotImplementedError, match="forward"):
        m(codes, conds)


def test_new_symbols_are_bound():
    from enhancing import _C
    for name in ("enh_rq_embed_seq", "enh_ln_rows_strided", "enh_short_causal_attention_forward"):
        assert name in _C.SIGNATURES
    for name in ("rq_embed_seq", "ln_rows_strided", "short_causal_attention"):
        assert callable(getattr(_C, name))


RQ_LABELS = [f"rq_short_causal_kernel<{L}, {ot}>" for L in range(1, 9) for ot in ("F16", "BF16")] + ["rq_embed_seq_kernel", "rq_ln_strided_kernel"]


def test_rq_labels_are_kernel_symbols_without_scratch():
    """every label the new launches report (enh_last_kernel) is exactly one kernel symbol of the shipped library; none of them uses scratch or LDS
    beyond the LayerNorm's four reduction words"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"):
        pytest.skip("needs the built library and the ROCm llvm tools")
    stats = isa_lint.kernel_stats()
    for label in RQ_LABELS:
        hits = [n for n in stats if n.startswith(label + "(") or n.startswith("void " + label + "(")]
        assert len(hits) == 1, (label, hits)
        s = stats[hits[0]]
        assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0, (label, s)
