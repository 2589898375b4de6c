"""dim_head as a config choice, end to end, pinned to the reference: the tiny ViT-VQGAN at head widths 32 / 96 / 128 (tests/dim_head_cases.py) against
tests/golden/vit_tiny_dh*.npz, which tools/make_golden_dim_head.py wrote from the reference's OWN modules on the same seeded parameters and images.
Limits are the numbers of tests/test_model_gpu.py."""
import os

import numpy as np
import pytest
import torch

import dim_head_cases as DC
from util import rel

pytestmark = pytest.mark.gpu

ACT_TOL, GRAD_TOL = 1e-2, 3e-2                  # tests/test_model_gpu.py
EXACT_ACT_TOL, EXACT_GRAD_TOL = 1e-5, 1e-5      # tests/test_model_gpu.py
LOSS = {"target": "enhancing.losses.vqperceptual.VQLPIPS",
        "params": dict(codebook_weight=1.0, loglaplace_weight=0.0, loggaussian_weight=1.0, perceptual_weight=0.0)}


def _model(cfg, precision=None):
    """the package's ViTVQ for `cfg` with the seeded parameters of dim_head_cases.make_params (shapes from its own state_dict, position tables its own)"""
    from enhancing.modules.stage1.vitvqgan import ViTVQ
    from enhancing.utils.general import AttrDict
    m = ViTVQ("image", cfg["image_size"], cfg["patch_size"], AttrDict.wrap(cfg["encoder"]), AttrDict.wrap(cfg["decoder"]),
              AttrDict.wrap(cfg["quantizer"]), AttrDict.wrap(LOSS))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("loss.")}
    P = DC.make_params(shapes, cfg)
    missing = m.load_state_dict(P, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("pos_embedding") for k in missing.missing_keys), missing
    if precision is not None:
        m.precision = precision
    assert m.engine.precision == (precision or os.environ.get("ENH_PRECISION", "fp16"))
    return m, shapes


def _images(cfg):
    import vitvq_oracle as O
    return O.make_images(DC.IMAGE_SEED, DC.BATCH, cfg["image_size"])


def _grad_checks(m, g, tol):
    names = list(g["grad_names"])
    m.engine.unscale_grads()      # fp16 engine: param.grad carries the loss scale until the step (or this call)
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None and k in names}
    assert set(grads) == set(names), set(grads) ^ set(names)
    norm_err = {n: abs(grads[n].double().norm().item() - ref) / max(ref, 1e-12) for n, ref in zip(names, g["grad_norms"])}
    worst = max(norm_err, key=norm_err.get)
    rows = torch.from_numpy(g["g_qkv0_rows"]).to(grads[names[0]].device)
    sampled = dict(qkv0=rel(grads["encoder.transformer.layers.0.0.fn.to_qkv.weight"][rows], torch.from_numpy(g["g_qkv0"])),
                   pixel=rel(grads["decoder.to_pixel.1.weight"], torch.from_numpy(g["g_pixel_w"])),
                   codebook=rel(grads["quantizer.embedding.weight"], torch.from_numpy(g["g_codebook"])))
    print(f"  gradients vs REFERENCE: worst norm {worst} {norm_err[worst]:.2e}; sampled tensors " + " ".join(f"{k} {v:.2e}" for k, v in sampled.items()))
    assert norm_err[worst] <= tol, (worst, norm_err[worst])
    assert all(v <= tol for v in sampled.values()), sampled


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_default_engine_against_the_reference_golden(name, golden_dir):
    cfg = DC.case_cfg(name)
    g = np.load(f"{golden_dir}/vit_tiny_{name}.npz")
    m, shapes = _model(cfg)
    x = _images(cfg)
    # state dict: the reference's names and shapes
    ref_shapes = {k: tuple(int(v) for v in s if v) for k, s in zip(g["state_names"], g["state_shapes"])}
    assert shapes == ref_shapes
    assert m.engine.enc.dim_head == m.engine.dec.dim_head == DC.CASES[name][0]
    h = m.pre_quant_tokens(x)
    with torch.no_grad():
        xrec, qloss = m(x)
    e_h, e_x = rel(h, torch.from_numpy(g["h"])), rel(xrec, torch.from_numpy(g["xrec"]))
    codes = m.encode_codes(x)
    match = (codes.cpu().numpy() == g["idx"].astype(np.int64)).mean()
    print(f"{name} fwd vs REFERENCE: h rel {e_h:.2e}, xrec rel {e_x:.2e}, qloss {qloss.item():.6f} vs {float(g['qloss']):.6f}, code match {match:.4f}")
    assert e_h <= ACT_TOL and e_x <= ACT_TOL
    # codes -> image: decode_codes(encode_codes(x)) is reconstruct at the forward's precision
    rec = m.decode_codes(codes)
    xr2, _, idx2 = m.engine.reconstruct(x)
    assert torch.equal(idx2.view(-1), codes.view(-1))
    assert rel(rec, xr2) <= ACT_TOL
    assert m.encode(x)[0].shape == (DC.BATCH, m.engine.n_tok, cfg["quantizer"]["embed_dim"]) and m.decode(m.encode(x)[0]).shape == x.shape
    loss = m.training_step({"image": x}, 0, 0)
    print(f"{name} train step: loss {loss.item():.6f} vs REFERENCE {float(g['loss']):.6f}")
    assert abs(loss.item() - float(g["loss"])) <= 1e-2 * abs(float(g["loss"]))
    _grad_checks(m, g, GRAD_TOL)


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_exact_fp32_mode_against_the_reference_golden(name, golden_dir):
    cfg = DC.case_cfg(name)
    g = np.load(f"{golden_dir}/vit_tiny_{name}.npz")
    m, _ = _model(cfg, precision="fp32")
    x = _images(cfg)
    h = m.pre_quant_tokens(x)
    with torch.no_grad():
        xrec, qloss = m(x)
    codes = m.encode_codes(x)
    e_h, e_x = rel(h, torch.from_numpy(g["h"])), rel(xrec, torch.from_numpy(g["xrec"]))
    print(f"{name} exact mode vs REFERENCE: h rel {e_h:.2e}, xrec rel {e_x:.2e}, qloss {qloss.item():.7f} vs {float(g['qloss']):.7f}")
    assert e_h <= EXACT_ACT_TOL and e_x <= EXACT_ACT_TOL
    assert np.array_equal(codes.cpu().numpy(), g["idx"].astype(np.int64)), "end-to-end code indices must equal the reference's"
    loss = m.training_step({"image": x}, 0, 0)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    _grad_checks(m, g, EXACT_GRAD_TOL)


def _mixed_cfg():
    cfg = DC.case_cfg("dh32")
    cfg["decoder"].update(heads=2, dim_head=128)
    return cfg


def test_mixed_towers_take_a_reproducible_training_step():
    """encoder dim_head 32, decoder dim_head 128: the step runs, the loss is finite and a second model's step gives the same bits"""
    cfg = _mixed_cfg()
    x = _images(cfg)
    losses, grads = [], []
    for _ in range(2):
        m, _ = _model(cfg)
        assert (m.engine.enc.dim_head, m.engine.dec.dim_head) == (32, 128) and (m.engine.enc.inner, m.engine.dec.inner) == (128, 256)
        loss = m.training_step({"image": x}, 0, 0)
        assert bool(torch.isfinite(loss))
        losses.append(loss.detach().clone())
        grads.append(m.decoder.transformer.layers[0][0].fn.to_qkv.weight.grad.detach().clone())
    assert torch.equal(losses[0], losses[1]) and torch.equal(grads[0], grads[1])
    assert bool(torch.isfinite(grads[0]).all()) and float(grads[0].abs().max()) > 0


def test_unsupported_width_and_x3_are_value_errors():
    from enhancing.engine.stage1 import Stage1Engine
    from enhancing.modules.stage1.layers import Attention, ViTEncoder
    with pytest.raises(ValueError, match=r"\(32, 64, 96, 128\)"):
        Attention(128, heads=2, dim_head=80)
    with pytest.raises(ValueError, match=r"\(32, 64, 96, 128\)"):
        ViTEncoder(64, 8, dim=128, depth=1, heads=2, mlp_dim=256, dim_head=80)
    with pytest.raises(ValueError, match="to_out"):
        Attention(96, heads=1, dim_head=96)
    Attention(64, heads=1, dim_head=64)       # the width-64 behaviour is what it was
    cfg = DC.case_cfg("dh32")
    x = _images(cfg)
    m, _ = _model(cfg)
    with pytest.raises(ValueError, match="dim_head = 64 only"):
        m.encode_codes(x, precision="x3")
    with pytest.raises(ValueError, match="dim_head = 64 only"):
        m.pre_quant_tokens(x, precision="x3")
    for kw in (dict(precision="bf16", encoder_precision="x3"), dict(precision="bf16", decoder_precision="x3"), dict(precision="bf16", codes_precision="x3")):
        with pytest.raises(ValueError, match="dim_head = 64 only"):
            Stage1Engine(m, **kw)
    mixed, _ = _model(_mixed_cfg())
    with pytest.raises(ValueError, match="the decoder has dim_head = 128"):
        Stage1Engine(mixed, precision="bf16", decoder_precision="x3")


def test_bf16_engine_defaults_to_single_pass_codes(monkeypatch):
    """under the bf16 engine codes_precision defaults to x3 at dim_head 64; at another encoder width it is the engine's single pass, so encode_codes(x) works"""
    monkeypatch.delenv("ENH_CODES_PRECISION", raising=False)
    cfg = DC.case_cfg("dh32")
    x = _images(cfg)
    m, _ = _model(cfg, precision="bf16")
    assert m.engine.codes_precision == "bf16"
    codes = m.encode_codes(x)
    assert codes.shape == (DC.BATCH, 64) and torch.equal(codes.view(-1), m.engine.reconstruct(x)[2].view(-1))
    assert m.decode_codes(codes).shape == x.shape


def test_the_shipped_dh32_config_loads_and_builds():
    from enhancing.utils.general import get_config_from_file, initialize_from_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    config = get_config_from_file(os.path.join(root, "configs", "imagenet_vitvq_small_dh32.yaml"))
    assert config.model.params.encoder.dim_head == 32 and config.model.params.decoder.heads == 16
    m = initialize_from_config(config.model)
    att = m.encoder.transformer.layers[0][0].fn
    assert (att.heads, att.dim_head) == (16, 32) and tuple(att.to_qkv.weight.shape) == (3 * 512, 512)
    e = m.engine
    assert (e.enc.dim_head, e.dec.dim_head, e.enc.inner, e.dec.inner) == (32, 32, 512, 512) and abs(e.enc.scale - 32 ** -0.5) < 1e-12
