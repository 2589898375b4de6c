"""The model at image / patch sizes whose token count is no multiple of 64: O.TINY_CFG at 48 px (N = 36) and 80 px (N = 100), patch 8, B = 2, against
the CPU oracle with the limits of tests/test_model_gpu.py (ACT_TOL, GRAD_TOL, loss within 1e-2 relative).  The 64-px tiny model (N = 64) meets them
on the aligned attention kernels; a ragged size that misses one has a bug in the tail path."""
import copy

import pytest
import torch

from util import rel

pytestmark = pytest.mark.gpu

ACT_TOL = 1e-2    # tests/test_model_gpu.py
GRAD_TOL = 3e-2
SIZES = [48, 80]


def _build(cfg, P, **kw):
    """tests/test_model_gpu.py::_build (kw: attributes set before the parameters are loaded, as tests/test_x3_gpu.py::_build)"""
    from enhancing.modules.stage1.vitvqgan import ViTVQ
    from enhancing.utils.general import AttrDict
    loss = {"target": "enhancing.losses.vqperceptual.VQLPIPS",
            "params": dict(codebook_weight=1.0, loglaplace_weight=0.0, loggaussian_weight=1.0, perceptual_weight=0.0)}
    m = ViTVQ("image", cfg["image_size"], cfg["patch_size"], AttrDict.wrap(cfg["encoder"]), AttrDict.wrap(cfg["decoder"]),
              AttrDict.wrap(cfg["quantizer"]), AttrDict.wrap(loss))
    for k, v in kw.items():
        setattr(m, k, v)
    m.load_state_dict(P, strict=not any(n.startswith("loss.") for n, _ in m.named_parameters()))
    m.engine  # bind to the GPU
    return m


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s}px")
def ragged(request):
    import vitvq_oracle as O
    assert torch.cuda.is_available()
    cfg = copy.deepcopy(O.TINY_CFG)
    cfg["image_size"] = request.param
    n_tok = (request.param // cfg["patch_size"]) ** 2
    assert n_tok % 64 != 0
    P = O.make_params(cfg, seed=11)
    x = O.make_images(5, 2, cfg["image_size"])
    return cfg, P, x, _build(cfg, P), n_tok


def test_forward_against_the_oracle(ragged):
    import vitvq_oracle as O
    cfg, P, x, m, n_tok = ragged
    h = m.pre_quant_tokens(x)
    xrec, qloss = m(x)
    with torch.no_grad():
        o_q, o_ql, o_idx, o_h = O.encode(x, P, cfg)
        o_xrec, o_qloss = O.forward(x, P, cfg)
    assert h.shape == (2, n_tok, cfg["quantizer"]["embed_dim"]) and xrec.shape == x.shape
    e_h, e_x = rel(h, o_h.view_as(h.cpu())), rel(xrec, o_xrec)
    print(f"{cfg['image_size']} px (N = {n_tok}) fwd vs oracle: h rel {e_h:.2e}, xrec rel {e_x:.2e}, qloss {qloss.item():.6f} vs {o_qloss.item():.6f}")
    assert e_h <= ACT_TOL and e_x <= ACT_TOL
    assert abs(qloss.item() - o_qloss.item()) <= 1e-2 * abs(o_qloss.item())


def test_quantizer_indices_equal_the_oracle_on_identical_input(ragged):
    import vitvq_oracle as O
    cfg, P, x, m, n_tok = ragged
    h = m.pre_quant_tokens(x)
    zq, loss, idx = m.quantizer(h)
    zq_o, loss_o, idx_o = O.quantizer_forward(h.cpu(), P["quantizer.embedding.weight"])
    assert torch.equal(idx.cpu(), idx_o)
    assert rel(zq, zq_o) <= 1e-6 and abs(loss.item() - loss_o.item()) <= 1e-6


def test_decode_codes_roundtrip(ragged):
    import vitvq_oracle as O
    cfg, P, x, m, n_tok = ragged
    codes = m.encode_codes(x)
    assert codes.shape == (2, n_tok)
    rec = m.decode_codes(codes)
    ref = O.decode_codes(codes.cpu(), P, cfg)
    assert rel(rec, ref) <= ACT_TOL


def test_train_step_gradients_vs_oracle(ragged):
    import vitvq_oracle as O
    cfg, P, x, m, n_tok = ragged
    loss = m.training_step({"image": x}, 0, 0)
    o_loss, o_log, o_grads, o_xrec = O.train_step_grads(x, P, cfg)
    assert abs(loss.item() - o_loss.item()) <= 1e-2 * abs(o_loss.item())
    m.engine.unscale_grads()      # fp16 engine: param.grad carries the loss scale until the step (or this call)
    errs = {k: rel(p.grad, o_grads[k]) for k, p in m.named_parameters() if k in o_grads}
    worst = max(errs, key=errs.get)
    print(f"{cfg['image_size']} px (N = {n_tok}) train-step grads vs oracle: worst {worst} {errs[worst]:.2e}")
    assert set(errs) == set(o_grads)
    assert errs[worst] <= GRAD_TOL, errs


def test_x3_encoder_at_a_ragged_token_count(ragged):
    """the split-operand encoder (tests/test_x3_gpu.py builds it on the bf16 product path): h within the 5e-5 the x3 golden test asks"""
    import vitvq_oracle as O
    cfg, P, x, _, n_tok = ragged
    m = _build(cfg, P, precision="bf16")
    codes = m.encode_codes(x, precision="x3")
    assert codes.shape == (2, n_tok) and codes.dtype == torch.int64
    h = m.pre_quant_tokens(x, precision="x3")
    with torch.no_grad():
        o_h = O.encode(x, P, cfg)[3]
    e_h = rel(h, o_h.view_as(h.cpu()))
    print(f"{cfg['image_size']} px (N = {n_tok}) x3 encoder vs oracle: h rel {e_h:.2e}")
    assert e_h <= 5e-5


def test_training_rejects_a_batch_whose_token_rows_are_no_multiple_of_8():
    """N = 36 and B = 1: the weight-gradient GEMMs would contract over 36 rows.  The training step says so before its first launch; inference takes any B."""
    import vitvq_oracle as O
    cfg = copy.deepcopy(O.TINY_CFG)
    cfg["image_size"] = 48
    P = O.make_params(cfg, seed=11)
    m = _build(cfg, P)
    x1 = O.make_images(5, 1, 48)
    with pytest.raises(ValueError, match=r"B \* N % 8 == 0.*B = 1.*N = 36"):
        m.training_step({"image": x1}, 0, 0)
    codes = m.encode_codes(x1)
    assert codes.shape == (1, 36)
    assert rel(m.decode_codes(codes), O.decode_codes(codes.cpu(), P, cfg)) <= ACT_TOL
    m.training_step({"image": O.make_images(5, 2, 48)}, 0, 0)      # B * N = 72
