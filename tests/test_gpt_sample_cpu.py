"""Stage-2 GPT, host side: the module tree mirrors the reference's (names, shapes, init), the reference's own yaml resolves, the limits of the decode
kernels are ValueErrors, what is not built says so, and the plain-torch restatement of the cached sampling step that the GPU tests use as their
yardstick (tests/gpt_cases.py step_logits / host_filter) reproduces the reference's golden logits when stepped on the CPU."""
import math
import os

import numpy as np
import pytest
import torch

import gpt_cases as GC
from enhancing.modules.stage2.layers import GPT
from enhancing.modules.stage2.transformer import CondTransformer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"gpt_{name}.npz"))


@pytest.mark.parametrize("name", list(GC.CASES))
def test_state_dict_names_and_shapes_equal_the_reference(golden_dir, name):
    g = _golden(golden_dir, name)
    sd = GPT(**GC.case_kwargs(name)).state_dict()
    assert sorted(sd) == list(g["state_names"])
    for k, shp in zip(g["state_names"], g["state_shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(v) for v in shp if v), k
    assert not any("mask" in k for k in sd)


def test_init_statistics_and_time_mix_ramp():
    torch.manual_seed(0)
    m = GPT(vocab_cond_size=10, vocab_img_size=512, embed_dim=256, cond_num_tokens=1, img_num_tokens=16, n_heads=4, n_layers=2)
    for n, p in m.named_parameters():
        if n.startswith("pos_emb") or n.endswith("bias"):
            assert not p.any(), n
        elif ".ln" in n or n.startswith("layer_norm"):
            assert bool((p == 1).all()), n
        elif n.endswith("time_mix"):
            assert tuple(p.shape) == (1, 1, 256)
            assert torch.allclose(p.view(-1), torch.arange(256, dtype=torch.float32) / 255, atol=1e-7)
        else:      # Linear / Embedding weights: normal(0, 0.02); 3 sigma of the sample std and mean
            n_el = p.numel()
            assert abs(p.std().item() - 0.02) < 3 * 0.02 / math.sqrt(2 * n_el) + 1e-5, n
            assert abs(p.mean().item()) < 4 * 0.02 / math.sqrt(n_el), n


def test_reference_yaml_resolves_its_targets():
    """the reference's own configs/imagenet_gpt_vitvq_base.yaml (a verbatim copy): the three targets resolve; the 10.9 G-weight model is not instantiated"""
    from enhancing.modules.cond.dummycond import ClassCond
    from enhancing.utils.general import get_config_from_file, get_obj_from_str
    for path in (os.path.join(ROOT, "tests", "golden", "reference_configs", "imagenet_gpt_vitvq_base.yaml"), os.path.join(ROOT, "configs", "imagenet_gpt_vitvq_base.yaml")):
        cfg = get_config_from_file(path)
        assert get_obj_from_str(cfg.model.target) is CondTransformer
        assert get_obj_from_str(cfg.model.params.cond.target) is ClassCond
        assert get_obj_from_str(cfg.model.params.transformer.target) is GPT
        tp = cfg.model.params.transformer.params
        assert (tp.embed_dim, tp.n_heads, tp.n_layers, tp.vocab_img_size, tp.img_num_tokens, tp.cond_num_tokens) == (6144, 16, 24, 8192, 1024, 1)
        assert tp.embed_dim // tp.n_heads == 384
    c = ClassCond(image_size=256, class_name="assets/class/imagenet.txt")
    x = torch.arange(3)
    assert c.encode_codes(x) is x


@pytest.mark.parametrize("kw, word", [(dict(cond_num_tokens=2), "cond_num_tokens"), (dict(embed_dim=96, n_heads=2), "head size"),
                                      (dict(embed_dim=1024, n_heads=2), "384"), (dict(vocab_img_size=16385), "16384"),
                                      (dict(embed_dim=8448, n_heads=33, n_layers=0), "8192"), (dict(vocab_img_size=1004), "multiple of 8"),
                                      (dict(img_num_tokens=8193, n_layers=0), "img_num_tokens")])
def test_refused_shapes_are_value_errors(kw, word):
    base = dict(vocab_cond_size=10, vocab_img_size=512, embed_dim=128, cond_num_tokens=1, img_num_tokens=4, n_heads=2, n_layers=1)
    base.update(kw)
    with pytest.raises(ValueError, match=word):
        GPT(**base)


def test_unbuilt_parts_say_so():
    m = GPT(**GC.case_kwargs("tiny"))
    with pytest.raises(NotImplementedError, match="forward"):
        m(torch.zeros(1, 20, dtype=torch.long), torch.zeros(1, 1, dtype=torch.long))
    ct = CondTransformer.__new__(CondTransformer)
    with pytest.raises(NotImplementedError, match="training"):
        ct.training_step({}, 0)
    with pytest.raises(NotImplementedError, match="training"):
        ct.configure_optimizers()
    with pytest.raises(RuntimeError, match="device"):
        m.sample(torch.zeros(1, 1, dtype=torch.long))


@pytest.mark.parametrize("name", list(GC.CASES))
def test_host_restatement_reproduces_the_golden_logits(golden_dir, name):
    """the yardstick's own check: the T == 1 restatement (time_shift term zero) in plain fp32 torch is the reference's cached sample() to fp32 accuracy:
    within 4x the fp32 reference module's own error against fp64 (another summation order of the same fp32 arithmetic) + 1e-6"""
    g = _golden(golden_dir, name)
    m = GPT(**GC.case_kwargs(name))
    P = GC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})
    conds, forced = GC.make_inputs(name)
    assert np.array_equal(conds.numpy(), g["conds"]) and np.array_equal(forced.numpy(), g["forced_codes"])
    lg = GC.step_logits(P, name, conds, forced, prod=torch.float32)
    err = (lg.double() - torch.from_numpy(g["logits64"])).abs().max().item()
    assert err <= 4 * float(g["ref32_err"]) + 1e-6, (err, float(g["ref32_err"]))


def test_host_filter_is_the_reference_filter():
    """host_filter on known rows: top-k keeps ties, top-p drops an entry when the mass in front of it reaches top_p, the first entry always stays"""
    x = torch.tensor([[2.0, 1.0, 1.0, 0.0, -1.0]], dtype=torch.float64)
    lg, keep, pr = GC.host_filter(x, top_k=2)
    assert keep.tolist() == [[True, True, True, False, False]] and torch.isinf(lg[0, 3])
    _, keep, pr = GC.host_filter(torch.log(torch.tensor([[0.5, 0.3, 0.15, 0.05]], dtype=torch.float64)), top_p=0.7)
    assert keep.tolist() == [[True, True, False, False]] and abs(pr[0, 0].item() - 0.625) < 1e-12
    _, keep, _ = GC.host_filter(torch.log(torch.tensor([[0.9, 0.1]], dtype=torch.float64)), top_p=0.5)
    assert keep.tolist() == [[True, False]]
    assert GC.inverse_cdf(torch.tensor([[0.25, 0.0, 0.75]], dtype=torch.float64), torch.tensor([0.25])).tolist() == [2]
    assert GC.inverse_cdf(torch.tensor([[0.25, 0.0, 0.75]], dtype=torch.float64), torch.tensor([0.2])).tolist() == [0]
