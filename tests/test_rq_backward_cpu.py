"""The yardstick of the RQ prior's backward, checked without a GPU: the hand-written fp64 backward of tests/rq_backward_cases.py against autograd of
its own forward and against the REFERENCE's fp64 gradients (tests/golden/rq_bwd_<case>.npz, both code_sum modes), the emulation's rounding points, the
new entry points, the optimizer's parameter groups, the refusals of CondTransformer with an RQ prior off the device, and the new kernels' resources."""
import json
import os

import numpy as np
import pytest
import torch

import rq_backward_cases as BC
from util import floor16, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
_HAND = {}


def _params(name):
    from enhancing.modules.stage2.layers import RQTransformer
    m = RQTransformer(**BC.case_kwargs(name))
    return BC.make_params({k: tuple(v.shape) for k, v in m.state_dict().items()})


def _hand(name, mode):
    if (name, mode) not in _HAND:
        conds, codes = BC.case_inputs(name)
        _HAND[(name, mode)] = BC.loss_and_grads(_params(name), BC.case_dims(name), conds, codes, mode)
    return _HAND[(name, mode)]


@pytest.mark.parametrize("mode", BC.MODES)
@pytest.mark.parametrize("name", ["rq_tiny", "rq_d3", "rq_t2"])
def test_hand_written_backward_equals_autograd(name, mode):
    conds, codes = BC.case_inputs(name)
    loss, G, _ = _hand(name, mode)
    W = {k: v.double().requires_grad_(True) for k, v in _params(name).items()}
    _, loss_a, _ = BC.forward(W, BC.case_dims(name), conds, codes, mode)
    loss_a.backward()
    assert abs(loss.item() - loss_a.item()) <= 1e-12 * abs(loss_a.item())
    assert sorted(G) == sorted(W)
    for k in W:
        if k.endswith("attn.key.bias"):      # analytically zero: measured against its query twin
            assert (G[k] - W[k].grad).norm().item() <= 1e-9 * W[k.replace("key", "query")].grad.norm().item(), k
        else:
            assert rel(G[k].reshape(W[k].shape), W[k].grad) <= 1e-9, (k, rel(G[k].reshape(W[k].shape), W[k].grad))


@pytest.mark.parametrize("mode", BC.MODES)
@pytest.mark.parametrize("name", list(BC.CASES))
def test_hand_written_backward_equals_the_reference(name, mode):
    z = np.load(os.path.join(GOLD, f"rq_bwd_{name}.npz"))
    conds, codes = BC.case_inputs(name)
    assert np.array_equal(z["conds"], conds.numpy()) and np.array_equal(z["codes"], codes.numpy())
    loss, G, _ = _hand(name, mode)
    assert abs(loss.item() - float(z[f"loss64.{mode}"])) <= 1e-9 * abs(loss.item())
    names = sorted(str(k) for k in z["state_names"])
    assert names == sorted(G)
    close = lambda a, b, n: float(np.linalg.norm(a - b)) <= 1e-9 * n
    for i, k in enumerate(names):
        g = G[k].double()
        twin = G[k.replace("key", "query")].norm().item() if k.endswith("attn.key.bias") else None      # key.bias is analytically zero
        if f"g.{mode}.{k}" in z.files:
            ref = torch.from_numpy(z[f"g.{mode}.{k}"]).reshape(g.shape)
            err = (g - ref).norm().item() / (twin or ref.norm().item())
            assert err <= 1e-9, (k, err)
        else:
            n, gr, lg = BC.folded_projections(g, int(z["proj_seed"]) + i)
            n_ref = float(z[f"n.{mode}.{k}"])
            scale = twin or n_ref
            assert abs(n.item() - n_ref) <= 1e-9 * scale, k
            # a projection of G has the size of |G| times the norm of the random vector: that product is the scale of its error
            assert close(gr.numpy(), z[f"r.{mode}.{k}"], scale * np.sqrt(g.shape[-1])), k
            assert close(lg.numpy(), z[f"l.{mode}.{k}"], scale * np.sqrt(g.numel() // g.shape[-1])), k


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_emulation_is_finite_and_its_rounding_points_are_live(fmt):
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[fmt]
    scale = 1024.0 if fmt == "fp16" else 1.0
    conds, codes = BC.case_inputs("rq_tiny")
    _, G, _ = _hand("rq_tiny", "depth")
    loss, GE, _ = BC.loss_and_grads(_params("rq_tiny"), BC.case_dims("rq_tiny"), conds, codes, "depth", rnd=lambda t: t.to(dt).to(torch.float64), loss_scale=scale)
    assert bool(torch.isfinite(loss))
    for k in G:
        assert bool(torch.isfinite(GE[k]).all()), k
        if not k.endswith("attn.key.bias"):
            assert rel(GE[k] / scale, G[k]) > floor16(G[k], dt), (k, "the emulation equals fp64 to the format's floor: a rounding point is dead")


def test_new_entry_points_exist():
    from enhancing import _C
    from enhancing.modules.stage2.layers import RQTransformer
    for sym in ("enh_short_causal_attention_backward", "enh_ln_rows_strided_backward", "enh_rq_embed_seq_backward"):
        assert sym in _C.SIGNATURES, sym
    for fn in ("short_causal_attention_backward", "ln_rows_strided_backward", "rq_embed_seq_backward"):
        assert callable(getattr(_C, fn, None)), fn
    assert callable(getattr(RQTransformer, "forward_backward", None))
    m = RQTransformer(**BC.case_kwargs("rq_d3"))
    C, Hs, Hd, Ls, Ld, V, T, D, _ = BC.CASES["rq_d3"]
    assert m.saved_bytes_per_image() == Ls * T * (28 * C + 4 * Hs) + Ld * T * D * (28 * C + 4 * Hd)
    hdr = open(os.path.join(ROOT, "include", "enh_hip.h")).read()
    assert all(f"int {s}(" in hdr for s in ("enh_short_causal_attention_backward", "enh_ln_rows_strided_backward", "enh_rq_embed_seq_backward"))


def test_parameter_groups_are_the_references():
    from enhancing.engine.optim import gpt_param_groups
    from enhancing.modules.stage2.layers import RQTransformer
    with open(os.path.join(GOLD, "rq_optim_groups.json")) as f:
        gold = json.load(f)["rq_tiny"]
    decay, no_decay = gpt_param_groups(RQTransformer(**BC.case_kwargs("rq_tiny")))
    by_wd = {g["weight_decay"]: g["names"] for g in gold["groups"]}
    assert sorted(decay) == by_wd[0.01] and sorted(no_decay) == by_wd[0.0]
    assert gold["betas"] == [0.9, 0.96]


def _cpu_cond_transformer():
    from enhancing.modules.stage2.transformer import CondTransformer
    from enhancing.utils.general import AttrDict
    tower = dict(dim=128, depth=1, heads=2, mlp_dim=256)
    cfg = AttrDict.wrap(dict(
        cond=dict(target="enhancing.modules.cond.dummycond.ClassCond", params=dict(image_size=32, class_name=["a", "b", "c"])),
        stage1=dict(target="enhancing.modules.stage1.vitvqgan.ViTVQ",
                    params=dict(image_key="image", image_size=32, patch_size=8, encoder=tower, decoder=tower,
                                quantizer=dict(embed_dim=32, n_embed=64, use_residual=True, num_quantizers=4),
                                loss=dict(target="enhancing.losses.vqperceptual.DummyLoss"))),
        transformer=dict(target="enhancing.modules.stage2.layers.RQTransformer",
                         params=dict(vocab_cond_size=3, vocab_img_size=64, embed_dim=128, cond_num_tokens=1, img_num_tokens=16, depth_num_tokens=4,
                                     spatial_n_heads=2, depth_n_heads=2, spatial_n_layers=1, depth_n_layers=1))))
    return CondTransformer(cond_key="class", cond=cfg.cond, stage1=cfg.stage1, transformer=cfg.transformer)


def test_cpu_refusals_name_the_device():
    """with an RQ prior off the device: loss_and_grads, training_step and configure_optimizers refuse before anything is tokenized; sample stays unbuilt"""
    ct = _cpu_cond_transformer()
    called = []
    ct._tokenize = lambda batch: called.append(1)
    batch = {"image": torch.rand(2, 3, 32, 32), "class": torch.tensor([0, 2])}
    with pytest.raises(NotImplementedError, match="RQ prior's backward"):
        ct.loss_and_grads(batch)
    with pytest.raises(NotImplementedError, match="RQ training runs on a ROCm device only"):
        ct.training_step(batch, 0)
    ct.learning_rate = 1e-4
    with pytest.raises(NotImplementedError, match="RQ training runs on a ROCm device only"):
        ct.configure_optimizers()
    with pytest.raises(NotImplementedError, match="sampling"):
        ct.sample(torch.tensor([0, 2]))
    assert not called, "the batch was tokenized before the refusal"
    with pytest.raises(NotImplementedError, match="device"):
        ct.transformer.forward_backward(torch.zeros(2, 16, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="exact-f32 backward is not built"):
        ct.transformer.forward_backward(torch.zeros(2, 16, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), use_fp16=False)


RQ_BWD_LABELS = [f"rq_short_causal_bwd_kernel<{L}, {ot}>" for L in range(1, 9) for ot in ("F16", "BF16")] + \
                ["rq_ln_strided_bwd_kernel<F16>", "rq_ln_strided_bwd_kernel<BF16>", "rq_embed_seq_bwd_kernel"]


def test_rq_backward_labels_are_kernel_symbols_without_scratch():
    """every label the new launches report is exactly one kernel symbol of the shipped library; none of them uses scratch or spills"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    if not os.path.exists(isa_lint.DEFAULT_SO) or not os.path.exists(isa_lint.LLVM + "/llvm-objdump"):
        pytest.skip("needs the built library and the ROCm llvm tools")
    stats = isa_lint.kernel_stats()
    for label in RQ_BWD_LABELS:
        hits = [n for n in stats if n.startswith(label + "(") or n.startswith("void " + label + "(")]
        assert len(hits) == 1, (label, hits)
        s = stats[hits[0]]
        assert s.get("scratch_bytes", 0) == 0 and s.get("spills", 0) == 0 and s.get("scratch_ops", 0) == 0, (label, s)
