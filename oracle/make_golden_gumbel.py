"""Pins GumbelQuantizer against the REAL reference and writes tests/golden/gumbel.npz.

Run next to a checkout of the reference (located by oracle/_reference_loader.py):  python oracle/make_golden_gumbel.py
Runs the reference's own GumbelQuantizer (quantizers.py:95-126 + the residual loop of BaseQuantizer.forward) under the seeds of
tests/test_host_cpu.py::test_gumbel_quantizer_equals_the_reference_class, single-stage and residual, in training (soft) and eval (hard)
mode, and stores its embedding, input, outputs and gradients (under 100 KB).
TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def run(Q, residual):
    """Q.GumbelQuantizer (the reference's module or this package's): construction under seed 3, then per mode (train = soft, eval = hard) under
    seed 11 the outputs and the gradients of zq.pow(2).sum() + loss w.r.t. z and the embedding.  Returns (quantizer, {name: tensor or None})."""
    kw = dict(embed_dim=32, n_embed=64, temp_init=0.7, use_residual=residual, num_quantizers=3 if residual else None)
    torch.manual_seed(3)
    q = Q.GumbelQuantizer(**kw)
    z = torch.randn(2, 16, 32, requires_grad=True)
    out = {"embedding": q.embedding.weight.detach().clone(), "z": z.detach().clone()}
    for mode in ("train", "eval"):
        q.train(mode == "train")
        torch.manual_seed(11)
        zq, loss, idx = q(z)
        gz, ge = torch.autograd.grad(zq.pow(2).sum() + loss, [z, q.embedding.weight], allow_unused=True)
        out.update({f"{mode}_zq": zq.detach(), f"{mode}_loss": loss.detach(), f"{mode}_idx": idx, f"{mode}_gz": gz, f"{mode}_ge": ge})
    return q, out


if __name__ == "__main__":
    import _reference_loader as RL
    Q = RL.load_quantizers()
    gold = {}
    for residual in (False, True):
        tag = "rq" if residual else "vq"
        for k, v in run(Q, residual)[1].items():
            gold[f"{tag}_{k}_is_none"] = np.array(v is None)
            gold[f"{tag}_{k}"] = np.zeros(0, np.float32) if v is None else v.numpy()
    path = os.path.join(os.path.dirname(HERE), "tests", "golden", "gumbel.npz")
    np.savez_compressed(path, **gold)
    print("wrote", path, {k: v.shape for k, v in gold.items() if not k.endswith("_is_none")})
