"""Writes tests/golden/gpt_bwd_<case>.npz for the cases of tests/gpt_backward_cases.py: the REFERENCE's own stage-2 GPT
(enhancing/modules/stage2/layers.py, loaded by file path as tools/make_golden_gpt.py does) as a .double() module, its teacher-forced forward and
F.cross_entropy(logits.view(-1, V), codes.view(-1)).backward().  Run once where the reference tree is available (ENH_REFERENCE_ROOT):
    python tools/make_golden_gpt_backward.py

The files hold data only: the condition ids and codes, the fp64 loss, and for every state-dict parameter `g.<name>` = its whole fp64 gradient when
it has at most 4096 elements, else `n.<name>` (Frobenius norm), `r.<name>` = G r and `l.<name>` = l G of the gradient seen as a matrix
[-1, last axis], with r and l drawn from `proj_seed` + the parameter's index in sorted order (gpt_backward_cases.projections)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpt_backward_cases as BC  # noqa: E402
from make_golden_gpt import GOLD, REF, load_reference_layers  # noqa: E402

PROJ_SEED = 1234


def gold(name: str) -> None:
    L = load_reference_layers()
    torch.manual_seed(0)
    gpt = L.GPT(**BC.case_kwargs(name)).eval()
    shapes = {k: tuple(v.shape) for k, v in gpt.state_dict().items()}
    gpt.load_state_dict(BC.make_params(shapes), strict=True)
    gpt = gpt.double()
    conds, codes = BC.case_inputs(name)
    logits = gpt(codes, conds)
    V = logits.shape[-1]
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), codes.reshape(-1))
    loss.backward()
    grads = {k: p.grad for k, p in gpt.named_parameters()}
    assert sorted(grads) == sorted(shapes), "a state-dict entry without a gradient"
    out = dict(param_seed=BC.PARAM_SEED, proj_seed=PROJ_SEED, conds=conds.numpy(), codes=codes.numpy().astype(np.int32), loss64=loss.item(),
               state_names=np.array(sorted(shapes)))
    for i, k in enumerate(sorted(shapes)):
        G = grads[k].detach()
        if G.numel() <= BC.FULL_LIMIT:
            out["g." + k] = G.numpy()
        else:
            n, gr, lg = BC.projections(G, PROJ_SEED + i)
            out["n." + k], out["r." + k], out["l." + k] = float(n), gr.numpy(), lg.numpy()
    path = os.path.join(GOLD, f"gpt_bwd_{name}.npz")
    np.savez_compressed(path, **out)
    limit = os.path.getsize(os.path.join(GOLD, "vit_tiny.npz"))
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    kb, qb = grads["blocks.0.attn.key.bias"].norm().item(), grads["blocks.0.attn.query.bias"].norm().item()
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): loss {loss.item():.4f}, |d key.bias| / |d query.bias| = {kb / qb:.2e}")


if __name__ == "__main__":
    assert REF and os.path.isdir(REF), "needs the reference tree: set ENH_REFERENCE_ROOT"
    for name in BC.CASES:
        gold(name)
