"""Writes tests/golden/gpt_fwd_<case>.npz for the cases of tests/gpt_forward_cases.py: the REFERENCE's own stage-2 GPT.forward
(enhancing/modules/stage2/layers.py:193-211, loaded by file path as tools/make_golden_gpt.py does).  Run once where the reference tree is available
(ENH_REFERENCE_ROOT):  python tools/make_golden_gpt_forward.py

The files hold data only: the condition ids and codes, `logits64` of a .double() copy of the module, `nll64` = the per-position cross-entropy of
logits64 against the codes, `ref32_err` = the fp32 module's max error against logits64, and the state-dict names / shapes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpt_forward_cases as FC  # noqa: E402
from make_golden_gpt import GOLD, REF, load_reference_layers  # noqa: E402


def gold(name: str) -> None:
    L = load_reference_layers()
    torch.manual_seed(0)
    gpt = L.GPT(**FC.case_kwargs(name)).eval()
    shapes = {k: tuple(v.shape) for k, v in gpt.state_dict().items()}
    gpt.load_state_dict(FC.make_params(shapes), strict=True)
    conds, codes = FC.case_inputs(name)
    with torch.no_grad():
        l32 = gpt(codes, conds)
        l64 = gpt.double()(codes, conds)
    V = l64.shape[-1]
    nll64 = torch.nn.functional.cross_entropy(l64.reshape(-1, V), codes.reshape(-1), reduction="none").view(codes.shape)
    state_names = sorted(shapes)
    state_shapes = np.zeros((len(state_names), 4), dtype=np.int64)
    for i, k in enumerate(state_names):
        state_shapes[i, :len(shapes[k])] = shapes[k]
    path = os.path.join(GOLD, f"gpt_fwd_{name}.npz")
    np.savez_compressed(path, param_seed=FC.PARAM_SEED, conds=conds.numpy(), codes=codes.numpy().astype(np.int32), logits64=l64.numpy(),
                        nll64=nll64.numpy(), ref32_err=float((l32.double() - l64).abs().max()), state_names=np.array(state_names),
                        state_shapes=state_shapes)
    limit = os.path.getsize(os.path.join(GOLD, "vit_tiny.npz"))
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): logits rms {l64.pow(2).mean().sqrt().item():.3f}, "
          f"fp32 reference max error {float((l32.double() - l64).abs().max()):.3e}, mean nll {nll64.mean().item():.4f}")


if __name__ == "__main__":
    assert REF and os.path.isdir(REF), "needs the reference tree: set ENH_REFERENCE_ROOT"
    for name in FC.CASES:
        gold(name)
