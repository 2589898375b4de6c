"""Writes tests/golden/rq_fwd_<case>.npz for the cases of tests/rq_cases.py from the REFERENCE's own stage-2 RQTransformer
(enhancing/modules/stage2/layers.py:306-395, loaded by file path as tools/make_golden_gpt.py does).  Run once where the reference tree is available
(ENH_REFERENCE_ROOT):  python tools/make_golden_rq_forward.py

Two goldens per case.  `logits64_channels` is the reference's own `forward` on a .double() copy of the module: its `codes.cumsum(-1)` runs along the
embedding channels.  `logits64_depth` is the reference's own submodules (tok_emb_*, spatial_transformer, ln_spatial, depth_transformer, ln_depth,
head) composed here with the running sum over DEPTH, which is what the reference's sampler (`codes.sum(1)`) assumes.  The files hold data only: the
ids, the two logits, `nll64_*` = their cross-entropy against the codes, `ref32_err_*` = the fp32 module's max error against its fp64 self, and the
state-dict names / shapes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rq_cases as RC  # noqa: E402
from make_golden_gpt import GOLD, REF, load_reference_layers  # noqa: E402


def depth_forward(m, codes, conds):
    """RQTransformer.forward with `cumsum` along depth instead of along the channels, on the module's own submodules"""
    emb = m.tok_emb_code(codes.view(codes.shape[0], -1, codes.shape[-1]))          # [B, T, D, C]
    cs = emb.cumsum(2)
    c = m.tok_emb_cond(conds) + m.pos_emb_cond
    h = torch.cat([c, cs[:, :, -1] + m.pos_emb_code], 1).contiguous()
    h = m.ln_spatial(m.spatial_transformer(h))[:, c.shape[1] - 1:-1].contiguous()
    v = torch.cat([h.unsqueeze(2), cs[:, :, :-1] + m.pos_emb_depth], 2).contiguous()
    v = m.depth_transformer(v.view(-1, *v.shape[2:]))
    return m.head(m.ln_depth(v))


def gold(name: str) -> None:
    L = load_reference_layers()
    torch.manual_seed(0)
    m = L.RQTransformer(**RC.case_kwargs(name)).eval()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(RC.make_params(shapes), strict=True)
    conds, codes = RC.case_inputs(name)
    with torch.no_grad():
        c32, d32 = m(codes, conds), depth_forward(m, codes, conds)
        m = m.double()
        c64, d64 = m(codes, conds), depth_forward(m, codes, conds)
    V = c64.shape[-1]
    nll = lambda l: torch.nn.functional.cross_entropy(l.reshape(-1, V), codes.reshape(-1), reduction="none").view(-1, codes.shape[-1])
    err = lambda a, b: float((a.double() - b).abs().max())
    state_names = sorted(shapes)
    state_shapes = np.zeros((len(state_names), 4), dtype=np.int64)
    for i, k in enumerate(state_names):
        state_shapes[i, :len(shapes[k])] = shapes[k]
    path = os.path.join(GOLD, f"rq_fwd_{name}.npz")
    np.savez_compressed(path, param_seed=RC.PARAM_SEED, conds=conds.numpy(), codes=codes.numpy().astype(np.int32), logits64_channels=c64.numpy(),
                        logits64_depth=d64.numpy(), nll64_channels=nll(c64).numpy(), nll64_depth=nll(d64).numpy(), ref32_err_channels=err(c32, c64),
                        ref32_err_depth=err(d32, d64), state_names=np.array(state_names), state_shapes=state_shapes)
    limit = os.path.getsize(os.path.join(GOLD, "vit_tiny.npz"))
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): logits rms {c64.pow(2).mean().sqrt().item():.3f} (channels) "
          f"{d64.pow(2).mean().sqrt().item():.3f} (depth), the two differ by {err(c64, d64):.3f}, fp32 reference max error {err(c32, c64):.3e} / "
          f"{err(d32, d64):.3e}, mean nll {nll(c64).mean().item():.4f} / {nll(d64).mean().item():.4f}")


if __name__ == "__main__":
    assert REF and os.path.isdir(REF), "needs the reference tree: set ENH_REFERENCE_ROOT"
    for name in RC.CASES:
        gold(name)
