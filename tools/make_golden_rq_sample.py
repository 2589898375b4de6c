"""Writes tests/golden/rq_sample_<case>.npz for the cases of tests/rq_sample_cases.py from the REFERENCE's own stage-2 RQTransformer
(enhancing/modules/stage2/layers.py:397-547, loaded by file path as tools/make_golden_gpt.py does).  Run once where the reference tree is available
(ENH_REFERENCE_ROOT):  python tools/make_golden_rq_sample.py

The reference's cached sampling loop (RQTransformer.sample: sample_spatial_step / sample_depth_step with the growing `past` lists) is stepped with
FORCED codes in place of the multinomial draws, without top-k / top-p, use_fp16=False.  Two goldens per case.  `logits64_twice` is that loop on a
.double() copy of the module: its sample_depth_step applies ln_depth to depth slot 0 twice (once in the `codes is None` branch, once in the common
line behind it).  `logits64_once` is the same loop with the depth step composed here from the reference's own submodules (depth_transformer's
Block.sample, ln_depth, head) with ONE ln_depth at every slot, which is what the teacher-forced forward, so training, computes.  The files hold data
only: the ids, the two logits [B T, D, V], `ref32_err_*` = the fp32 module's max error against its fp64 self (whole run, and per (t, d) as
`ref32_err_*_step` [T, D]), and the state-dict names / shapes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rq_sample_cases as SC  # noqa: E402
from make_golden_gpt import GOLD, REF, load_reference_layers  # noqa: E402


def depth_step_once(m, codes_, hidden, pos_depth, past):
    """sample_depth_step with one ln_depth at every slot, on the module's own submodules: (logits [B, V], presents)"""
    presents = []
    if codes_ is None:
        x, past = hidden, [None] * len(m.depth_transformer)
    else:
        x = m.tok_emb_code(codes_).sum(1, keepdim=True) + pos_depth
        past = torch.cat(past, dim=-2)
    for i, block in enumerate(m.depth_transformer):
        x, present = block.sample(x, layer_past=past[i])
        presents.append(present)
    return m.head(m.ln_depth(x)[:, -1].contiguous()), presents


def forced_sample(m, conds, forced, once: bool):
    """RQTransformer.sample's loop with `forced` [B, T, D] in place of the draws: logits [B T, D, V]"""
    B, T, D = forced.shape
    flat = forced.reshape(B, T * D)
    past, out = None, []
    with torch.no_grad():
        for i in range(T):
            codes_ = None if i == 0 else flat[:, (i - 1) * D:i * D]
            pos_code = None if i == 0 else m.pos_emb_code[:, i - 1:i, :]
            hidden, presents = m.sample_spatial_step(codes_, conds, pos_code, False, past)
            presents = torch.stack(presents).clone().detach()
            past = [presents] if past is None else past + [presents]
            depth_past = None
            for d in range(D):
                codes_ = None if d == 0 else flat[:, i * D:i * D + d]
                pos_depth = None if d == 0 else m.pos_emb_depth[:, d - 1:d, :]
                if once:
                    logits_, depth_presents = depth_step_once(m, codes_, hidden, pos_depth, depth_past)
                else:
                    logits_, depth_presents = m.sample_depth_step(codes_, hidden, pos_depth, False, depth_past)
                depth_presents = torch.stack(depth_presents).clone().detach()
                depth_past = [depth_presents] if depth_past is None else depth_past + [depth_presents]
                out.append(logits_)
    return torch.stack(out, 1).view(B * T, D, -1)


def gold(name: str) -> None:
    L = load_reference_layers()
    torch.manual_seed(0)
    m = L.RQTransformer(**SC.case_kwargs(name)).eval()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(SC.make_params(shapes), strict=True)
    conds, forced = SC.case_inputs(name)
    B, T, D = forced.shape
    o32, t32 = forced_sample(m, conds, forced, True), forced_sample(m, conds, forced, False)
    m = m.double()
    o64, t64 = forced_sample(m, conds, forced, True), forced_sample(m, conds, forced, False)
    step = lambda a, b: (a.double() - b).abs().view(B, T, D, -1).amax(dim=(0, 3)).numpy()
    eo, et = step(o32, o64), step(t32, t64)
    state_names = sorted(shapes)
    state_shapes = np.zeros((len(state_names), 4), dtype=np.int64)
    for i, k in enumerate(state_names):
        state_shapes[i, :len(shapes[k])] = shapes[k]
    path = os.path.join(GOLD, f"rq_sample_{name}.npz")
    np.savez_compressed(path, param_seed=SC.PARAM_SEED, conds=conds.numpy(), forced_codes=forced.numpy().astype(np.int32), logits64_once=o64.numpy(),
                        logits64_twice=t64.numpy(), ref32_err_once=float(eo.max()), ref32_err_twice=float(et.max()), ref32_err_once_step=eo,
                        ref32_err_twice_step=et, state_names=np.array(state_names), state_shapes=state_shapes)
    limit = os.path.getsize(os.path.join(GOLD, "vit_tiny.npz"))
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): logits rms {o64.pow(2).mean().sqrt().item():.3f} (once) "
          f"{t64.pow(2).mean().sqrt().item():.3f} (twice), the two differ by {float((o64 - t64).abs().max()):.3f}, fp32 reference max error "
          f"{eo.max():.3e} / {et.max():.3e}")


if __name__ == "__main__":
    assert REF and os.path.isdir(REF), "needs the reference tree: set ENH_REFERENCE_ROOT"
    for name in SC.CASES:
        gold(name)
