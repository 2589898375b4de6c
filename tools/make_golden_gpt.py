"""Writes tests/golden/gpt_tiny.npz, gpt_hs384.npz and gpt_h3.npz: the REFERENCE's own stage-2 GPT (enhancing/modules/stage2/layers.py, loaded by
file path) on the cases of tests/gpt_cases.py.  Run once where the reference tree is available (ENH_REFERENCE_ROOT):  python tools/make_golden_gpt.py

The reference's cached sampling loop (GPT.sample lines 222-240: sample_step + the growing `past`) is stepped with FORCED codes in place of the
multinomial draws, without top-k / top-p.  The files hold data only: the condition ids, the forced codes, the logits of a .double() copy of the module,
the fp32 module's max error against them (whole run and per step), and the state-dict names / shapes."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpt_cases as GC  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("ENH_REFERENCE_ROOT", "")
torch.set_num_threads(8)


def load_reference_layers():
    if "omegaconf" not in sys.modules:      # imported by the reference file and never used
        stub = types.ModuleType("omegaconf")
        stub.OmegaConf = object
        sys.modules["omegaconf"] = stub
    spec = importlib.util.spec_from_file_location("_ref_stage2_layers", os.path.join(REF, "enhancing", "modules", "stage2", "layers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def forced_sample(gpt, conds, forced):
    """GPT.sample's loop with `forced` in place of the draws: logits [B, T, V]"""
    past, out = None, []
    with torch.no_grad():
        for i in range(gpt.img_num_tokens):
            codes_ = None if i == 0 else forced[:, i - 1:i]
            pos_code = None if i == 0 else gpt.pos_emb_code[:, i - 1:i, :]
            logits_, presents = gpt.sample_step(codes_, conds, pos_code, False, past)
            presents = torch.stack(presents).clone().detach()
            past = [presents] if past is None else past + [presents]
            out.append(logits_)
    return torch.stack(out, 1)


def gold(name: str) -> None:
    L = load_reference_layers()
    torch.manual_seed(0)
    gpt = L.GPT(**GC.case_kwargs(name)).eval()
    shapes = {k: tuple(v.shape) for k, v in gpt.state_dict().items()}
    gpt.load_state_dict(GC.make_params(shapes), strict=True)
    conds, forced = GC.make_inputs(name)
    l32 = forced_sample(gpt, conds, forced)
    l64 = forced_sample(gpt.double(), conds, forced)
    err_step = (l32.double() - l64).abs().amax(dim=(0, 2)).numpy()
    state_names = sorted(shapes)
    state_shapes = np.zeros((len(state_names), 4), dtype=np.int64)
    for i, k in enumerate(state_names):
        state_shapes[i, :len(shapes[k])] = shapes[k]
    path = os.path.join(GOLD, f"gpt_{name}.npz")
    np.savez_compressed(path, param_seed=GC.PARAM_SEED, conds=conds.numpy(), forced_codes=forced.numpy().astype(np.int32), logits64=l64.numpy(),
                        ref32_err=float(err_step.max()), ref32_err_step=err_step, state_names=np.array(state_names), state_shapes=state_shapes)
    limit = os.path.getsize(os.path.join(GOLD, "vit_tiny.npz"))
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): logits rms {l64.pow(2).mean().sqrt().item():.3f}, "
          f"fp32 reference max error {err_step.max():.3e}")


if __name__ == "__main__":
    assert REF and os.path.isdir(REF), "needs the reference tree: set ENH_REFERENCE_ROOT"
    for name in GC.CASES:
        gold(name)
