"""Writes tests/golden/gpt_optim_groups.json and tests/golden/gpt_train_tiny.npz: the REFERENCE's own stage-2 optimizer
(enhancing/modules/stage2/transformer.py CondTransformer.configure_optimizers, loaded by file path beside the reference's GPT) on the cases of
tests/gpt_backward_cases.py.  Run once where the reference tree is available (ENH_REFERENCE_ROOT):
    python tools/make_golden_gpt_train.py

gpt_optim_groups.json: for the `tiny` and `h3` shapes, the sorted parameter names of the two groups that configure_optimizers hands to
torch.optim.Adam, each group's weight_decay, and the optimizer's lr-independent defaults (betas, eps).

gpt_train_tiny.npz: the reference GPT as a .double() module on the `tiny` case's batch, stepped STEPS times by that optimizer at lr LR (loss =
F.cross_entropy of the teacher-forced logits, as the reference's shared_step): the loss before every step and the final parameters, a tensor of at
most 4096 elements whole (`p.<name>`), a larger one as its Frobenius norm and two projections (`n.`, `r.`, `l.`: gpt_backward_cases.projections, seeds
PROJ_SEED + the parameter's index in sorted order) of the CHANGE final - initial, which is what three steps at this lr leave to compare.

The files hold data only.  configure_optimizers is called on a stand-in object with the three attributes it reads (transformer, learning_rate,
scheduler): the reference's class derives from pytorch_lightning.LightningModule, which is stubbed by torch.nn.Module for the import."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpt_backward_cases as BC  # noqa: E402
from make_golden_gpt import GOLD, REF, load_reference_layers  # noqa: E402

PROJ_SEED = 4321
STEPS = 3
LR = 1e-3
GROUP_CASES = ("tiny", "h3")


def load_reference_transformer(layers):
    """the reference's stage2/transformer.py as a module of a stand-in package: `.layers` is the reference's own file, `...utils.general` and
    pytorch_lightning are stubs (configure_optimizers uses neither)"""
    for name in ("_refpkg", "_refpkg.modules", "_refpkg.modules.stage2", "_refpkg.utils"):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = []
            sys.modules[name] = pkg
    sys.modules["_refpkg.modules.stage2.layers"] = layers
    general = types.ModuleType("_refpkg.utils.general")
    general.initialize_from_config = lambda cfg: None
    sys.modules["_refpkg.utils.general"] = general
    if "pytorch_lightning" not in sys.modules:
        pl = types.ModuleType("pytorch_lightning")
        pl.LightningModule = torch.nn.Module
        sys.modules["pytorch_lightning"] = pl
    spec = importlib.util.spec_from_file_location("_refpkg.modules.stage2.transformer", os.path.join(REF, "enhancing", "modules", "stage2", "transformer.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def reference_optimizer(T, gpt, lr: float):
    stand_in = types.SimpleNamespace(transformer=gpt, learning_rate=lr, scheduler=None)
    opts, scheds = T.CondTransformer.configure_optimizers(stand_in)
    assert len(opts) == 1 and scheds == [] and type(opts[0]) is torch.optim.Adam
    return opts[0]


def reference_gpt(L, name: str):
    torch.manual_seed(0)
    gpt = L.GPT(**BC.case_kwargs(name)).eval()
    shapes = {k: tuple(v.shape) for k, v in gpt.state_dict().items()}
    gpt.load_state_dict(BC.make_params(shapes), strict=True)
    return gpt, shapes


def groups(L, T) -> None:
    out = {}
    for name in GROUP_CASES:
        gpt, _ = reference_gpt(L, name)
        opt = reference_optimizer(T, gpt, LR)
        names = {id(p): k for k, p in gpt.named_parameters()}
        assert len(opt.param_groups) == 2
        d = opt.defaults
        assert not d["amsgrad"] and not d.get("maximize", False)
        out[name] = dict(betas=list(opt.param_groups[0]["betas"]), eps=opt.param_groups[0]["eps"],
                         groups=[dict(weight_decay=g["weight_decay"], names=sorted(names[id(p)] for p in g["params"])) for g in opt.param_groups])
        print(f"  {name}: {[(g['weight_decay'], len(g['names'])) for g in out[name]['groups']]} betas {out[name]['betas']} eps {out[name]['eps']}")
    with open(os.path.join(GOLD, "gpt_optim_groups.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def trajectory(L, T, name: str = "tiny") -> None:
    gpt, shapes = reference_gpt(L, name)
    gpt = gpt.double()
    start = {k: v.detach().clone() for k, v in gpt.state_dict().items()}
    opt = reference_optimizer(T, gpt, LR)
    conds, codes = BC.case_inputs(name)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad()
        logits = gpt(codes, conds)
        loss = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[-1]), codes.reshape(-1))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out = dict(param_seed=BC.PARAM_SEED, proj_seed=PROJ_SEED, steps=STEPS, lr=LR, conds=conds.numpy(), codes=codes.numpy().astype(np.int32),
               loss64=np.array(losses), state_names=np.array(sorted(shapes)))
    final = gpt.state_dict()
    for i, k in enumerate(sorted(shapes)):
        P = final[k].detach()
        if P.numel() <= BC.FULL_LIMIT:
            out["p." + k] = P.numpy()
        else:
            n, gr, lg = BC.projections(P - start[k], PROJ_SEED + i)
            out["n." + k], out["r." + k], out["l." + k] = float(n), gr.numpy(), lg.numpy()
    path = os.path.join(GOLD, f"gpt_train_{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 250_000, (path, os.path.getsize(path))
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): losses {losses}")


if __name__ == "__main__":
    assert REF and os.path.isdir(REF), "needs the reference tree: set ENH_REFERENCE_ROOT"
    L = load_reference_layers()
    T = load_reference_transformer(L)
    groups(L, T)
    trajectory(L, T)
