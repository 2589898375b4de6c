"""Writes tests/golden/rq_bwd_<case>.npz for the cases of tests/rq_backward_cases.py: the REFERENCE's own stage-2 RQTransformer
(enhancing/modules/stage2/layers.py, loaded by file path as tools/make_golden_gpt.py does) as a .double() module and
F.cross_entropy(logits.view(-1, V), codes.view(-1)).backward(), once through the reference's own `forward` (mode "channels": its cumsum runs along
the embedding channels) and once through make_golden_rq_forward.depth_forward (mode "depth": the module's own submodules with the running sum over
depth).  Run once where the reference tree is available (ENH_REFERENCE_ROOT):
    python tools/make_golden_rq_backward.py

The files hold data only: the condition ids and codes, and per mode the fp64 loss `loss64.<mode>` and for every state-dict parameter
`g.<mode>.<name>` = its whole fp64 gradient when it has at most 4096 elements, else `n.<mode>.<name>` (Frobenius norm), `r.<mode>.<name>` = G r and
`l.<mode>.<name>` = l G of the gradient seen as a matrix [-1, last axis], each folded to 64 sums when longer than 256 (so that two modes of a 384-wide
model fit the size rule), with r and l drawn from `proj_seed` + the parameter's index in sorted order (rq_backward_cases.folded_projections).

Also writes tests/golden/rq_optim_groups.json the way tools/make_golden_gpt_train.py writes gpt_optim_groups.json: for the `rq_tiny` shape, the sorted
parameter names of the two groups that the reference's CondTransformer.configure_optimizers hands to torch.optim.Adam, each group's weight_decay, and
the optimizer's betas and eps."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rq_backward_cases as BC  # noqa: E402
from make_golden_gpt import GOLD, REF, load_reference_layers  # noqa: E402
from make_golden_gpt_train import LR, load_reference_transformer, reference_optimizer  # noqa: E402
from make_golden_rq_forward import depth_forward  # noqa: E402

PROJ_SEED = 1234


def gold(name: str) -> None:
    L = load_reference_layers()
    conds, codes = BC.case_inputs(name)
    out = dict(param_seed=BC.PARAM_SEED, proj_seed=PROJ_SEED, conds=conds.numpy(), codes=codes.numpy().astype(np.int32))
    note = []
    for mode in BC.MODES:
        torch.manual_seed(0)
        m = L.RQTransformer(**BC.case_kwargs(name)).eval()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict(BC.make_params(shapes), strict=True)
        m = m.double()
        logits = m(codes, conds) if mode == "channels" else depth_forward(m, codes, conds)
        V = logits.shape[-1]
        loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), codes.reshape(-1))
        loss.backward()
        grads = {k: p.grad for k, p in m.named_parameters()}
        assert sorted(grads) == sorted(shapes) and all(g is not None for g in grads.values()), "a state-dict entry without a gradient"
        out["state_names"] = np.array(sorted(shapes))
        out[f"loss64.{mode}"] = loss.item()
        for i, k in enumerate(sorted(shapes)):
            G = grads[k].detach()
            if G.numel() <= BC.WHOLE_LIMIT:
                out[f"g.{mode}.{k}"] = G.numpy()
            else:
                n, gr, lg = BC.folded_projections(G, PROJ_SEED + i)
                out[f"n.{mode}.{k}"], out[f"r.{mode}.{k}"], out[f"l.{mode}.{k}"] = float(n), gr.numpy(), lg.numpy()
        note.append(f"{mode}: loss {loss.item():.4f}")
    path = os.path.join(GOLD, f"rq_bwd_{name}.npz")
    np.savez_compressed(path, **out)
    limit = os.path.getsize(os.path.join(GOLD, "vit_tiny.npz"))
    assert os.path.getsize(path) <= limit, (path, os.path.getsize(path), limit)
    print(f"  wrote {os.path.basename(path)} ({os.path.getsize(path)} bytes): " + ", ".join(note))


def groups(name: str = "rq_tiny") -> None:
    L = load_reference_layers()
    T = load_reference_transformer(L)
    torch.manual_seed(0)
    m = L.RQTransformer(**BC.case_kwargs(name)).eval()
    opt = reference_optimizer(T, m, LR)
    names = {id(p): k for k, p in m.named_parameters()}
    assert len(opt.param_groups) == 2 and not opt.defaults["amsgrad"] and not opt.defaults.get("maximize", False)
    out = {name: dict(betas=list(opt.param_groups[0]["betas"]), eps=opt.param_groups[0]["eps"],
                      groups=[dict(weight_decay=g["weight_decay"], names=sorted(names[id(p)] for p in g["params"])) for g in opt.param_groups])}
    print(f"  {name}: {[(g['weight_decay'], len(g['names'])) for g in out[name]['groups']]} betas {out[name]['betas']} eps {out[name]['eps']}")
    with open(os.path.join(GOLD, "rq_optim_groups.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    assert REF and os.path.isdir(REF), "needs the reference tree: set ENH_REFERENCE_ROOT"
    groups()
    for name in BC.CASES:
        gold(name)
