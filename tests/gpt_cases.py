"""The stage-2 GPT sampling cases and their seeded parameters and inputs: shared by tools/make_golden_gpt.py (which runs the REFERENCE's GPT on them and
writes tests/golden/gpt_<case>.npz) and tests/test_gpt_sample_*.py (which run this package on them).

Parameters are drawn with numpy's MT19937 in sorted-key order, from the SHAPES of a state dict.  Unlike the modules' init the position tables, biases
and LayerNorm offsets are non-zero and time_mix is its ramp plus noise, so a wrong row, a dropped bias or a missing time_mix shows in the logits;
Linear weights have std 1 / sqrt(fan_in), which puts the logits at scale ~1.

`step_logits` is a plain-torch restatement of the reference's cached sampling step (GPT.sample_step with one condition token: T == 1 in every block,
so the time-shift term is zero), fed with forced codes.  With rnd=None it is the fp32 / fp64 statement of the model; with rnd = a 16-bit rounding it
emulates the device path: every GEMM operand and cache entry rounded to the format, products in `prod`, everything else in f32."""
import math

import numpy as np
import torch

PARAM_SEED, INPUT_SEED, VOCAB_COND = 7, 3, 10
#         name     C  heads layers  V    T  B
CASES = {"tiny": (128, 2, 2, 512, 20, 2), "hs384": (768, 2, 1, 256, 6, 3), "h3": (192, 3, 2, 1000, 9, 1)}


def case_kwargs(name: str) -> dict:
    C, H, L, V, T, _ = CASES[name]
    return dict(vocab_cond_size=VOCAB_COND, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, n_heads=H, n_layers=L)


def make_params(shapes: dict, seed: int = PARAM_SEED) -> dict:
    """{name: tensor} for every entry of `shapes` ({state_dict key: shape}), drawn in sorted-key order"""
    rs = np.random.RandomState(seed)
    P = {}
    for k in sorted(shapes):
        shp = tuple(shapes[k])
        if k.endswith("time_mix"):
            C = shp[-1]
            a = (np.arange(C) / (C - 1)).reshape(shp) + 0.05 * rs.standard_normal(shp)
        elif k.startswith("pos_emb"):
            a = 0.1 * rs.standard_normal(shp)
        elif k.startswith("tok_emb"):
            a = rs.standard_normal(shp)
        elif ".ln" in k or k.startswith("layer_norm"):
            a = (1.0 if k.endswith("weight") else 0.0) + 0.05 * rs.standard_normal(shp)
        elif k.endswith("bias"):
            a = 0.02 * rs.standard_normal(shp)
        else:
            a = rs.standard_normal(shp) / math.sqrt(shp[1])
        P[k] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return P


def make_inputs(name: str):
    """(conds [B, 1] int64, forced codes [B, T] int64)"""
    _, _, _, V, T, B = CASES[name]
    rs = np.random.RandomState(INPUT_SEED + len(name))
    conds = torch.from_numpy(rs.randint(0, VOCAB_COND, size=(B, 1)).astype(np.int64))
    codes = torch.from_numpy(rs.randint(0, V, size=(B, T)).astype(np.int64))
    return conds, codes


def step_logits(P: dict, name: str, conds: torch.Tensor, forced: torch.Tensor, rnd=None, prod=torch.float64, work=torch.float32):
    """logits [B, T, V] (`work` dtype) of the cached sampling loop fed with `forced`; P on the device the computation should run on"""
    C, H, L, V, T, _ = CASES[name]
    hs = C // H
    B = conds.shape[0]
    dev = P["head.weight"].device
    r = (lambda t: t) if rnd is None else rnd
    W = {k: v.to(work) for k, v in P.items()}

    def mm(a, w):       # operands rounded to the format, products and sums in `prod`
        return (r(a).to(prod) @ r(w).to(prod).t()).to(work)

    def ln(x, pre):
        return torch.nn.functional.layer_norm(x, (C,), W[pre + ".weight"], W[pre + ".bias"], 1e-5)

    conds, forced = conds.to(dev), forced.to(dev)
    kc = [torch.zeros(B, H, T, hs, dtype=work, device=dev) for _ in range(L)]
    vc = [torch.zeros(B, H, T, hs, dtype=work, device=dev) for _ in range(L)]
    out = []
    for t in range(T):
        if t == 0:
            x = W["tok_emb_cond.weight"][conds[:, 0]] + W["pos_emb_cond"][0, 0]
        else:
            x = W["tok_emb_code.weight"][forced[:, t - 1]] + W["pos_emb_code"][0, t - 1]
        for i in range(L):
            pre = f"blocks.{i}."
            a = ln(x, pre + "ln1") * W[pre + "attn.time_mix"].reshape(-1)
            wqkv = torch.cat([W[pre + "attn.query.weight"], W[pre + "attn.key.weight"], W[pre + "attn.value.weight"]], 0)
            bqkv = torch.cat([W[pre + "attn.query.bias"], W[pre + "attn.key.bias"], W[pre + "attn.value.bias"]])
            qkv = r(mm(a, wqkv) + bqkv)
            q, k, v = (z.view(B, H, hs) for z in qkv.split(C, dim=1))
            kc[i][:, :, t], vc[i][:, :, t] = k, v
            s = torch.einsum("bhd,bhtd->bht", q, kc[i][:, :, :t + 1]) * (1.0 / math.sqrt(hs))
            y = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), vc[i][:, :, :t + 1]).reshape(B, C)
            x = x + mm(y, W[pre + "attn.proj.weight"]) + W[pre + "attn.proj.bias"]
            hdn = torch.square(torch.relu(mm(ln(x, pre + "ln2"), W[pre + "mlp.p0.weight"]) + W[pre + "mlp.p0.bias"]))
            x = x + mm(hdn, W[pre + "mlp.p1.weight"]) + W[pre + "mlp.p1.bias"]
        out.append(mm(ln(x, "layer_norm"), W["head.weight"]))
    return torch.stack(out, 1)


def host_filter(logits: torch.Tensor, top_k=None, top_p=None, temperature: float = 1.0):
    """GPT.sample lines 233-258 on one batch of rows in the dtype of `logits`: (processed logits, kept mask, renormalised probabilities)"""
    x = logits / temperature
    if top_k is not None:
        v, _ = torch.topk(x, top_k)
        x = x.masked_fill(x < v[:, [-1]], -float("inf"))
    probs = torch.softmax(x, dim=-1)
    keep = torch.isfinite(x)
    if top_p is not None:
        sp, si = torch.sort(probs, dim=-1, descending=True)
        rm = torch.cumsum(sp, dim=-1) >= top_p
        rm[..., 1:] = rm[..., :-1].clone()
        rm[..., 0] = False
        remove = rm.scatter(-1, si, rm)
        probs = probs.masked_fill(remove, 0.0)
        probs = probs / probs.sum(-1, keepdim=True)
        keep = keep & ~remove
    return x, keep, probs


def inverse_cdf(probs: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """the first index whose running sum of probs exceeds u * sum(probs), per row"""
    c = torch.cumsum(probs, dim=-1)
    return (c > (u * c[:, -1]).unsqueeze(-1)).to(torch.int64).argmax(dim=-1)
