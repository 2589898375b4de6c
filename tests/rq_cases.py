"""The cases of the stage-2 RQTransformer's teacher-forced forward, their seeded parameters and inputs.  Shared by tools/make_golden_rq_forward.py
(which runs the REFERENCE's RQTransformer on them and writes tests/golden/rq_fwd_<case>.npz) and tests/test_rq_forward_*.py.

Parameters are gpt_cases.make_params' draws (numpy MT19937 in sorted-key order from the SHAPES of a state dict: non-zero position tables, biases and
LayerNorm offsets, a noisy time_mix ramp, Linear weights of std 1 / sqrt(fan_in)); ln_spatial and ln_depth get the LayerNorm rule.

`forward_logits` is a plain-torch restatement of the reference's RQTransformer.forward with one condition token, built on S = T spatial rows (the
condition and the first T - 1 positions: the causal mask keeps the last position's row from every logit).  code_sum = "channels" is the reference's
line (`cumsum(-1)` of the [B, T, D, C] embeddings: along the channels), "depth" the running sum along the depth axis that the reference's sampler
assumes.  With rnd=None it is the fp32 / fp64 statement of the model; with rnd = a 16-bit rounding it has the rounding points of the device path:
every GEMM operand, q / k / v and the softmax numerators rounded to the format, products in `prod`, everything else in `work`."""
import math

import numpy as np
import torch

PARAM_SEED, INPUT_SEED, VOCAB_COND = 7, 3, 10
#          name       C  spatial heads  depth heads  spatial layers  depth layers  V   T   D  B
CASES = {"rq_tiny": (128, 2, 2, 1, 1, 64, 5, 4, 2),        # smallest
         "rq_d3": (192, 3, 1, 1, 2, 48, 7, 3, 3),          # depth head 192; 21 sequences, an odd pack
         "rq_hs384": (384, 1, 6, 1, 1, 64, 4, 2, 1),       # spatial head 384
         "rq_d8": (128, 2, 2, 1, 1, 40, 9, 8, 2),          # D = 8
         "rq_long": (128, 2, 2, 1, 1, 32, 131, 4, 1)}      # two query blocks of the spatial attention; 131 sequences


def case_kwargs(name: str) -> dict:
    C, Hs, Hd, Ls, Ld, V, T, D, _ = CASES[name]
    return dict(vocab_cond_size=VOCAB_COND, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, depth_num_tokens=D,
                spatial_n_heads=Hs, depth_n_heads=Hd, spatial_n_layers=Ls, depth_n_layers=Ld)


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
        elif ".ln" in k or k.startswith("ln_"):
            a = (1.0 if k.endswith("weight") else 0.0) + 0.05 * rs.standard_normal(shp)
        elif k.endswith("bias"):
            a = 0.02 * rs.standard_normal(shp)
        else:
            a = rs.standard_normal(shp) / math.sqrt(shp[1])
        P[k] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return P


def case_inputs(name: str):
    """(conds [B, 1] int64, codes [B, T, D] int64)"""
    V, T, D, B = CASES[name][5:]
    rs = np.random.RandomState(INPUT_SEED + len(name))
    conds = torch.from_numpy(rs.randint(0, VOCAB_COND, size=(B, 1)).astype(np.int64))
    codes = torch.from_numpy(rs.randint(0, V, size=(B, T, D)).astype(np.int64))
    return conds, codes


def forward_logits(P: dict, name: str, conds: torch.Tensor, codes: torch.Tensor, code_sum: str, rnd=None, prod=torch.float64, work=torch.float32):
    """logits [B T, D, V] (`work` dtype) of the teacher-forced forward; P on the device the computation should run on"""
    C, Hs, Hd, Ls, Ld, V, T, D, _ = CASES[name]
    B = conds.shape[0]
    dev = P["head.weight"].device
    r = (lambda t: t) if rnd is None else rnd
    W = {k: v.to(work) for k, v in P.items()}

    def mm(a, w):       # operands rounded to the format, products and sums in `prod`
        return (r(a).to(prod) @ r(w).to(prod).t()).to(work)

    def ln(x, pre):
        return torch.nn.functional.layer_norm(x, (C,), W[pre + ".weight"], W[pre + ".bias"], 1e-5)

    def blocks(x, stack: str, L: int, H: int):       # x [n, S, C]: n causal sequences of S rows
        n, S, hs = x.shape[0], x.shape[1], C // H
        causal = torch.ones(S, S, dtype=torch.bool, device=dev).tril()
        for i in range(L):
            pre = f"{stack}.{i}."
            tm = W[pre + "attn.time_mix"].reshape(-1)
            a = ln(x, pre + "ln1")
            prev = torch.cat([torch.zeros_like(a[:, :1]), a[:, :-1]], 1)      # time_shift: per sequence, row -1 is zero
            a = a * tm + prev * (1 - tm)
            wqkv = torch.cat([W[pre + "attn.query.weight"], W[pre + "attn.key.weight"], W[pre + "attn.value.weight"]], 0)
            bqkv = torch.cat([W[pre + "attn.query.bias"], W[pre + "attn.key.bias"], W[pre + "attn.value.bias"]])
            qkv = r(mm(a.reshape(n * S, C), wqkv) + bqkv)
            q, k, v = (z.reshape(n, S, H, hs).permute(0, 2, 1, 3).to(prod) for z in qkv.split(C, dim=1))
            s = (q @ k.transpose(-1, -2)).to(work) * (1.0 / math.sqrt(hs))
            s = s.masked_fill(~causal, float("-inf"))
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            y = ((r(e).to(prod) @ v).to(work) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(n * S, C)
            x = x + (mm(y, W[pre + "attn.proj.weight"]) + W[pre + "attn.proj.bias"]).view(n, S, C)
            hdn = torch.square(torch.relu(mm(ln(x, pre + "ln2").reshape(n * S, C), W[pre + "mlp.p0.weight"]) + W[pre + "mlp.p0.bias"]))
            x = x + (mm(hdn, W[pre + "mlp.p1.weight"]) + W[pre + "mlp.p1.bias"]).view(n, S, C)
        return x

    conds, codes = conds.to(dev).view(B, -1), codes.to(dev).view(B, T, D)
    emb = W["tok_emb_code.weight"][codes]                                         # [B, T, D, C]
    cs = emb.cumsum({"channels": -1, "depth": 2}[code_sum])                       # the reference's line / the running sum over depth
    x = torch.cat([W["tok_emb_cond.weight"][conds[:, :1]] + W["pos_emb_cond"][:, :1], cs[:, :T - 1, D - 1] + W["pos_emb_code"][:, :T - 1]], 1)
    h = ln(blocks(x, "spatial_transformer", Ls, Hs), "ln_spatial")                # [B, T, C]
    v = torch.cat([h.unsqueeze(2), cs[:, :, :D - 1] + W["pos_emb_depth"]], 2).reshape(B * T, D, C)
    v = blocks(v, "depth_transformer", Ld, Hd)
    return mm(ln(v, "ln_depth").reshape(B * T * D, C), W["head.weight"]).view(B * T, D, V)
