"""The stage-2 RQTransformer sampling cases and their seeded parameters and inputs: shared by tools/make_golden_rq_sample.py (which steps the
REFERENCE's sample_spatial_step / sample_depth_step on them and writes tests/golden/rq_sample_<case>.npz) and tests/test_rq_sample_*.py.

Parameters are rq_cases.make_params' draws (non-zero position tables, biases and LayerNorm offsets, a noisy time_mix ramp, Linear weights of std
1 / sqrt(fan_in)).  The cases are the smallest shapes that reach each path of the loop.

`step_logits` is a plain-torch restatement of the reference's cached sampling loop with one condition token, fed with forced codes: every Block of
both transformers sees one row (time_shift is zero, the mix is ln1(x) * time_mix), the spatial stack under a cache of T slots, the depth stack
under a cache of D slots rebuilt at every position.  slot0_ln = "twice" applies ln_depth to depth slot 0 twice, as the reference's
sample_depth_step does; "once" is what the teacher-forced forward (so training) computes.  With rnd=None it is the fp32 / fp64 statement of the
model; with rnd = a 16-bit rounding it has the rounding points of the device path: every GEMM operand and cache entry rounded to the format,
products in `prod`, everything else in `work`."""
import math

import numpy as np
import torch

import rq_cases as RC

PARAM_SEED, INPUT_SEED, VOCAB_COND = RC.PARAM_SEED, RC.INPUT_SEED, RC.VOCAB_COND
make_params = RC.make_params
#          name       C  spatial heads  depth heads  spatial layers  depth layers  V   T   D  B
CASES = {"rq_tiny": (128, 2, 2, 1, 1, 64, 5, 4, 2),        # smallest
         "rq_d3": (192, 3, 1, 1, 2, 48, 7, 3, 3),          # depth head 192, two depth layers, odd D
         "rq_hs384": (384, 1, 6, 1, 1, 64, 4, 2, 1),       # spatial head 384
         "rq_d8": (128, 2, 2, 1, 1, 40, 9, 8, 2),          # D = 8, the cap
         "rq_t70": (128, 2, 2, 1, 1, 32, 70, 2, 1)}        # the spatial cache passes 64 slots: the decode attention's split + merge


def case_kwargs(name: str) -> dict:
    C, Hs, Hd, Ls, Ld, V, T, D, _ = CASES[name]
    return dict(vocab_cond_size=VOCAB_COND, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, depth_num_tokens=D,
                spatial_n_heads=Hs, depth_n_heads=Hd, spatial_n_layers=Ls, depth_n_layers=Ld)


def case_inputs(name: str):
    """(conds [B, 1] int64, forced codes [B, T, D] int64)"""
    V, T, D, B = CASES[name][5:]
    rs = np.random.RandomState(INPUT_SEED + 100 + len(name))
    conds = torch.from_numpy(rs.randint(0, VOCAB_COND, size=(B, 1)).astype(np.int64))
    codes = torch.from_numpy(rs.randint(0, V, size=(B, T, D)).astype(np.int64))
    return conds, codes


def step_logits(P: dict, name: str, conds: torch.Tensor, forced: torch.Tensor, slot0_ln: str, rnd=None, prod=torch.float64, work=torch.float32):
    """logits [B T, D, V] (`work` dtype) of the cached sampling loop fed with `forced`; P on the device the computation should run on"""
    C, Hs, Hd, Ls, Ld, V, T, D, _ = CASES[name]
    assert slot0_ln in ("once", "twice")
    B = conds.shape[0]
    dev = P["head.weight"].device
    r = (lambda t: t) if rnd is None else rnd
    W = {k: v.to(work) for k, v in P.items()}

    def mm(a, w):       # operands rounded to the format, products and sums in `prod`
        return (r(a).to(prod) @ r(w).to(prod).t()).to(work)

    def ln(x, pre):
        return torch.nn.functional.layer_norm(x, (C,), W[pre + ".weight"], W[pre + ".bias"], 1e-5)

    def caches(L: int, H: int, slots: int):
        return [[torch.zeros(B, H, slots, C // H, dtype=work, device=dev) for _ in range(2)] for _ in range(L)]

    def blocks(x, stack: str, L: int, H: int, cache, t: int):       # x [B, C]: one row per batch element, appended at slot t of the caches
        hs = C // H
        for i in range(L):
            pre = f"{stack}.{i}."
            a = ln(x, pre + "ln1") * W[pre + "attn.time_mix"].reshape(-1)
            wqkv = torch.cat([W[pre + "attn.query.weight"], W[pre + "attn.key.weight"], W[pre + "attn.value.weight"]], 0)
            bqkv = torch.cat([W[pre + "attn.query.bias"], W[pre + "attn.key.bias"], W[pre + "attn.value.bias"]])
            qkv = r(mm(a, wqkv) + bqkv)
            q, k, v = (z.view(B, H, hs) for z in qkv.split(C, dim=1))
            kc, vc = cache[i]
            kc[:, :, t], vc[:, :, t] = k, v
            s = torch.einsum("bhd,bhtd->bht", q, kc[:, :, :t + 1]) * (1.0 / math.sqrt(hs))
            y = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), vc[:, :, :t + 1]).reshape(B, C)
            x = x + mm(y, W[pre + "attn.proj.weight"]) + W[pre + "attn.proj.bias"]
            hdn = torch.square(torch.relu(mm(ln(x, pre + "ln2"), W[pre + "mlp.p0.weight"]) + W[pre + "mlp.p0.bias"]))
            x = x + mm(hdn, W[pre + "mlp.p1.weight"]) + W[pre + "mlp.p1.bias"]
        return x

    def code_sum(ids):      # [B, n] -> the sum of the n embedding rows in ascending depth
        e = W["tok_emb_code.weight"][ids]
        x = e[:, 0]
        for j in range(1, ids.shape[1]):
            x = x + e[:, j]
        return x

    conds, forced = conds.to(dev).view(B, -1), forced.to(dev).view(B, T, D)
    spatial = caches(Ls, Hs, T)
    out = torch.empty(B, T, D, V, dtype=work, device=dev)
    for t in range(T):
        if t == 0:
            x = W["tok_emb_cond.weight"][conds[:, 0]] + W["pos_emb_cond"][0, 0]
        else:
            x = code_sum(forced[:, t - 1]) + W["pos_emb_code"][0, t - 1]
        hidden = ln(blocks(x, "spatial_transformer", Ls, Hs, spatial, t), "ln_spatial")
        depth = caches(Ld, Hd, D)
        for d in range(D):
            x = hidden if d == 0 else code_sum(forced[:, t, :d]) + W["pos_emb_depth"][0, d - 1]
            x = blocks(x, "depth_transformer", Ld, Hd, depth, d)
            if d == 0 and slot0_ln == "twice":
                x = ln(x, "ln_depth")
            out[:, t, d] = mm(ln(x, "ln_depth"), W["head.weight"])
    return out.view(B * T, D, V)
