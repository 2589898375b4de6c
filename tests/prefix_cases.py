"""The yardstick of sample(prefix_codes=): the plain-torch restatements of the cached sampling loops (kv8_cases.step_logits / rq_step_logits, which
with kv=None are gpt_cases.step_logits / rq_sample_cases.step_logits bit for bit) with ONE addition: for the steps t < n_prefix, whose rows the
device runs through the batched prefill, the softmax numerators exp(s - max) pass through `rnd` before they meet V and the sum is divided out
afterwards.  That is the tile attention's extra rounding point, as gpt_forward_cases.forward_logits models it; the decode attention of the steps
t >= n_prefix keeps its f32 numerators.  Nothing else differs: the prefill computes the SAMPLER's model (every row is ln1(x) * time_mix, no
previous-row term), not the teacher-forced one.  With n_prefix = 0 the functions are the existing restatements bit for bit
(tests/test_sample_prefix_cpu.py), which are pinned to the reference's goldens.

The case table is this module's own: the sampling cases of gpt_cases.py and `long`, whose prefix of 150 rows crosses one 128-query block boundary
of the tile attention and ends in a ragged third 64-key tile.  gpt_cases.CASES is not touched."""
import math

import numpy as np
import torch

import gpt_cases as GC
import rq_sample_cases as SC

#                          name    C  heads layers V    T  B
CASES = dict(GC.CASES, long=(128, 2, 2, 64, 200, 2))
LONG_PREFIX = 150


def case_kwargs(name: str) -> dict:
    C, H, L, V, T, _ = CASES[name]
    return dict(vocab_cond_size=GC.VOCAB_COND, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, n_heads=H, n_layers=L)


def case_inputs(name: str):
    """(conds [B, 1] int64, forced codes [B, T] int64): gpt_cases.make_inputs with this module's case table"""
    _, _, _, V, T, B = CASES[name]
    rs = np.random.RandomState(GC.INPUT_SEED + len(name))
    conds = torch.from_numpy(rs.randint(0, GC.VOCAB_COND, size=(B, 1)).astype(np.int64))
    codes = torch.from_numpy(rs.randint(0, V, size=(B, T)).astype(np.int64))
    return conds, codes


def _attend(q, kc, vc, hs, r, prefilled: bool):
    """one row per (batch, head) over the cache slots given; prefilled: the tile attention's rounding of the numerators"""
    s = torch.einsum("bhd,bhtd->bht", q, kc) * (1.0 / math.sqrt(hs))
    if not prefilled:
        return torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), vc)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    return torch.einsum("bht,bhtd->bhd", r(e), vc) / e.sum(-1, keepdim=True)


def prefix_step_logits(P: dict, name: str, conds: torch.Tensor, forced: torch.Tensor, n_prefix: int, rnd=None, prod=torch.float64, work=torch.float32,
                       kv=None, table=None):
    """kv8_cases.step_logits with the numerators of the steps t < n_prefix through `rnd`; table: the case table (default: this module's)"""
    C, H, L, V, T, _ = (CASES if table is None else table)[name]
    hs = C // H
    B = conds.shape[0]
    dev = P["head.weight"].device
    r = (lambda t: t) if rnd is None else rnd
    kv = (lambda t: t) if kv is None else kv
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
            kc[i][:, :, t], vc[i][:, :, t] = kv(k), kv(v)
            y = _attend(q, kc[i][:, :, :t + 1], vc[i][:, :, :t + 1], hs, r, t < n_prefix).reshape(B, C)
            x = x + mm(y, W[pre + "attn.proj.weight"]) + W[pre + "attn.proj.bias"]
            hdn = torch.square(torch.relu(mm(ln(x, pre + "ln2"), W[pre + "mlp.p0.weight"]) + W[pre + "mlp.p0.bias"]))
            x = x + mm(hdn, W[pre + "mlp.p1.weight"]) + W[pre + "mlp.p1.bias"]
        out.append(mm(ln(x, "layer_norm"), W["head.weight"]))
    return torch.stack(out, 1)


def rq_prefix_step_logits(P: dict, name: str, conds: torch.Tensor, forced: torch.Tensor, slot0_ln: str, n_prefix: int, rnd=None, prod=torch.float64,
                          work=torch.float32, kv=None):
    """kv8_cases.rq_step_logits (rq_sample_cases.step_logits with the kv hook on the spatial stack) with the numerators of the SPATIAL steps
    t < n_prefix through `rnd`; the depth stack has no prefill"""
    C, Hs, Hd, Ls, Ld, V, T, D, _ = SC.CASES[name]
    assert slot0_ln in ("once", "twice")
    B = conds.shape[0]
    dev = P["head.weight"].device
    r = (lambda t: t) if rnd is None else rnd
    ident = lambda t: t
    kv = ident if kv is None else kv
    W = {k: v.to(work) for k, v in P.items()}

    def mm(a, w):       # operands rounded to the format, products and sums in `prod`
        return (r(a).to(prod) @ r(w).to(prod).t()).to(work)

    def ln(x, pre):
        return torch.nn.functional.layer_norm(x, (C,), W[pre + ".weight"], W[pre + ".bias"], 1e-5)

    def caches(L: int, H: int, slots: int):
        return [[torch.zeros(B, H, slots, C // H, dtype=work, device=dev) for _ in range(2)] for _ in range(L)]

    def blocks(x, stack: str, L: int, H: int, cache, t: int, hook, prefilled: bool):
        hs = C // H
        for i in range(L):
            pre = f"{stack}.{i}."
            a = ln(x, pre + "ln1") * W[pre + "attn.time_mix"].reshape(-1)
            wqkv = torch.cat([W[pre + "attn.query.weight"], W[pre + "attn.key.weight"], W[pre + "attn.value.weight"]], 0)
            bqkv = torch.cat([W[pre + "attn.query.bias"], W[pre + "attn.key.bias"], W[pre + "attn.value.bias"]])
            qkv = r(mm(a, wqkv) + bqkv)
            q, k, v = (z.view(B, H, hs) for z in qkv.split(C, dim=1))
            kc, vc = cache[i]
            kc[:, :, t], vc[:, :, t] = hook(k), hook(v)
            y = _attend(q, kc[:, :, :t + 1], vc[:, :, :t + 1], hs, r, prefilled).reshape(B, C)
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
        hidden = ln(blocks(x, "spatial_transformer", Ls, Hs, spatial, t, kv, t < n_prefix), "ln_spatial")
        depth = caches(Ld, Hd, D)
        for d in range(D):
            x = hidden if d == 0 else code_sum(forced[:, t, :d]) + W["pos_emb_depth"][0, d - 1]
            x = blocks(x, "depth_transformer", Ld, Hd, depth, d, ident, False)
            if d == 0 and slot0_ln == "twice":
                x = ln(x, "ln_depth")
            out[:, t, d] = mm(ln(x, "ln_depth"), W["head.weight"])
    return out.view(B * T, D, V)
