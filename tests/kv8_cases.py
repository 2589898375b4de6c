"""The yardstick of sample(cache="fp8"): the plain-torch restatements of the cached sampling loops (gpt_cases.step_logits,
rq_sample_cases.step_logits) with a hook `kv` that every step's k and v rows pass through BEFORE they enter the cache and the step's own attention.
With kv=None the functions are those restatements bit for bit (tests/test_kv8_cpu.py), which are pinned to the reference's goldens; with kv=kv8 a
slot holds, and every step that reads it sees, the MXFP8 form of the row (tests/mxfp8_util.py: blocks of 32 along the head dimension).  In the RQ
loop only the spatial stack's rows are passed through the hook: the depth caches stay as they are."""
import math

import torch

import gpt_cases as GC
import mxfp8_util as MX
import rq_sample_cases as SC


def kv8(z):
    """[B, H, hs] -> the MXFP8 form of every head row, in the dtype and on the device of z: dequant(quant(z as [B H, hs] f32)), computed on the CPU
    (where torch's e4m3fn cast is the specification)"""
    B, H, hs = z.shape
    q = MX.dequant(*MX.quant(z.detach().float().cpu().contiguous().view(B * H, hs)))
    return q.view(B, H, hs).to(device=z.device, dtype=z.dtype)


def step_logits(P: dict, name: str, conds: torch.Tensor, forced: torch.Tensor, rnd=None, prod=torch.float64, work=torch.float32, kv=None):
    """gpt_cases.step_logits with k and v passed through `kv` before they enter the cache and the step's attention"""
    C, H, L, V, T, _ = GC.CASES[name]
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
            s = torch.einsum("bhd,bhtd->bht", q, kc[i][:, :, :t + 1]) * (1.0 / math.sqrt(hs))
            y = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), vc[i][:, :, :t + 1]).reshape(B, C)
            x = x + mm(y, W[pre + "attn.proj.weight"]) + W[pre + "attn.proj.bias"]
            hdn = torch.square(torch.relu(mm(ln(x, pre + "ln2"), W[pre + "mlp.p0.weight"]) + W[pre + "mlp.p0.bias"]))
            x = x + mm(hdn, W[pre + "mlp.p1.weight"]) + W[pre + "mlp.p1.bias"]
        out.append(mm(ln(x, "layer_norm"), W["head.weight"]))
    return torch.stack(out, 1)


def rq_step_logits(P: dict, name: str, conds: torch.Tensor, forced: torch.Tensor, slot0_ln: str, rnd=None, prod=torch.float64, work=torch.float32,
                   kv=None):
    """rq_sample_cases.step_logits with the SPATIAL stack's k and v passed through `kv` before they enter the cache and the step's attention; the
    depth stack is untouched"""
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

    def blocks(x, stack: str, L: int, H: int, cache, t: int, hook):       # x [B, C]: one row per batch element, appended at slot t of the caches
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
        hidden = ln(blocks(x, "spatial_transformer", Ls, Hs, spatial, t, kv), "ln_spatial")
        depth = caches(Ld, Hd, D)
        for d in range(D):
            x = hidden if d == 0 else code_sum(forced[:, t, :d]) + W["pos_emb_depth"][0, d - 1]
            x = blocks(x, "depth_transformer", Ld, Hd, depth, d, ident)
            if d == 0 and slot0_ln == "twice":
                x = ln(x, "ln_depth")
            out[:, t, d] = mm(ln(x, "ln_depth"), W["head.weight"])
    return out.view(B * T, D, V)
