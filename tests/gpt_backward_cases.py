"""The cases of the stage-2 GPT's backward (GPT.forward_backward): the five of tests/gpt_forward_cases.py and two that put the causal attention
backward on its other paths (`hs128`: D = 128, the widest unsliced kernel, T = 70 spans two key tiles; `hs384long`: D = 384 over three key tiles
and two query blocks).  Shared by tools/make_golden_gpt_backward.py (which runs the REFERENCE's GPT with F.cross_entropy(...).backward() in fp64
and writes tests/golden/gpt_bwd_<case>.npz) and tests/test_gpt_backward_*.py.

`forward` / `loss_and_grads` are a plain-torch restatement of the teacher-forced forward and a HAND-WRITTEN backward of it, taking the dimensions
directly.  With rnd=None they are the fp64 statement of the model.  With rnd = a 16-bit rounding they have the device path's rounding points, with
every product and everything else in fp64:
  forward  (gpt_forward_cases.py): every GEMM operand, q / k / v, the softmax numerators exp(s - max), the attention's stored output;
  backward: every GEMM operand (the 16-bit copies of the residual stream's gradient, datt = the 16-bit output of proj's input-gradient product),
            dlogits, P = exp(s - lse) and P o (dP - delta) before their products (delta on the STORED output), dq / dk / dv, dh, and relu(h) taken
            as sqrt of the stored 16-bit relu(h)^2 (what enh_relu_sq_backward reads: h itself is not kept).
Bias gradients are column sums of the 16-bit operand, as on the device.  loss_scale multiplies dlogits BEFORE its rounding, so fp16 underflow is
modelled; the returned gradients carry the factor."""
import math

import numpy as np
import torch

import gpt_forward_cases as FC
from gpt_forward_cases import PARAM_SEED, VOCAB_COND, make_params  # noqa: F401

#                                name      C  heads layers V   T   B
CASES = dict(FC.CASES, hs128=(256, 2, 1, 64, 70, 2), hs384long=(768, 2, 1, 64, 150, 1))
FULL_LIMIT = 4096         # a golden keeps the whole gradient of a tensor up to this many elements, else its norm and two projections
EPS = 1e-5


def case_kwargs(name: str) -> dict:
    C, H, L, V, T, _ = CASES[name]
    return dict(vocab_cond_size=VOCAB_COND, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, n_heads=H, n_layers=L)


def case_dims(name: str):
    C, H, L, V, T, _ = CASES[name]
    return C, H, L, V, T


def case_inputs(name: str):
    """(conds [B, 1] int64, codes [B, T] int64): gpt_forward_cases.case_inputs' draw with this module's table (the shared cases get the same inputs)"""
    _, _, _, V, T, B = CASES[name]
    rs = np.random.RandomState(FC.GC.INPUT_SEED + len(name))
    conds = torch.from_numpy(rs.randint(0, VOCAB_COND, size=(B, 1)).astype(np.int64))
    codes = torch.from_numpy(rs.randint(0, V, size=(B, T)).astype(np.int64))
    return conds, codes


def projections(G: torch.Tensor, seed: int):
    """(norm, G r, l G) of a gradient seen as a matrix [-1, last axis], r and l standard normal from `seed` (numpy MT19937, r first)"""
    G2 = G.detach().double().reshape(-1, G.shape[-1])
    rs = np.random.RandomState(seed)
    r = torch.from_numpy(rs.standard_normal(G2.shape[1]))
    l = torch.from_numpy(rs.standard_normal(G2.shape[0]))
    return G2.norm(), G2 @ r, l @ G2


def _ln(x, w, b):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + EPS)
    xh = xc * rstd
    return xh * w + b, xh, rstd


def _ln_bwd(g, xh, rstd, w):
    """gradient of x given the gradient g of xh w + b"""
    gw = g * w
    return (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True)) * rstd


def forward(W: dict, dims, conds, codes, rnd=None):
    """(logits [B, T, V], mean cross-entropy, what the backward needs) in the dtype of W (fp64 for the statements above); differentiable by autograd"""
    C, H, L, V, T = dims
    hs, S = C // H, T
    B = conds.shape[0]
    r = (lambda t: t) if rnd is None else rnd
    conds, codes = conds.view(B, -1), codes.view(B, -1)
    x = torch.cat([W["tok_emb_cond.weight"][conds[:, :1]] + W["pos_emb_cond"][:, :1], W["tok_emb_code.weight"][codes[:, :S - 1]] + W["pos_emb_code"][:, :S - 1]], 1)
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    heads = lambda z: z.reshape(B, S, H, hs).permute(0, 2, 1, 3)
    sv = []
    for i in range(L):
        pre = f"blocks.{i}."
        tm = W[pre + "attn.time_mix"].reshape(-1)
        l1, xh1, rs1 = _ln(x, W[pre + "ln1.weight"], W[pre + "ln1.bias"])
        prev = torch.cat([torch.zeros_like(l1[:, :1]), l1[:, :-1]], 1)      # time_shift: per batch element, row -1 is zero
        a = r(l1 * tm + prev * (1 - tm))
        wqkv = r(torch.cat([W[pre + "attn.query.weight"], W[pre + "attn.key.weight"], W[pre + "attn.value.weight"]], 0))
        bqkv = torch.cat([W[pre + "attn.query.bias"], W[pre + "attn.key.bias"], W[pre + "attn.value.bias"]])
        qkv = r(a @ wqkv.t() + bqkv)
        q, k, v = (heads(z) for z in qkv.split(C, dim=-1))
        s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hs))
        s = s.masked_fill(~causal, float("-inf"))
        mx = s.amax(dim=-1, keepdim=True)
        e = torch.exp(s - mx)
        lsum = e.sum(-1, keepdim=True)
        y = r(((r(e) @ v) / lsum).permute(0, 2, 1, 3).reshape(B, S, C))
        wproj = r(W[pre + "attn.proj.weight"])
        x2 = x + y @ wproj.t() + W[pre + "attn.proj.bias"]
        l2, xh2, rs2 = _ln(x2, W[pre + "ln2.weight"], W[pre + "ln2.bias"])
        a2 = r(l2)
        w0, w1 = r(W[pre + "mlp.p0.weight"]), r(W[pre + "mlp.p1.weight"])
        h = a2 @ w0.t() + W[pre + "mlp.p0.bias"]
        hid = r(torch.square(torch.relu(h)))
        sv.append(dict(xh1=xh1, rs1=rs1, l1=l1, prev=prev, tm=tm, a=a, wqkv=wqkv, q=q, k=k, v=v, s=s, lse=mx + torch.log(lsum), y=y, wproj=wproj, xh2=xh2, rs2=rs2,
                       a2=a2, w0=w0, w1=w1, h=h, hid=hid))
        x = x2 + hid @ w1.t() + W[pre + "mlp.p1.bias"]
    lf, xhf, rsf = _ln(x, W["layer_norm.weight"], W["layer_norm.bias"])
    af, wh = r(lf), r(W["head.weight"])
    logits = af @ wh.t()
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), codes.reshape(-1))
    return logits, loss, dict(layers=sv, xhf=xhf, rsf=rsf, af=af, wh=wh)


def loss_and_grads(P: dict, dims, conds, codes, rnd=None, loss_scale: float = 1.0):
    """(loss, {state-dict name: loss_scale x gradient of the mean cross-entropy}, logits) by the hand-written backward, in fp64 on the CPU"""
    C, H, L, V, T = dims
    hs, S = C // H, T
    B = conds.shape[0]
    scale = 1.0 / math.sqrt(hs)
    r = (lambda t: t) if rnd is None else rnd
    W = {k: v.detach().double().cpu() for k, v in P.items()}
    conds, codes = conds.cpu().view(B, -1), codes.cpu().view(B, -1)
    with torch.no_grad():
        logits, loss, sv = forward(W, dims, conds, codes, rnd)
        G = {}
        heads = lambda z: z.reshape(B, S, H, hs).permute(0, 2, 1, 3)
        back = lambda z: z.permute(0, 2, 1, 3).reshape(B, S, C)
        rows = lambda z: z.reshape(B * S, -1)
        # 1. loss gradient
        dl = torch.softmax(logits, dim=-1)
        dl.view(-1, V)[torch.arange(B * T), codes.reshape(-1)] -= 1.0
        dl = r(dl * (loss_scale / (B * T)))
        # 2. head, 3. final LayerNorm
        G["head.weight"] = rows(dl).t() @ rows(sv["af"])
        da = dl @ sv["wh"]
        G["layer_norm.weight"], G["layer_norm.bias"] = (da * sv["xhf"]).sum((0, 1)), da.sum((0, 1))
        g = _ln_bwd(da, sv["xhf"], sv["rsf"], W["layer_norm.weight"])
        # 4. the layers, last to first
        for i in range(L - 1, -1, -1):
            pre, A = f"blocks.{i}.", sv["layers"][i]
            g16 = r(g)
            G[pre + "mlp.p1.weight"], G[pre + "mlp.p1.bias"] = rows(g16).t() @ rows(A["hid"]), rows(g16).sum(0)
            dhid = g16 @ A["w1"]
            relu_h = torch.relu(A["h"]) if rnd is None else torch.sqrt(A["hid"])
            dh = r(dhid * (2.0 * relu_h))
            G[pre + "mlp.p0.weight"], G[pre + "mlp.p0.bias"] = rows(dh).t() @ rows(A["a2"]), rows(dh).sum(0)
            da2 = dh @ A["w0"]
            G[pre + "ln2.weight"], G[pre + "ln2.bias"] = (da2 * A["xh2"]).sum((0, 1)), da2.sum((0, 1))
            g2 = g + _ln_bwd(da2, A["xh2"], A["rs2"], W[pre + "ln2.weight"])
            g2_16 = r(g2)
            G[pre + "attn.proj.weight"], G[pre + "attn.proj.bias"] = rows(g2_16).t() @ rows(A["y"]), rows(g2_16).sum(0)
            do = heads(r(g2_16 @ A["wproj"]))
            # causal attention backward: P from lse, delta on the stored output
            p = torch.exp(A["s"] - A["lse"])
            dv = r(r(p).transpose(-1, -2) @ do)
            delta = (do * heads(A["y"])).sum(-1, keepdim=True)
            ds = r(p * (do @ A["v"].transpose(-1, -2) - delta))
            dq, dk = r((ds @ A["k"]) * scale), r((ds.transpose(-1, -2) @ A["q"]) * scale)
            dqkv = torch.cat([back(dq), back(dk), back(dv)], -1)
            dw, db = rows(dqkv).t() @ rows(A["a"]), rows(dqkv).sum(0)
            for j, nm in enumerate(("query", "key", "value")):
                G[pre + f"attn.{nm}.weight"], G[pre + f"attn.{nm}.bias"] = dw[j * C:(j + 1) * C], db[j * C:(j + 1) * C]
            da1 = dqkv @ A["wqkv"]
            # ln1 + time shift
            tm = A["tm"]
            nxt = torch.cat([da1[:, 1:], torch.zeros_like(da1[:, :1])], 1)      # the gradient row s + 1 sends back to ln[s]: nothing crosses a batch element
            gl = da1 * tm + nxt * (1 - tm)
            G[pre + "attn.time_mix"] = (da1 * (A["l1"] - A["prev"])).sum((0, 1)).view(1, 1, C)
            G[pre + "ln1.weight"], G[pre + "ln1.bias"] = (gl * A["xh1"]).sum((0, 1)), gl.sum((0, 1))
            g = g2 + _ln_bwd(gl, A["xh1"], A["rs1"], W[pre + "ln1.weight"])
        # 5. embeddings: only the condition and the first T - 1 codes are fed
        G["tok_emb_code.weight"] = torch.zeros_like(W["tok_emb_code.weight"]).index_add_(0, codes[:, :S - 1].reshape(-1), g[:, 1:].reshape(-1, C))
        G["tok_emb_cond.weight"] = torch.zeros_like(W["tok_emb_cond.weight"]).index_add_(0, conds[:, 0], g[:, 0])
        G["pos_emb_code"] = torch.zeros_like(W["pos_emb_code"])
        G["pos_emb_code"][0, :S - 1] = g[:, 1:].sum(0)
        G["pos_emb_cond"] = g[:, :1].sum(0, keepdim=True)
    return loss, G, logits
