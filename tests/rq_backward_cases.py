"""The cases of the stage-2 RQTransformer's backward (RQTransformer.forward_backward): the five of tests/rq_cases.py and two more (`rq_dh384`: a
depth head of 384 at D = 8, the register extreme of the short-sequence attention backward, and two spatial layers; `rq_t2`: 6 spatial and 12 depth rows,
so both stages contract over more rows than they have).  Shared by tools/make_golden_rq_backward.py (which runs the REFERENCE's RQTransformer with
F.cross_entropy(...).backward() in fp64 and writes tests/golden/rq_bwd_<case>.npz) and tests/test_rq_backward_*.py, tests/test_rq_train_gpu.py.

`forward` / `loss_and_grads` are a plain-torch restatement of the teacher-forced forward (S = T spatial rows) and a HAND-WRITTEN backward of it, in
either code_sum mode.  With rnd=None they are the fp64 statement of the model.  With rnd = a 16-bit rounding they have the device path's rounding
points, which are tests/gpt_backward_cases.py's list for the Blocks of both stacks (every GEMM operand, q / k / v, the softmax numerators, the stored
attention output; dlogits, P and P o (dP - delta), dq / dk / dv, dh, relu(h) as sqrt of the stored relu(h)^2) with everything else in fp64: the
gradients that cross ln_depth, ln_spatial and the embedding stage stay unrounded (f32 on the device).  loss_scale multiplies dlogits BEFORE its
rounding; the returned gradients carry the factor."""
import math

import numpy as np
import torch

import rq_cases as RC
from gpt_backward_cases import _ln, _ln_bwd, projections  # noqa: F401
from rq_cases import PARAM_SEED, VOCAB_COND, make_params  # noqa: F401

#                                  name       C  spatial heads  depth heads  spatial layers  depth layers  V   T   D  B
CASES = dict(RC.CASES, rq_dh384=(384, 6, 1, 2, 1, 40, 3, 8, 1), rq_t2=(128, 2, 2, 1, 1, 32, 2, 2, 3))
MODES = ("depth", "channels")
WHOLE_LIMIT = 256         # a golden keeps the whole gradient of a tensor up to this many elements, else its norm and two folded projections


def folded_projections(G: torch.Tensor, seed: int):
    """gpt_backward_cases.projections' (norm, G r, l G) of a gradient seen as a matrix [-1, last axis], with a projection of more than WHOLE_LIMIT
    elements (a multiple of 64) folded to 64 sums of every 64th element: still 64 independent random functionals of G per side, at a size that lets
    two modes of a 384-wide model with three layers fit one golden file"""
    fold = lambda v: v.reshape(-1, 64).sum(0) if v.numel() > WHOLE_LIMIT and v.numel() % 64 == 0 else v
    n, gr, lg = projections(G, seed)
    return n, fold(gr), fold(lg)


def case_kwargs(name: str) -> dict:
    C, Hs, Hd, Ls, Ld, V, T, D, _ = CASES[name]
    return dict(vocab_cond_size=VOCAB_COND, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, depth_num_tokens=D,
                spatial_n_heads=Hs, depth_n_heads=Hd, spatial_n_layers=Ls, depth_n_layers=Ld)


def case_dims(name: str):
    return CASES[name][:8]


def case_inputs(name: str):
    """(conds [B, 1] int64, codes [B, T, D] int64): rq_cases.case_inputs' draw with this module's table (the shared cases get the same inputs)"""
    V, T, D, B = CASES[name][5:]
    rs = np.random.RandomState(RC.INPUT_SEED + len(name))
    conds = torch.from_numpy(rs.randint(0, VOCAB_COND, size=(B, 1)).astype(np.int64))
    codes = torch.from_numpy(rs.randint(0, V, size=(B, T, D)).astype(np.int64))
    return conds, codes


def _blocks(W, stack: str, L: int, H: int, x, r):
    """x [n, S, C] through the L Blocks of `stack`: (output, what the backward needs per layer); gpt_backward_cases.forward's Block"""
    n, S, C = x.shape
    hs = C // H
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    heads = lambda z: z.reshape(n, S, H, hs).permute(0, 2, 1, 3)
    sv = []
    for i in range(L):
        pre = f"{stack}.{i}."
        tm = W[pre + "attn.time_mix"].reshape(-1)
        l1, xh1, rs1 = _ln(x, W[pre + "ln1.weight"], W[pre + "ln1.bias"])
        prev = torch.cat([torch.zeros_like(l1[:, :1]), l1[:, :-1]], 1)      # time_shift: per sequence, row -1 is zero
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
        y = r(((r(e) @ v) / lsum).permute(0, 2, 1, 3).reshape(n, S, C))
        wproj = r(W[pre + "attn.proj.weight"])
        x2 = x + y @ wproj.t() + W[pre + "attn.proj.bias"]
        l2, xh2, rs2 = _ln(x2, W[pre + "ln2.weight"], W[pre + "ln2.bias"])
        a2 = r(l2)
        w0, w1 = r(W[pre + "mlp.p0.weight"]), r(W[pre + "mlp.p1.weight"])
        h = a2 @ w0.t() + W[pre + "mlp.p0.bias"]
        hid = r(torch.square(torch.relu(h)))
        sv.append(dict(xh1=xh1, rs1=rs1, l1=l1, prev=prev, tm=tm, a=a, wqkv=wqkv, q=q, k=k, v=v, s=s, lse=mx + torch.log(lsum), y=y, wproj=wproj, xh2=xh2,
                       rs2=rs2, a2=a2, w0=w0, w1=w1, h=h, hid=hid))
        x = x2 + hid @ w1.t() + W[pre + "mlp.p1.bias"]
    return x, sv


def _blocks_backward(W, G, stack: str, L: int, H: int, g, layers, r, exact: bool):
    """the hand-written backward of _blocks: g [n, S, C] is the gradient of the output; fills G, returns the gradient of the input.
    gpt_backward_cases.loss_and_grads' step 4."""
    n, S, C = g.shape
    hs = C // H
    scale = 1.0 / math.sqrt(hs)
    heads = lambda z: z.reshape(n, S, H, hs).permute(0, 2, 1, 3)
    back = lambda z: z.permute(0, 2, 1, 3).reshape(n, S, C)
    rows = lambda z: z.reshape(n * S, -1)
    for i in range(L - 1, -1, -1):
        pre, A = f"{stack}.{i}.", layers[i]
        g16 = r(g)
        G[pre + "mlp.p1.weight"], G[pre + "mlp.p1.bias"] = rows(g16).t() @ rows(A["hid"]), rows(g16).sum(0)
        dhid = g16 @ A["w1"]
        relu_h = torch.relu(A["h"]) if exact else torch.sqrt(A["hid"])
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
        tm = A["tm"]
        nxt = torch.cat([da1[:, 1:], torch.zeros_like(da1[:, :1])], 1)      # the gradient row s + 1 sends back to ln[s]: nothing crosses a sequence
        gl = da1 * tm + nxt * (1 - tm)
        G[pre + "attn.time_mix"] = (da1 * (A["l1"] - A["prev"])).sum((0, 1)).view(1, 1, C)
        G[pre + "ln1.weight"], G[pre + "ln1.bias"] = (gl * A["xh1"]).sum((0, 1)), gl.sum((0, 1))
        g = g2 + _ln_bwd(gl, A["xh1"], A["rs1"], W[pre + "ln1.weight"])
    return g


def forward(W: dict, dims, conds, codes, code_sum: str = "depth", rnd=None):
    """(logits [B T, D, V], mean cross-entropy over all B T D codes, what the backward needs) in the dtype of W; differentiable by autograd"""
    C, Hs, Hd, Ls, Ld, V, T, D = dims
    B = conds.shape[0]
    r = (lambda t: t) if rnd is None else rnd
    conds, codes = conds.view(B, -1), codes.view(B, T, D)
    emb = W["tok_emb_code.weight"][codes]                                          # [B, T, D, C]
    cs = emb.cumsum({"channels": -1, "depth": 2}[code_sum])
    x = torch.cat([W["tok_emb_cond.weight"][conds[:, :1]] + W["pos_emb_cond"][:, :1], cs[:, :T - 1, D - 1] + W["pos_emb_code"][:, :T - 1]], 1)
    xs, sv_s = _blocks(W, "spatial_transformer", Ls, Hs, x, r)
    h, xhs, rss = _ln(xs, W["ln_spatial.weight"], W["ln_spatial.bias"])            # [B, T, C]
    v = torch.cat([h.unsqueeze(2), cs[:, :, :D - 1] + W["pos_emb_depth"]], 2).reshape(B * T, D, C)
    xd, sv_d = _blocks(W, "depth_transformer", Ld, Hd, v, r)
    lf, xhf, rsf = _ln(xd, W["ln_depth.weight"], W["ln_depth.bias"])
    af, wh = r(lf), r(W["head.weight"])
    logits = af @ wh.t()
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), codes.reshape(-1))
    return logits, loss, dict(spatial=sv_s, depth=sv_d, xhs=xhs, rss=rss, xhf=xhf, rsf=rsf, af=af, wh=wh)


def loss_and_grads(P: dict, dims, conds, codes, code_sum: str = "depth", rnd=None, loss_scale: float = 1.0):
    """(loss, {state-dict name: loss_scale x gradient of the mean cross-entropy}, logits) by the hand-written backward, in fp64 on the CPU"""
    C, Hs, Hd, Ls, Ld, V, T, D = dims
    B = conds.shape[0]
    r = (lambda t: t) if rnd is None else rnd
    W = {k: v.detach().double().cpu() for k, v in P.items()}
    conds, codes = conds.cpu().view(B, -1), codes.cpu().view(B, T, D)
    with torch.no_grad():
        logits, loss, sv = forward(W, dims, conds, codes, code_sum, rnd)
        G = {}
        N = B * T * D
        # 1. loss gradient, 2. head, 3. ln_depth
        dl = torch.softmax(logits, dim=-1)
        dl.view(-1, V)[torch.arange(N), codes.reshape(-1)] -= 1.0
        dl = r(dl * (loss_scale / N))
        G["head.weight"] = dl.reshape(N, V).t() @ sv["af"].reshape(N, C)
        da = dl @ sv["wh"]
        G["ln_depth.weight"], G["ln_depth.bias"] = (da * sv["xhf"]).sum((0, 1)), da.sum((0, 1))
        g = _ln_bwd(da, sv["xhf"], sv["rsf"], W["ln_depth.weight"])
        # 4. the depth Blocks: gd [B T, D, C], the gradient of the depth stream's input
        gd = _blocks_backward(W, G, "depth_transformer", Ld, Hd, g, sv["depth"], r, rnd is None).view(B, T, D, C)
        # 5. ln_spatial through slot 0
        dh = gd[:, :, 0]
        G["ln_spatial.weight"], G["ln_spatial.bias"] = (dh * sv["xhs"]).sum((0, 1)), dh.sum((0, 1))
        g = _ln_bwd(dh, sv["xhs"], sv["rss"], W["ln_spatial.weight"])
        # 6. the spatial Blocks: gs [B, T, C], the gradient of the spatial stream's input
        gs = _blocks_backward(W, G, "spatial_transformer", Ls, Hs, g, sv["spatial"], r, rnd is None)
        # 7. the embedding stage: d cs, then d emb by the transpose of the cumsum
        dcs = torch.zeros(B, T, D, C, dtype=torch.float64)
        dcs[:, :, :D - 1] = gd[:, :, 1:]
        dcs[:, :T - 1, D - 1] += gs[:, 1:]
        axis = {"channels": 3, "depth": 2}[code_sum]
        demb = dcs.flip(axis).cumsum(axis).flip(axis)
        G["tok_emb_code.weight"] = torch.zeros_like(W["tok_emb_code.weight"]).index_add_(0, codes.reshape(-1), demb.reshape(-1, C))
        G["tok_emb_cond.weight"] = torch.zeros_like(W["tok_emb_cond.weight"]).index_add_(0, conds[:, 0], gs[:, 0])
        G["pos_emb_code"] = torch.zeros_like(W["pos_emb_code"])
        G["pos_emb_code"][0, :T - 1] = gs[:, 1:].sum(0)
        G["pos_emb_depth"] = gd[:, :, 1:].sum((0, 1)).unsqueeze(0)
        G["pos_emb_cond"] = gs[:, :1].sum(0, keepdim=True)
    return loss, G, logits
