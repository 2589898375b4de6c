"""The cases of the stage-2 GPT's teacher-forced forward: the three sampling cases of tests/gpt_cases.py and two whose sequences span more than one
key tile and query block of the causal attention kernel (`long`: 200 rows, two batch elements; `long3`: 131 rows, three heads of 64, two layers).
Shared by tools/make_golden_gpt_forward.py (which runs the REFERENCE's GPT.forward on them and writes tests/golden/gpt_fwd_<case>.npz) and
tests/test_gpt_forward_*.py.  Parameters and inputs are gpt_cases.make_params / make_inputs.

`forward_logits` is a plain-torch restatement of the reference's GPT.forward with one condition token, built on S = T rows (the condition and the
first T - 1 codes: the causal mask keeps the last code's row from every logit that is kept).  With rnd=None it is the fp32 / fp64 statement of the
model; with rnd = a 16-bit rounding it has the rounding points of the device path: every GEMM operand, q / k / v and the softmax numerators rounded
to the format, products in `prod`, everything else in `work`."""
import math

import torch

import gpt_cases as GC
from gpt_cases import PARAM_SEED, VOCAB_COND, make_inputs, make_params  # noqa: F401

#                          name     C  heads layers  V    T  B
CASES = dict(GC.CASES, long=(128, 2, 1, 64, 200, 2), long3=(192, 3, 2, 48, 131, 1))


def case_kwargs(name: str) -> dict:
    C, H, L, V, T, _ = CASES[name]
    return dict(vocab_cond_size=VOCAB_COND, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, n_heads=H, n_layers=L)


def case_inputs(name: str):
    """(conds [B, 1] int64, codes [B, T] int64): gpt_cases.make_inputs with this module's case table"""
    import numpy as np
    _, _, _, V, T, B = CASES[name]
    rs = np.random.RandomState(GC.INPUT_SEED + len(name))
    conds = torch.from_numpy(rs.randint(0, VOCAB_COND, size=(B, 1)).astype(np.int64))
    codes = torch.from_numpy(rs.randint(0, V, size=(B, T)).astype(np.int64))
    return conds, codes


def forward_logits(P: dict, name: str, conds: torch.Tensor, codes: torch.Tensor, rnd=None, prod=torch.float64, work=torch.float32):
    """logits [B, T, V] (`work` dtype) of the teacher-forced forward; P on the device the computation should run on"""
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

    conds, codes = conds.to(dev).view(B, -1), codes.to(dev).view(B, -1)
    S = T
    x = torch.cat([W["tok_emb_cond.weight"][conds[:, :1]] + W["pos_emb_cond"][:, :1],
                   W["tok_emb_code.weight"][codes[:, :S - 1]] + W["pos_emb_code"][:, :S - 1]], 1)
    causal = torch.ones(S, S, dtype=torch.bool, device=dev).tril()
    for i in range(L):
        pre = f"blocks.{i}."
        tm = W[pre + "attn.time_mix"].reshape(-1)
        a = ln(x, pre + "ln1")
        prev = torch.cat([torch.zeros_like(a[:, :1]), a[:, :-1]], 1)      # time_shift: per batch element, row -1 is zero
        a = a * tm + prev * (1 - tm)
        wqkv = torch.cat([W[pre + "attn.query.weight"], W[pre + "attn.key.weight"], W[pre + "attn.value.weight"]], 0)
        bqkv = torch.cat([W[pre + "attn.query.bias"], W[pre + "attn.key.bias"], W[pre + "attn.value.bias"]])
        qkv = r(mm(a.reshape(B * S, C), wqkv) + bqkv)
        q, k, v = (z.reshape(B, S, H, hs).permute(0, 2, 1, 3).to(prod) for z in qkv.split(C, dim=1))
        s = (q @ k.transpose(-1, -2)).to(work) * (1.0 / math.sqrt(hs))
        s = s.masked_fill(~causal, float("-inf"))
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))
        y = ((r(e).to(prod) @ v).to(work) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B * S, C)
        x = x + (mm(y, W[pre + "attn.proj.weight"]) + W[pre + "attn.proj.bias"]).view(B, S, C)
        hdn = torch.square(torch.relu(mm(ln(x, pre + "ln2").reshape(B * S, C), W[pre + "mlp.p0.weight"]) + W[pre + "mlp.p0.bias"]))
        x = x + (mm(hdn, W[pre + "mlp.p1.weight"]) + W[pre + "mlp.p1.bias"]).view(B, S, C)
    return mm(ln(x, "layer_norm").reshape(B * S, C), W["head.weight"]).view(B, T, V)
