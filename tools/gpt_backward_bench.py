"""Times GPT.forward_backward at the shipped width (configs/imagenet_gpt_vitvq_base.yaml: C = 6144, 16 heads of 384, T = 1024, V = 8192; random weights,
fp16 operands) and writes profiles/gpt_backward.txt:  python tools/gpt_backward_bench.py [--out FILE] [--layers N] [--full-depth]

--layers defaults to 2: the run then takes seconds and a few GB.  --full-depth adds one row of the device path alone at the shipped 24 layers
(about 110 GB: f32 masters, operand copies and the flat gradient), skipped with a note when the memory is not there.

Per batch size (1 | 4): ms per forward_backward and per step of the yardstick, the same model in plain fp16 torch with autograd (torch.addmm,
F.layer_norm, F.scaled_dot_product_attention(is_causal=True), F.cross_entropy, loss.backward()), alternating inside this process: median [min .. max]
of 5 windows, after a warm-up of both; and the call's MFMA FLOP (3 x the forward's products, the attention's 2 + 5 products on the triangle) over the
time: an end-to-end rate, not a kernel's share of peak.
Then every kernel of one forward_backward at batch 4 (KernelTimer: HIP events around each launch, which also adds the launch gaps to short kernels): time, the
algorithmic FLOP or bytes the binding states, and the rate against the MFMA ceiling (fp16 dense: 16 x the 157.3 TFLOP/s f32 matrix rate = 2517) or the
HBM ceiling (8.0 TB/s spec; a float4 copy reaches 6.29).
Then each new kernel alone against what torch runs for the same step at the shipped shape, batch 4."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from enhancing import _C  # noqa: E402
from enhancing.modules.stage2.layers import GPT  # noqa: E402
from gpt_forward_bench import ab  # noqa: E402

MFMA_PEAK, HBM_PEAK = 16 * 157.3e12, 8.0e12


class TorchStep:
    """the yardstick: the same model as fp16 leaves with autograd"""

    def __init__(self, m):
        self.m = m
        h = lambda p: p.detach().half().requires_grad_(True)
        self.P = {k: h(p) for k, p in m.named_parameters()}

    def __call__(self, codes, conds):
        m, P = self.m, self.P
        C, H, B, S, V = m.embed_dim, m.n_heads, codes.shape[0], m.img_num_tokens, m.vocab_img_size
        hs = C // H
        for p in P.values():
            p.grad = None
        x = torch.cat([(P["tok_emb_cond.weight"][conds[:, 0]] + P["pos_emb_cond"][0, 0])[:, None], P["tok_emb_code.weight"][codes[:, :S - 1]] + P["pos_emb_code"][0, :S - 1]], 1)
        for i in range(len(m.blocks)):
            g = lambda n: P[f"blocks.{i}.{n}"]
            tm = g("attn.time_mix").view(-1)
            a = F.layer_norm(x, (C,), g("ln1.weight"), g("ln1.bias"))
            a = (a * tm + F.pad(a, (0, 0, 1, -1)) * (1 - tm)).view(B * S, C)
            q, k, v = (torch.addmm(g(f"attn.{n}.bias"), a, g(f"attn.{n}.weight").t()).view(B, S, H, hs).transpose(1, 2) for n in ("query", "key", "value"))
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B * S, C)
            x = x + torch.addmm(g("attn.proj.bias"), y, g("attn.proj.weight").t()).view(B, S, C)
            hdn = torch.square(torch.relu(torch.addmm(g("mlp.p0.bias"), F.layer_norm(x, (C,), g("ln2.weight"), g("ln2.bias")).view(B * S, C), g("mlp.p0.weight").t())))
            x = x + torch.addmm(g("mlp.p1.bias"), hdn, g("mlp.p1.weight").t()).view(B, S, C)
        logits = torch.matmul(F.layer_norm(x, (C,), P["layer_norm.weight"], P["layer_norm.bias"]), P["head.weight"].t())
        loss = F.cross_entropy(logits.float().view(-1, V), codes.reshape(-1))
        (loss * 1024.0).backward()
        return loss.detach()


def build(L, C, H, V, T):
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = GPT(vocab_cond_size=1000, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, n_heads=H, n_layers=L)
        with torch.no_grad():
            m.pos_emb_code.normal_(0, 0.02)
    return m


def step_flop(b, T, C, H, V, L):
    """MFMA FLOP of one forward_backward in an unsplit attention: every dense product three times (forward, input gradient, weight gradient), the
    causal attention's two forward and five backward products on the lower triangle"""
    return 3 * b * T * (2.0 * 12 * C * C * L + 2.0 * V * C) + L * (2.0 + 5.0) * b * H * T * (T + 1) * (C // H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_backward.txt"))
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--full-depth", action="store_true")
    args = ap.parse_args()
    C, H, V, T, L = 6144, 16, 8192, 1024, args.layers
    f3 = lambda v: f"{v[1]:.2f} [{v[0]:.2f} .. {v[2]:.2f}]"
    m = build(L, C, H, V, T)
    lines = [f"stage-2 forward_backward on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} x {C // H} T={T} V={V}, fp16 operands, loss_scale 1024",
             "times: median [min .. max] ms of 5 alternating windows of 2 back-to-back calls, after a warm-up of both paths",
             f"{'batch':>5} {'device ms [min .. max]':>30} {'torch ms [min .. max]':>30} {'torch/dev':>9} {'TFLOP':>7} {'device TF/s':>11} {'loss dev / torch':>20} {'rel diff dW_head':>17}"]
    ts = TorchStep(m)
    data = {}
    for b in (1, 4):
        codes = torch.randint(0, V, (b, T), device="cuda")
        conds = torch.randint(0, 1000, (b, 1), device="cuda")
        data[b] = (codes, conds)
        ld, lt = m.forward_backward(codes, conds, loss_scale=1024.0).item(), ts(codes, conds).item()
        gd, gt = m.head.weight.grad.double(), ts.P["head.weight"].grad.double()
        diff = ((gd - gt).norm() / gt.norm()).item()
        d, r = ab(lambda i: m.forward_backward(codes, conds, loss_scale=1024.0), lambda i: ts(codes, conds), inner=2)
        flop = step_flop(b, T, C, H, V, L)
        lines.append(f"{b:>5} {f3(d):>30} {f3(r):>30} {r[1] / d[1]:>9.2f} {flop / 1e12:>7.1f} {flop / d[1] / 1e9:>11.0f} {ld:>9.4f} / {lt:<8.4f} {diff:>17.1e}")
    del ts
    torch.cuda.empty_cache()

    # ---- every kernel of one call at batch 4 -----------------------------------------------------------------------------------------------------
    codes, conds = data[4]
    timer = _C.KernelTimer()
    _C.TIMER = timer
    try:
        m.forward_backward(codes, conds, loss_scale=1024.0)
    finally:
        _C.TIMER = None
    lines.append(f"kernels of one forward_backward at batch 4, {L} layers (HIP events around each launch; calls the binding does not time are not listed):")
    lines.append(f"  {'kernel':<58} {'launches':>8} {'total ms':>9} {'work':>12} {'rate':>12} {'of ceiling':>10}")
    for name, s in sorted(timer.summary().items(), key=lambda kv: -kv[1]["total_ms"]):
        rate = s["work"] / (s["total_ms"] * 1e-3)
        if s["unit"] == "byte":
            lines.append(f"  {name:<58} {s['launches']:>8} {s['total_ms']:>9.3f} {s['work'] / 1e9:>9.2f} GB {rate / 1e12:>7.2f} TB/s {100 * rate / HBM_PEAK:>8.1f} % HBM")
        else:
            lines.append(f"  {name:<58} {s['launches']:>8} {s['total_ms']:>9.3f} {s['work'] / 1e12:>9.3f} TF {rate / 1e12:>7.0f} TF/s {100 * rate / MFMA_PEAK:>8.1f} % MFMA")
    m._bwd_states = {}
    torch.cuda.empty_cache()

    # ---- each new kernel against torch's step, batch 4 -----------------------------------------------------------------------------------------
    b, M, hs = 4, 4 * T, C // H
    lines.append("new kernels alone against torch's same step (fp16, batch 4, the shipped shape): us median [min .. max] of 5 windows of 10 launches")
    us = lambda v: f"{v[1] * 1e3:9.1f} [{v[0] * 1e3:.1f} .. {v[2] * 1e3:.1f}]"

    def row(name, dev, ref, note=""):
        d, r = ab(dev, ref, inner=10)
        lines.append(f"  {name:<34} device {us(d)} us   torch {us(r)} us   torch/device {r[1] / d[1]:5.2f}{note}")

    qkv = (torch.randn(b, T, 3 * C, device="cuda") * 0.5).half()
    out, lse, do, dqkv = torch.empty(b, T, C, device="cuda").half(), torch.empty(b, H, T, device="cuda"), torch.randn(b, T, C, device="cuda").half(), torch.empty_like(qkv)
    _C.causal_attention(qkv, b, T, H, hs, out, lse)
    q, k, v = (t.detach().requires_grad_(True) for t in qkv.view(b, T, 3, H, hs).permute(2, 0, 3, 1, 4))
    y = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    gy = do.view(b, T, H, hs).transpose(1, 2)
    row("causal attention backward", lambda i: _C.causal_attention_backward(qkv, out, do, lse, b, T, H, hs, dqkv),
        lambda i: torch.autograd.grad(y, (q, k, v), gy, retain_graph=True), "   (torch: the backward of scaled_dot_product_attention alone)")
    del q, k, v, y, gy, qkv, out, do, dqkv
    logits = torch.randn(M, V, device="cuda")
    tgt = torch.randint(0, V, (M,), device="cuda")
    nll, dl = torch.empty(M, device="cuda"), torch.empty(M, V, device="cuda").half()
    lg = logits.clone().requires_grad_(True)

    def torch_ce(i):
        lg.grad = None
        F.cross_entropy(lg, tgt).backward()
        return lg.grad.half()
    row("cross-entropy + dlogits", lambda i: _C.cross_entropy_backward(logits, tgt, nll, dl, 1.0 / M), torch_ce, "   (torch: f32 cross_entropy forward + backward, cast)")
    del logits, lg, dl
    dy, yh, dx = torch.randn(M, 4 * C, device="cuda"), torch.rand(M, 4 * C, device="cuda").half(), torch.empty(M, 4 * C, device="cuda").half()
    row("relu^2 backward", lambda i: _C.relu_sq_backward(dy, yh, dx), lambda i: (dy * (2.0 * torch.sqrt(yh.float()))).half())
    del dy, yh, dx
    x, g = torch.randn(M, C, device="cuda"), torch.randn(M, C, device="cuda")
    w, bb, tm = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), torch.rand(C, device="cuda")
    dxo, dx16, dw, db, dtm = torch.empty_like(x), torch.empty(M, C, device="cuda").half(), torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    xr, wr, br, tr = (t.clone().requires_grad_(True) for t in (x, w, bb, tm))

    def torch_ln(mix):
        def f(i):
            a = F.layer_norm(xr.view(b, T, C), (C,), wr, br)
            if mix:
                a = a * tr + F.pad(a, (0, 0, 1, -1)) * (1 - tr)
            return torch.autograd.grad(a, (xr, wr, br) + ((tr,) if mix else ()), g.view(b, T, C))
        return f
    row("LayerNorm backward (ln2)", lambda i: _C.ln_timeshift_backward(g, x, w, T, dxo, dw, db, dres=g, dx16=dx16), torch_ln(False), "   (torch: f32 forward + backward)")
    row("LayerNorm + time-shift backward", lambda i: _C.ln_timeshift_backward(g, x, w, T, dxo, dw, db, b=bb, colscale=tm, dcolscale=dtm, dres=g, dx16=dx16), torch_ln(True),
        "   (torch: f32 forward + backward)")
    codes, conds = data[4]
    tabs = [torch.empty(1000, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(V, C, device="cuda"), torch.empty(T, C, device="cuda")]
    gv = g.view(b, T, C)

    def torch_emb(i):
        return (torch.zeros(V, C, device="cuda").index_add_(0, codes[:, :T - 1].reshape(-1), gv[:, 1:].reshape(-1, C)),
                torch.zeros(1000, C, device="cuda").index_add_(0, conds[:, 0], gv[:, 0]), gv[:, 1:].sum(0), gv[:, 0].sum(0))
    row("embedding backward", lambda i: _C.gpt_embed_seq_backward(gv, conds[:, 0].contiguous(), codes, *tabs), torch_emb, "   (torch: index_add_ with atomics, two sums)")
    del x, g, xr, dxo, dx16, tabs
    del m
    torch.cuda.empty_cache()

    if args.full_depth:
        try:
            m = build(24, C, H, V, T)
            for b in (1, 4):
                codes, conds = data[b]
                d, _ = ab(lambda i: m.forward_backward(codes, conds, loss_scale=1024.0), lambda i: None, inner=2)
                flop = step_flop(b, T, C, H, V, 24)
                lines.append(f"full depth, 24 layers, device path alone, batch {b}: {f3(d)} ms, {flop / 1e12:.1f} TFLOP, {flop / d[1] / 1e9:.0f} TF/s end to end; "
                             f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB allocated at most")
        except torch.OutOfMemoryError as e:
            lines.append(f"full depth, 24 layers: not measured, the device's free memory did not hold it ({str(e).splitlines()[0][:120]})")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
