"""Times the stage-2 RQTransformer's training at the shipped size (configs/imagenet_rqtransformer_rqvae_base.yaml: C = 1536, 24 spatial and 4 depth
layers, 12 heads of 128 in both, T = 1024, D = 4, V = 8192; random weights) and writes profiles/rq_backward.txt:
python tools/rq_train_bench.py [--out FILE] [--spatial_layers N]

1. The depth attention's backward alone at the shipped shape (NSEQ = batch x 1024 sequences of L = 4, 12 heads of 128), batch 1 and 4, fp16 and bf16:
   the short-sequence kernel (enh_short_causal_attention_backward) against the tile kernels (enh_causal_attention_backward at N = L) in the same run.
2. RQTransformer.forward_backward (fp16 operands), batch 1 and 4, against the plain fp16 torch autograd of tools/rq_forward_bench.py's restatement on
   the model's own operand copies (F.cross_entropy(...).backward()), and the three new kernels alone at the shapes the step launches them with: their
   share of the step.
3. forward_backward with the optimizer's device loss scale + GPTAdam.step, the same batches.
Timing as tools/rq_forward_bench.py: median [min .. max] of 5 alternating windows of back-to-back calls, after a warm-up of both paths."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from enhancing import _C  # noqa: E402
from enhancing.engine.optim import GPTAdam  # noqa: E402
from enhancing.modules.stage2.layers import RQTransformer  # noqa: E402
from gpt_forward_bench import ab  # noqa: E402
from rq_forward_bench import TorchForward  # noqa: E402


class TorchTraining(TorchForward):
    """the yardstick: rq_forward_bench.TorchForward with every fp16 operand a leaf that requires a gradient, F.cross_entropy and autograd"""

    def __init__(self, m):
        super().__init__(m)
        leaf = lambda t: t.detach().clone().requires_grad_(True) if torch.is_tensor(t) and t.is_floating_point() else t
        self.ops = {k: [{n: leaf(t) for n, t in W.items()} for W in v] if isinstance(v, list) else leaf(v) for k, v in self.ops.items()}
        self.small = {k: tuple(leaf(t) for t in v) for k, v in self.small.items()}
        self.lns, self.lnd = tuple(leaf(t) for t in self.lns), tuple(leaf(t) for t in self.lnd)
        self.emb_c, self.pos_c, self.emb, self.pos, self.pos_d = (leaf(t) for t in (self.emb_c, self.pos_c, self.emb, self.pos, self.pos_d))
        self.leaves = [t for v in self.ops.values() for W in (v if isinstance(v, list) else [{"": v}]) for t in W.values() if torch.is_tensor(t) and t.requires_grad]
        self.leaves += [t for v in self.small.values() for t in v] + list(self.lns) + list(self.lnd) + [self.emb_c, self.pos_c, self.emb, self.pos, self.pos_d]

    def step(self, codes, conds):
        for t in self.leaves:
            t.grad = None
        with torch.enable_grad():
            logits = TorchForward.__call__.__wrapped__(self, codes, conds)
            loss = F.cross_entropy(logits.view(-1, logits.shape[-1]), codes.reshape(-1))
            loss.backward()
        return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rq_backward.txt"))
    ap.add_argument("--spatial_layers", type=int, default=24)
    args = ap.parse_args()
    C, H, V, T, D, Ls, Ld = 1536, 12, 8192, 1024, 4, args.spatial_layers, 4
    hs = C // H
    f3 = lambda v, k=1.0: f"{v[1] * k:.1f} [{v[0] * k:.1f} .. {v[2] * k:.1f}]"
    lines = [f"stage-2 RQTransformer training on {torch.cuda.get_device_name(0)}: C={C} spatial layers={Ls} depth layers={Ld} heads={H} x {hs} T={T} D={D} V={V}",
             "times: median [min .. max] of 5 alternating windows of back-to-back calls, after a warm-up of both paths",
             f"1. depth attention backward alone, NSEQ = batch x {T} sequences of L = {D}, H = {H}, Dh = {hs}: windows of 200 launches; byte floor 16 C = {16 * C} bytes per token row",
             f"{'batch':>5} {'fmt':>5} {'short us [min .. max]':>28} {'tile us [min .. max]':>28} {'tile/short':>10} {'spread-free':>11} {'short GB/s':>10} {'max |diff|':>10}"]
    all_faster = True
    for b in (1, 4):
        for dt, fmt in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
            nseq = b * T
            qkv = (torch.randn(nseq, D, 3 * C, device="cuda") * 1.5).to(dt)
            do = torch.randn(nseq, D, C, device="cuda").to(dt)
            out, lse = torch.empty(nseq, D, C, device="cuda", dtype=dt), torch.empty(nseq, H, D, device="cuda")
            _C.short_causal_attention(qkv, nseq, D, H, hs, out, lse)
            g_s, g_t = torch.empty_like(qkv), torch.empty_like(qkv)
            s, t = ab(lambda i: _C.short_causal_attention_backward(qkv, out, do, lse, nseq, D, H, hs, g_s),
                      lambda i: _C.causal_attention_backward(qkv, out, do, lse, nseq, D, H, hs, g_t), inner=200)
            faster = s[2] < t[0]      # the slowest window of the new kernel against the fastest of the old ones: beyond the spread of both
            all_faster &= faster
            lines.append(f"{b:>5} {fmt:>5} {f3(s, 1e3):>28} {f3(t, 1e3):>28} {t[1] / s[1]:>10.2f} {'yes' if faster else 'NO':>11} "
                         f"{16.0 * C * nseq * D / (s[1] * 1e-3) / 1e9:>10.0f} {(g_s.float() - g_t.float()).abs().max().item():>10.1e}")
    lines.append(f"short kernel faster than the tile kernels beyond the run-to-run spread at every point: {'yes' if all_faster else 'NO'}")
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(vocab_cond_size=1000, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, depth_num_tokens=D,
                          spatial_n_heads=H, depth_n_heads=H, spatial_n_layers=Ls, depth_n_layers=Ld)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    tt = TorchTraining(m)
    lines += ["2. forward_backward, fp16 operands, loss scale 1024: windows of 5 calls; the new kernels alone at the step's shapes: windows of 50 launches",
              f"{'batch':>5} {'device ms [min .. max]':>30} {'torch autograd ms [min .. max]':>32} {'torch/dev':>9} {'loss dev':>9} {'loss torch':>10}"]
    shares = []
    for b in (1, 4):
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        conds = torch.randint(0, 1000, (b, 1), device="cuda")
        ld, lt = m.forward_backward(codes, conds, loss_scale=1024.0).item(), tt.step(codes, conds).item()
        d, r = ab(lambda i: m.forward_backward(codes, conds, loss_scale=1024.0), lambda i: tt.step(codes, conds), inner=5)
        lines.append(f"{b:>5} {f3(d):>30} {f3(r):>32} {r[1] / d[1]:>9.2f} {ld:>9.4f} {lt:>10.4f}")
        # the three new kernels at this batch
        Ms, M = b * T, b * T * D
        qkv, do = torch.randn(Ms, D, 3 * C, device="cuda").half(), torch.randn(Ms, D, C, device="cuda").half()
        out, lse, dq = torch.empty(Ms, D, C, device="cuda", dtype=torch.float16), torch.empty(Ms, H, D, device="cuda"), torch.empty_like(qkv)
        _C.short_causal_attention(qkv, Ms, D, H, hs, out, lse)
        g, xs, w = torch.randn(M, C, device="cuda"), torch.randn(Ms, C, device="cuda"), torch.ones(C, device="cuda")
        dx, dx16, dw, db = torch.empty(Ms, C, device="cuda"), torch.empty(Ms, C, device="cuda", dtype=torch.float16), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        gs = torch.randn(b, T, C, device="cuda")
        tabs = [torch.empty_like(p).view(-1, C) for p in (m.tok_emb_cond.weight, m.pos_emb_cond, m.tok_emb_code.weight, m.pos_emb_code, m.pos_emb_depth)]
        tabs[1] = tabs[1].view(-1)
        ka, kl = ab(lambda i: _C.short_causal_attention_backward(qkv, out, do, lse, Ms, D, H, hs, dq),
                    lambda i: _C.ln_rows_strided_backward(g, D * C, xs, w, dx, dw, db, dx16=dx16), inner=50)
        ke, _ = ab(lambda i: _C.rq_embed_seq_backward(gs, g.view(Ms, D, C), conds.view(-1), codes, *tabs), lambda i: None, inner=50)
        shares.append(f"{b:>5} short attention backward {ka[1] * 1e3:.1f} us x {Ld} = {100 * Ld * ka[1] / d[1]:.2f} %, strided LayerNorm backward {kl[1] * 1e3:.1f} us = "
                      f"{100 * kl[1] / d[1]:.2f} %, embedding backward {ke[1] * 1e3:.1f} us = {100 * ke[1] / d[1]:.2f} % of the step")
    lines += ["   the new kernels' share of forward_backward (median us per launch):"] + shares
    opt = GPTAdam(m, lr=1e-4)
    lines += ["3. forward_backward with the device loss scale + GPTAdam.step: windows of 5 steps (second column: GPTAdam.step alone, windows of 5)",
              f"{'batch':>5} {'training step ms [min .. max]':>32} {'GPTAdam.step ms [min .. max]':>32}"]
    for b in (1, 4):
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        conds = torch.randint(0, 1000, (b, 1), device="cuda")

        def train(i):
            m.forward_backward(codes, conds, loss_scale=opt.loss_scale)
            opt.step()
        tr, st = ab(train, lambda i: opt.step(), inner=5)
        lines.append(f"{b:>5} {f3(tr):>32} {f3(st):>32}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
