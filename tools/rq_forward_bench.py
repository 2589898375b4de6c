"""Times the stage-2 RQTransformer's teacher-forced forward at the shipped size (configs/imagenet_rqtransformer_rqvae_base.yaml: C = 1536, 24 spatial
and 4 depth layers, 12 heads of 128 in both, T = 1024, D = 4, V = 8192; random weights) and writes profiles/rq_forward.txt:
python tools/rq_forward_bench.py [--out FILE] [--spatial_layers N]

1. The depth attention alone at the shipped shape (NSEQ = batch x 1024 sequences of L = 4, 12 heads of 128), batch 1 and 4, fp16 and bf16: the
   short-sequence kernel (enh_short_causal_attention_forward) against the tile kernel (enh_causal_attention_forward at N = L) in the same run, the
   outputs compared; achieved bytes per second against the kernel's byte floor of 8 C bytes per token row (q, k, v read once, out written once).
2. The whole forward (fp16 operands), batch 1 and 4, against the same forward in plain fp16 torch (torch.addmm, F.layer_norm,
   F.scaled_dot_product_attention(is_causal=True)) on the model's own operand copies: ms and the forward's MFMA FLOP over the time.
Timing as tools/gpt_forward_bench.py: HIP events around a window of back-to-back calls; median, minimum and maximum of 5 windows that alternate
between the two paths, after a warm-up of both."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from enhancing import _C  # noqa: E402
from enhancing.modules.stage2.layers import RQTransformer  # noqa: E402
from gpt_forward_bench import ab  # noqa: E402


class TorchForward:
    """the yardstick: the same forward (code_sum="depth") in plain fp16 torch on the operand copies of the model"""

    def __init__(self, m):
        self.m = m
        self.ops = m._operand_copies(torch.float16)
        h = lambda p: None if p is None else p.detach().half()
        self.small = {id(k): (h(k.ln1.weight), h(k.ln1.bias), h(k.ln2.weight), h(k.ln2.bias), h(k.attn.proj.bias), h(k.mlp.p0.bias), h(k.mlp.p1.bias))
                      for k in list(m.spatial_transformer) + list(m.depth_transformer)}
        self.lns, self.lnd = (h(m.ln_spatial.weight), h(m.ln_spatial.bias)), (h(m.ln_depth.weight), h(m.ln_depth.bias))
        self.emb_c, self.pos_c = h(m.tok_emb_cond.weight), h(m.pos_emb_cond)[0, 0]
        self.emb, self.pos, self.pos_d = h(m.tok_emb_code.weight), h(m.pos_emb_code)[0], h(m.pos_emb_depth)[0]

    def blocks(self, x, stack, ops, H):
        n, S, C = x.shape
        for blk, W in zip(stack, ops):
            w1, b1, w2, b2, bp, b0, bq = self.small[id(blk)]
            tm, bqkv = W["time_mix"].half(), W["bqkv"].half()
            a = F.layer_norm(x, (C,), w1, b1)
            a = a * tm + F.pad(a, (0, 0, 1, -1)) * (1 - tm)
            q, k, v = torch.addmm(bqkv, a.view(n * S, C), W["wqkv"].t()).view(n, S, 3, H, C // H).permute(2, 0, 3, 1, 4)
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(n * S, C)
            x = x + torch.addmm(bp, y, W["wproj"].t()).view(n, S, C)
            hdn = torch.square(torch.relu(torch.addmm(b0, F.layer_norm(x, (C,), w2, b2).view(n * S, C), W["w0"].t())))
            x = x + torch.addmm(bq, hdn, W["w1"].t()).view(n, S, C)
        return x

    @torch.no_grad()
    def __call__(self, codes, conds):
        m = self.m
        C, B, T, D = m.embed_dim, codes.shape[0], m.img_num_tokens, m.depth_num_tokens
        cs = self.emb[codes].cumsum(2)
        x = torch.cat([(self.emb_c[conds[:, 0]] + self.pos_c)[:, None], cs[:, :T - 1, D - 1] + self.pos[:T - 1]], 1)
        hsp = F.layer_norm(self.blocks(x, m.spatial_transformer, self.ops["spatial"], m.spatial_n_heads), (C,), *self.lns)
        v = torch.cat([hsp.unsqueeze(2), cs[:, :, :D - 1] + self.pos_d], 2).reshape(B * T, D, C)
        v = self.blocks(v, m.depth_transformer, self.ops["depth"], m.depth_n_heads)
        return torch.matmul(F.layer_norm(v, (C,), *self.lnd), self.ops["head"].t()).float()


def forward_flop(b, C, V, T, D, Ls, Ld, Hs, Hd):
    """MFMA FLOP of one forward: 12 C^2 multiply-adds per row and Block, the head, and the two attentions on their lower triangles"""
    gemm = 2.0 * 12 * C * C * b * T * (Ls + D * Ld) + 2.0 * V * C * b * T * D
    return gemm + Ls * 2.0 * b * Hs * T * (T + 1) * (C // Hs) + Ld * 2.0 * b * T * Hd * D * (D + 1) * (C // Hd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rq_forward.txt"))
    ap.add_argument("--spatial_layers", type=int, default=24)
    args = ap.parse_args()
    C, H, V, T, D, Ls, Ld = 1536, 12, 8192, 1024, 4, args.spatial_layers, 4
    hs = C // H
    f3 = lambda v, k=1.0: f"{v[1] * k:.1f} [{v[0] * k:.1f} .. {v[2] * k:.1f}]"
    lines = [f"stage-2 RQTransformer forward on {torch.cuda.get_device_name(0)}: C={C} spatial layers={Ls} depth layers={Ld} heads={H} x {hs} T={T} D={D} V={V}",
             "times: median [min .. max] of 5 alternating windows of back-to-back calls, after a warm-up of both paths",
             f"depth attention alone, NSEQ = batch x {T} sequences of L = {D}, H = {H}, Dh = {hs}: windows of 200 launches; byte floor 8 C = {8 * C} bytes per token row",
             f"{'batch':>5} {'fmt':>5} {'short us [min .. max]':>28} {'tile us [min .. max]':>28} {'tile/short':>10} {'spread-free':>11} {'short GB/s':>10} {'max |diff|':>10}"]
    all_faster = True
    for b in (1, 4):
        for dt, fmt in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
            nseq = b * T
            qkv = (torch.randn(nseq, D, 3 * C, device="cuda") * 1.5).to(dt)
            o_s, o_t = torch.empty(nseq, D, C, device="cuda", dtype=dt), torch.empty(nseq, D, C, device="cuda", dtype=dt)
            s, t = ab(lambda i: _C.short_causal_attention(qkv, nseq, D, H, hs, o_s), lambda i: _C.causal_attention(qkv, nseq, D, H, hs, o_t), inner=200)
            faster = s[2] < t[0]      # the slowest window of the new kernel against the fastest of the old one: beyond the spread of both
            all_faster &= faster
            lines.append(f"{b:>5} {fmt:>5} {f3(s, 1e3):>28} {f3(t, 1e3):>28} {t[1] / s[1]:>10.2f} {'yes' if faster else 'NO':>11} "
                         f"{8.0 * C * nseq * D / (s[1] * 1e-3) / 1e9:>10.0f} {(o_s.float() - o_t.float()).abs().max().item():>10.1e}")
    lines.append(f"short kernel faster than the tile kernel beyond the run-to-run spread at every point: {'yes' if all_faster else 'NO'}")
    lines.append(f"(a window relaunches over the same buffers, {8 * C * T * D / 1e6:.0f} MB per unit of batch: they fit the 256 MiB last-level cache, so the rates are "
                 "cache-assisted and can pass the HBM rate)")
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(vocab_cond_size=1000, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, depth_num_tokens=D,
                          spatial_n_heads=H, depth_n_heads=H, spatial_n_layers=Ls, depth_n_layers=Ld)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    tf = TorchForward(m)
    lines += ["whole forward, fp16 operands: windows of 10 calls",
              f"{'batch':>5} {'device ms [min .. max]':>30} {'torch ms [min .. max]':>30} {'torch/dev':>9} {'TFLOP':>7} {'device TF/s':>11} {'rel diff':>9}"]
    for b in (1, 4):
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        conds = torch.randint(0, 1000, (b, 1), device="cuda")
        ref = tf(codes, conds).view(b * T, D, V)
        diff = ((m(codes, conds) - ref).norm() / ref.norm()).item()
        d, r = ab(lambda i: m(codes, conds), lambda i: tf(codes, conds), inner=10)
        flop = forward_flop(b, C, V, T, D, Ls, Ld, H, H)
        lines.append(f"{b:>5} {f3(d):>30} {f3(r):>30} {r[1] / d[1]:>9.2f} {flop / 1e12:>7.2f} {flop / d[1] / 1e9:>11.0f} {diff:>9.1e}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
