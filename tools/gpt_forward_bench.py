"""Times the stage-2 teacher-forced forward at the shipped size (configs/imagenet_gpt_vitvq_base.yaml: C = 6144, 24 layers, 16 heads of 384, T = 1024,
V = 8192; random weights) and writes profiles/gpt_forward.txt:  python tools/gpt_forward_bench.py [--out FILE] [--layers N]

Per batch size (1 | 4): ms per GPT.forward (fp16 operands) and per call of the same forward in plain fp16 torch (torch.addmm, F.layer_norm,
F.scaled_dot_product_attention(is_causal=True)) on the model's own operand copies, alternating inside this process; and the forward's MFMA FLOP over
the time.  Then the causal attention kernel alone at the shipped head shape against enh_attention_forward_dh at D = 128 on the same N and the same
C = H D: time per EXECUTED MFMA FLOP (the causal kernel's own count: only the tiles on and below a wave's diagonal, the score product once per V slice).
Timing as tools/gpt_sample_bench.py: HIP events around a window of back-to-back calls, median, minimum and maximum of 5 windows that alternate
between the two paths, after a warm-up."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
from enhancing import _C  # noqa: E402
from enhancing.modules.stage2.layers import GPT  # noqa: E402


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(inner):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def ab(fa, fb, inner, reps=5):
    """(min, median, max) ms per call of fa and of fb: `reps` alternating windows of `inner` back-to-back calls each, after a warm-up of both"""
    fa(0); fb(0)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa, inner))
        tb.append(timed(fb, inner))
    st = lambda v: (min(v), statistics.median(v), max(v))
    return st(ta), st(tb)


class TorchForward:
    """the yardstick: the same forward in plain fp16 torch on the operand copies of the model"""

    def __init__(self, m):
        self.m = m
        self.ops = m._operand_copies(torch.float16)
        h = lambda p: None if p is None else p.detach().half()
        self.ln = [(h(k.ln1.weight), h(k.ln1.bias), h(k.ln2.weight), h(k.ln2.bias), h(k.attn.proj.bias), h(k.mlp.p0.bias), h(k.mlp.p1.bias)) for k in m.blocks]
        self.lnf = (h(m.layer_norm.weight), h(m.layer_norm.bias))
        self.tm = [W["time_mix"].half() for W in self.ops["layers"]]
        self.bqkv = [W["bqkv"].half() for W in self.ops["layers"]]
        self.emb_c, self.pos_c = h(m.tok_emb_cond.weight), h(m.pos_emb_cond)[0, 0]
        self.emb, self.pos = h(m.tok_emb_code.weight), h(m.pos_emb_code)[0]

    @torch.no_grad()
    def __call__(self, codes, conds):
        m = self.m
        C, H, B, S = m.embed_dim, m.n_heads, codes.shape[0], m.img_num_tokens
        hs = C // H
        x = torch.cat([(self.emb_c[conds[:, 0]] + self.pos_c)[:, None], self.emb[codes[:, :S - 1]] + self.pos[:S - 1]], 1)
        for W, (w1, b1, w2, b2, bp, b0, bq), tm, bqkv in zip(self.ops["layers"], self.ln, self.tm, self.bqkv):
            a = F.layer_norm(x, (C,), w1, b1)
            a = a * tm + F.pad(a, (0, 0, 1, -1)) * (1 - tm)
            qkv = torch.addmm(bqkv, a.view(B * S, C), W["wqkv"].t()).view(B, S, 3, H, hs)
            q, k, v = qkv.permute(2, 0, 3, 1, 4)
            y = F.scaled_dot_product_attention(q, k, v, is_causal=True).transpose(1, 2).reshape(B * S, C)
            x = x + torch.addmm(bp, y, W["wproj"].t()).view(B, S, C)
            hdn = torch.square(torch.relu(torch.addmm(b0, F.layer_norm(x, (C,), w2, b2).view(B * S, C), W["w0"].t())))
            x = x + torch.addmm(bq, hdn, W["w1"].t()).view(B, S, C)
        return torch.matmul(F.layer_norm(x, (C,), *self.lnf), self.ops["head"].t()).float()


def causal_executed_flop(B, N, H, D):
    """MFMA FLOP the causal kernel executes: per wave (32 queries at q0) the tiles 0 .. q0 / 64 of 64 keys, the score product over D and P V over its
    slice's DV columns, once per slice"""
    dv = D if D <= 128 else D // 2
    tiles = sum(q0 // 64 + 1 for q0 in range(0, N, 32))
    return B * H * (D // dv) * tiles * 2.0 * 32 * 64 * (D + dv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_forward.txt"))
    ap.add_argument("--layers", type=int, default=24)
    args = ap.parse_args()
    C, H, V, T, L = 6144, 16, 8192, 1024, args.layers
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = GPT(vocab_cond_size=1000, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, n_heads=H, n_layers=L)
        with torch.no_grad():
            m.pos_emb_code.normal_(0, 0.02)
    f3 = lambda v: f"{v[1]:.2f} [{v[0]:.2f} .. {v[2]:.2f}]"
    lines = [f"stage-2 teacher-forced forward on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} x {C // H} T={T} V={V}, fp16 operands",
             "times: median [min .. max] ms of 5 alternating windows of 2 back-to-back calls, after a warm-up of both paths",
             f"{'batch':>5} {'device ms [min .. max]':>30} {'torch ms [min .. max]':>30} {'torch/dev':>9} {'TFLOP':>7} {'device TF/s':>11} {'rel diff':>9}"]
    tf = TorchForward(m)
    worst = 0.0
    for b in (1, 4):
        codes = torch.randint(0, V, (b, T), device="cuda")
        conds = torch.randint(0, 1000, (b, 1), device="cuda")
        diff = ((m(codes, conds) - tf(codes, conds)).norm() / tf(codes, conds).norm()).item()
        d, r = ab(lambda i: m(codes, conds), lambda i: tf(codes, conds), inner=2)
        flop = b * T * (2.0 * 12 * C * C * L + 2.0 * V * C) + L * 2.0 * b * H * T * (T + 1) * (C // H)
        worst = max(worst, d[1] / r[1])
        lines.append(f"{b:>5} {f3(d):>30} {f3(r):>30} {r[1] / d[1]:>9.2f} {flop / 1e12:>7.1f} {flop / d[1] / 1e9:>11.0f} {diff:>9.1e}")
    lines.append(f"device / torch (medians), worse of the two points: {worst:.3f} (the goal is <= 1)")
    del tf
    m._fwd_states = {}
    torch.cuda.empty_cache()
    lines.append("attention kernels alone (fp16), N = 1024, C = H D = 6144: us median [min .. max] of 5 windows of 20 launches; us per executed MFMA TFLOP")
    for b in (1, 4):
        D, Hc = C // H, H
        qkv = torch.randn(b, T, 3 * C, device="cuda").half()
        out, lse, lse_c = torch.empty(b, T, C, device="cuda").half(), torch.empty(b, C // 128, T, device="cuda"), torch.empty(b, Hc, T, device="cuda")
        dc, dn = ab(lambda i: _C.causal_attention(qkv, b, T, Hc, D, out, lse_c),
                    lambda i: _C.attention_forward(qkv, b, T, C // 128, 128 ** -0.5, out, lse, dim_head=128), inner=20)
        fc, fn = causal_executed_flop(b, T, Hc, D), 4.0 * b * (C // 128) * T * T * 128
        lines.append(f"  B={b}: causal D=384 H=16  {dc[1] * 1e3:8.1f} [{dc[0] * 1e3:.1f} .. {dc[2] * 1e3:.1f}] us, {fc / 1e9:7.1f} GFLOP executed, {dc[1] * 1e3 / (fc / 1e12):7.0f} us/TFLOP"
                     f" ({fc / dc[1] / 1e9:.0f} TF/s);  full D=128 H=48  {dn[1] * 1e3:8.1f} [{dn[0] * 1e3:.1f} .. {dn[2] * 1e3:.1f}] us, {fn / 1e9:7.1f} GFLOP, "
                     f"{dn[1] * 1e3 / (fn / 1e12):7.0f} us/TFLOP ({fn / dn[1] / 1e9:.0f} TF/s)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
