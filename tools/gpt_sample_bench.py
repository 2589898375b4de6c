"""Times stage-2 sampling at the shipped size (configs/imagenet_gpt_vitvq_base.yaml: C = 6144, 24 layers, 16 heads of 384, V = 8192; random weights)
and writes profiles/gpt_sample.txt:  python tools/gpt_sample_bench.py [--out FILE] [--layers N]

Per point (batch 4 | 16, cache length 1 | 512 | 1024): ms per sampling step of the device path (GPT._decode_step + the sampler) and of a plain-torch
fp16 restatement of the same step (torch.matmul / F.layer_norm / softmax on a preallocated cache), alternating inside this process; and the bytes the
step must move (every GEMM weight once + the cache up to t + the activations) over the time, as a share of the 6.29 TB/s that a plain copy reaches on
MI355X.  The same share for the skinny GEMM and the decode attention alone, and the time of a whole 1024-step sample at batch 4.
Timing: HIP events around a window of back-to-back calls (10 steps; 100 kernel launches over rotating operand buffers larger than the last-level
cache), median, minimum and maximum of 7 windows that alternate between the two paths, after a warm-up.

--graph writes profiles/gpt_sample_graph.txt instead: the eager loop against replays of one captured position (sample(graph=True)) at batch 1 and 4
(tools/sample_graph_bench.py).

--weights fp8 writes profiles/gpt_sample_fp8.txt instead: the step with MXFP8 Block weights (sample(weights="fp8")) against the
16-bit step at batch 1, 4 and 16, alternating windows in this process, and the five products alone in both forms with the TB/s of the bytes each
actually moves.

--weights fp4 writes profiles/gpt_sample_fp4.txt instead: the step with MXFP4 Block weights (sample(weights="fp4")) against the
fp8 and the 16-bit step, the three alternating in this process, and the four Block products alone in the three forms.

--weights fp6 writes profiles/gpt_sample_fp6.txt instead: the step with MXFP6 Block weights (sample(weights="fp6")) against the
16-bit, the fp8 and the fp4 step, the four alternating in this process, and the four Block products alone in the four forms.

--cache fp8 writes profiles/gpt_sample_kv8.txt instead: the step with MXFP8 k / v caches (sample(cache="fp8")) against the step
with 16-bit caches at batch 1, 4, 16 and 64, alternating windows in this process, under the weights of --weights (h16 or fp8: with fp8 the file is
profiles/gpt_sample_kv8_w8.txt), and the decode attention alone in both forms with the TB/s of the bytes each actually moves.

--prefix P [P ...] writes profiles/gpt_sample_prefix.txt instead: the batched prefill of P given codes (sample(prefix_codes=))
against the same P positions run by the forced loop (one weight-streaming step and one draw per position), alternating windows in this process, and
the whole sample(prefix_codes=) against the whole forced run, at batch 1 and 4 under 16-bit and one MX weight format (--weights, default fp8) and
under 16-bit and MXFP8 caches.  The MX prefill re-reads the Block weights once per piece of 64 rows: the table says how often and what it costs."""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
from enhancing import _C  # noqa: E402
from enhancing.modules.stage2.layers import GPT  # noqa: E402

COPY_TBS = 6.29


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(inner):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def ab(fa, fb, inner, reps=7):
    """(min, median, max) ms per call of fa and of fb: `reps` alternating windows of `inner` back-to-back calls each, after a warm-up of both.
    fa / fb take the call's index inside its window (the kernel-alone runs rotate their weight buffers with it)."""
    fa(0); fb(0)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa, inner))
        tb.append(timed(fb, inner))
    st = lambda v: (min(v), statistics.median(v), max(v))
    return st(ta), st(tb)


class TorchStep:
    """the yardstick: the same step in plain fp16 torch on the operand copies of the model"""

    def __init__(self, m, b, T):
        self.m, self.b = m, b
        C, H = m.embed_dim, m.n_heads
        self.ops = m._operand_copies(torch.float16)
        h = lambda p: None if p is None else p.detach().half()
        self.ln = [(h(k.ln1.weight), h(k.ln1.bias), h(k.ln2.weight), h(k.ln2.bias), h(k.attn.proj.bias), h(k.mlp.p0.bias), h(k.mlp.p1.bias)) for k in m.blocks]
        self.lnf = (h(m.layer_norm.weight), h(m.layer_norm.bias))
        self.tm = [W["time_mix"].half() for W in self.ops["layers"]]
        self.bqkv = [W["bqkv"].half() for W in self.ops["layers"]]
        self.emb, self.pos = h(m.tok_emb_code.weight), h(m.pos_emb_code)[0]
        self.kc = [torch.zeros(b * H, T, C // H, dtype=torch.float16, device="cuda") for _ in m.blocks]
        self.vc = [torch.zeros(b * H, T, C // H, dtype=torch.float16, device="cuda") for _ in m.blocks]

    def __call__(self, t, ids):
        m, b = self.m, self.b
        C, H = m.embed_dim, m.n_heads
        hs = C // H
        x = self.emb[ids] + self.pos[t - 1]
        for W, (w1, b1, w2, b2, bp, b0, bq), tm, bqkv, kc, vc in zip(self.ops["layers"], self.ln, self.tm, self.bqkv, self.kc, self.vc):
            a = F.layer_norm(x, (C,), w1, b1) * tm
            qkv = torch.addmm(bqkv, a, W["wqkv"].t())
            q, k, v = (z.reshape(b * H, 1, hs) for z in qkv.split(C, dim=1))
            kc[:, t:t + 1], vc[:, t:t + 1] = k, v
            att = torch.softmax(torch.bmm(q, kc[:, :t + 1].transpose(1, 2)) * (1.0 / math.sqrt(hs)), dim=-1)
            x = x + torch.addmm(bp, torch.bmm(att, vc[:, :t + 1]).reshape(b, C), W["wproj"].t())
            hdn = torch.square(torch.relu(torch.addmm(b0, F.layer_norm(x, (C,), w2, b2), W["w0"].t())))
            x = x + torch.addmm(bq, hdn, W["w1"].t())
        logits = torch.matmul(F.layer_norm(x, (C,), *self.lnf), self.ops["head"].t()).float()
        return torch.multinomial(torch.softmax(logits, -1), 1)


def graph_mode(m, L, out):
    """--graph: the eager loop against replays of one captured position (sample(graph=True)) at batch 1 and 4 and the cache fills
    of the table above; writes profiles/gpt_sample_graph.txt"""
    import sample_graph_bench as SG
    C, V, T = m.embed_dim, m.vocab_img_size, m.img_num_tokens
    dt, count = torch.float16, 10
    lines = [f"stage-2 GPT sampling, eager loop against replays of one captured position, on {torch.cuda.get_device_name(0)}: C={C} layers={L} "
             f"heads={m.n_heads} V={V} T={T}, fp16 operands, top_k 100, logits returned",
             f"ms per position: mean [min .. max] of 5 windows of {count} consecutive positions per path, the paths alternating, after a warm-up window of "
             "both; host clock around work that ends in a device synchronise",
             f"{'batch':>5} {'cache':>5} {'eager ms [min .. max]':>28} {'graph ms [min .. max]':>28} {'eager/graph':>11} {'beyond spread':>13} {'capture ms':>10} "
             f"{'nodes':>6} {'bit-equal':>9}"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for b in (1, 4):
            st = m._decode_state(b, dt, "cuda")
            for kc, vc in st["caches"]:
                kc.normal_(0, 0.5)
                vc.normal_(0, 0.5)
            forced = torch.randint(0, V, (b, T), device="cuda")
            outs = {k: (torch.zeros(b, T, dtype=torch.int64, device="cuda"), torch.zeros(b, T * V, device="cuda")) for k in ("eager", "graph")}
            draw = dict(temperature=1.0, top_k=100, top_p=None, seed=1, call=0, row0=0)

            def eager(t):
                codes, logits = outs["eager"]
                m._decode_step(st, t, forced[:, t - 1])
                _C.sample_logits(st["logits"], codes[:, t], step=t, logits_out=logits[:, t * V:(t + 1) * V], **draw)

            def later(cursor):
                codes, logits = outs["graph"]
                m._decode_step(st, None, forced, cursor=cursor)
                _C.sample_logits_at(st["logits"], codes, cursor, logits_out=logits, **draw)

            eager(1)      # warms the launches and their workspaces on this stream, as position 0 does in sample()
            g, cursor, cap_s, nodes = SG.capture_position(later, "cuda")
            for n in (1, 512, 1024):
                first = max(1, min(n - 1, T - count))
                e, r = SG.eager_against_graph(eager, g, cursor, first, count)
                sl = slice(first, first + count)
                same = all(SG.same_bits(a.view(b, T, -1)[:, sl], c.view(b, T, -1)[:, sl]) for a, c in zip(outs["eager"], outs["graph"]))
                assert same, f"graph and eager differ at batch {b}, positions {first} .. {first + count - 1}"
                assert int(cursor.item()) == first + count
                lines.append(f"{b:>5} {n:>5} {SG.fmt(e):>28} {SG.fmt(r):>28} {e[0] / r[0]:>11.3f} {'yes' if r[2] < e[1] else 'no':>13} {cap_s * 1e3:>10.1f} "
                             f"{'n/a' if nodes is None else nodes:>6} {'yes':>9}")
            del st, g, outs
            torch.cuda.empty_cache()
    torch.cuda.current_stream().wait_stream(side)
    lines.append("beyond spread: the slowest graph window is faster than the fastest eager window of the same point")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def fp8_mode(m, L, out):
    """--weights fp8: the MXFP8-weight step against the 16-bit step, and the five products alone; writes profiles/gpt_sample_fp8.txt"""
    C, V, T, H = m.embed_dim, m.vocab_img_size, m.img_num_tokens, m.n_heads
    dt = torch.float16
    w16 = (12 * C * C * L + V * C) * 2
    w8 = 12 * C * C * L + 12 * C * C * L // 32 + V * C * 2
    lines = [f"stage-2 GPT sampling step, MXFP8 Block weights against 16-bit weights, on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} V={V}, "
             f"fp16 activations and caches; weights per step {w16 / 1e9:.2f} GB (16-bit) / {w8 / 1e9:.2f} GB (fp8: codes + scales + the 16-bit head)",
             "times: median [min .. max] of 7 alternating windows in one process; a step window is 10 steps, a kernel window is 100 launches over rotating",
             "operand buffers of >= 1 GB in all; kernel times are event times over back-to-back launches: they include the launch boundary (~1-2 us each)",
             f"{'batch':>5} {'cache':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'16-bit/fp8':>10} {'beyond spread':>13} {'fp8 GB':>7} {'fp8 TB/s':>8}"]
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    f1 = lambda v: f"{v[1] * 1e3:.1f} [{v[0] * 1e3:.1f} .. {v[2] * 1e3:.1f}]"
    for b in (1, 4, 16):
        sts = {w: m._decode_state(b, dt, "cuda", weights=w) for w in ("h16", "fp8")}
        codes = torch.randint(0, V, (b, T), device="cuda")
        for n in (1, 512, 1024):
            t = n - 1

            def step(w):
                def run(i):
                    m._decode_step(sts[w], t, codes[:, t - 1] if t else codes[:, 0] % 1000)
                    _C.sample_logits(sts[w]["logits"], codes[:, t], top_k=None, top_p=None, seed=1, step=t)
                return run
            h, f = ab(step("h16"), step("fp8"), inner=10)
            moved = w8 + 2 * L * b * n * C * 2 + L * b * C * (4 * 6 + 2 * 10)
            lines.append(f"{b:>5} {n:>5} {f3(h):>28} {f3(f):>28} {h[1] / f[1]:>10.3f} {'yes' if f[2] < h[0] else 'no':>13} {moved / 1e9:>7.2f} "
                         f"{moved / (f[1] * 1e-3) / 1e12:>8.2f}")
        del sts
        torch.cuda.empty_cache()
    lines.append("beyond spread: the slowest fp8 window is faster than the fastest 16-bit window of the same point")
    lines.append("kernels alone (fp16 activations), us: median [min .. max]; TB/s of the bytes each form moves; kept = fp8 TB/s / 16-bit TB/s:")
    for b in (1, 4, 16):
        for name, N, K in (("qkv", 3 * C, C), ("proj", C, C), ("p0", 4 * C, C), ("p1", C, 4 * C), ("head", V, C)):
            nbuf = max(2, -(-(1 << 30) // (N * K)))
            x = torch.randn(b, K, device="cuda").half()
            y = torch.empty(b, N, device="cuda")
            ws = [(torch.randn(N, K, device="cuda") / math.sqrt(K)) for _ in range(2)]
            w16s = [ws[i % 2].half() for i in range(-(-nbuf // 2))]
            by16 = 2 * N * K + 2 * b * K + 4 * b * N
            if name == "head":       # stays 16-bit under weights="fp8": one form
                d, _ = ab(lambda i: _C.skinny_gemm(x, w16s[i % len(w16s)], y), lambda i: None, inner=100)
                lines.append(f"  {name:>4} M={b:<2} N={N:<5} K={K:<5}: 16-bit {f1(d):>24} us {by16 / d[1] / 1e9:5.2f} TB/s   (the head stays 16-bit)")
                continue
            q8 = []
            for i in range(nbuf):
                q = (torch.empty(N, K, dtype=torch.uint8, device="cuda"), torch.empty(N, K // 32, dtype=torch.uint8, device="cuda"))
                _C.quantize_mxfp8(ws[i % 2], q[0], q[1])
                q8.append(q)
            by8 = N * K + N * K // 32 + 2 * b * K + 4 * b * N
            d, f = ab(lambda i: _C.skinny_gemm(x, w16s[i % len(w16s)], y), lambda i: _C.skinny_gemm_w8(x, *q8[i % nbuf], y), inner=100)
            t16, t8 = by16 / d[1] / 1e9, by8 / f[1] / 1e9
            lines.append(f"  {name:>4} M={b:<2} N={N:<5} K={K:<5}: 16-bit {f1(d):>24} us {t16:5.2f} TB/s   fp8 {f1(f):>24} us {t8:5.2f} TB/s   "
                         f"time {d[1] / f[1]:5.2f}x   kept {t8 / t16:4.2f}")
            del ws, w16s, q8
        torch.cuda.empty_cache()
    ops8 = sum(t.numel() * t.element_size() for W in m._sample_operands(dt, "fp8")["layers"] for k in ("wqkv", "wproj", "w0", "w1") for t in W[k])
    ops16 = sum(W[k].numel() * 2 for W in m._operand_copies(dt)["layers"] for k in ("wqkv", "wproj", "w0", "w1"))
    lines.append(f"operand copies of the Blocks held by the process: {ops8 / 1e9:.2f} GB (fp8) against {ops16 / 1e9:.2f} GB (16-bit)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def alternate(fns, inner, reps=7):
    """`ab` for any number of forms: [(min, median, max) ms per call of each], `reps` rounds of one window of `inner` calls per form, in turn"""
    for fn in fns:
        fn(0)
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for v, fn in zip(ts, fns):
            v.append(timed(fn, inner))
    return [(min(v), statistics.median(v), max(v)) for v in ts]


def fp4_mode(m, L, out):
    """--weights fp4: the MXFP4-weight step against the MXFP8-weight step and the 16-bit step, the three alternating in one process, and the four
    Block products alone in the three forms; writes profiles/gpt_sample_fp4.txt"""
    C, V, T, H = m.embed_dim, m.vocab_img_size, m.img_num_tokens, m.n_heads
    dt = torch.float16
    blocks = 12 * C * C * L
    wb = {"h16": (blocks + V * C) * 2, "fp8": blocks + blocks // 32 + V * C * 2, "fp4": blocks // 2 + blocks // 32 + V * C * 2}
    forms = ("h16", "fp8", "fp4")
    lines = [f"stage-2 GPT sampling step, MXFP4 Block weights against MXFP8 and 16-bit weights, on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} "
             f"V={V}, fp16 activations and caches; weights per step {wb['h16'] / 1e9:.2f} GB (16-bit) / {wb['fp8'] / 1e9:.2f} GB (fp8) / "
             f"{wb['fp4'] / 1e9:.2f} GB (fp4: codes + scales + the 16-bit head)",
             "times: median [min .. max] of 7 rounds of alternating windows in one process; a step window is 10 steps, a kernel window is 100 launches over",
             "rotating operand buffers of >= 1 GB in all; kernel times are event times over back-to-back launches: they include the launch boundary (~1-2 us each)",
             f"{'batch':>5} {'cache':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'fp4 ms [min .. max]':>28} {'16-bit/fp4':>10} {'fp8/fp4':>8} "
             f"{'beyond fp8':>10} {'fp4 GB':>7} {'fp4 TB/s':>8}"]
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    f1 = lambda v: f"{v[1] * 1e3:.1f} [{v[0] * 1e3:.1f} .. {v[2] * 1e3:.1f}]"
    for b in (1, 4, 16):
        sts = {w: m._decode_state(b, dt, "cuda", weights=w) for w in forms}
        codes = torch.randint(0, V, (b, T), device="cuda")
        for n in (1, 512, 1024):
            t = n - 1

            def step(w):
                def run(i):
                    m._decode_step(sts[w], t, codes[:, t - 1] if t else codes[:, 0] % 1000)
                    _C.sample_logits(sts[w]["logits"], codes[:, t], top_k=None, top_p=None, seed=1, step=t)
                return run
            h, e, f = alternate([step(w) for w in forms], inner=10)
            moved = wb["fp4"] + 2 * L * b * n * C * 2 + L * b * C * (4 * 6 + 2 * 10)
            lines.append(f"{b:>5} {n:>5} {f3(h):>28} {f3(e):>28} {f3(f):>28} {h[1] / f[1]:>10.3f} {e[1] / f[1]:>8.3f} {'yes' if f[2] < e[0] else 'no':>10} "
                         f"{moved / 1e9:>7.2f} {moved / (f[1] * 1e-3) / 1e12:>8.2f}")
        del sts
        torch.cuda.empty_cache()
    lines.append("beyond fp8: the slowest fp4 window is faster than the fastest fp8 window of the same point")
    lines.append("kernels alone (fp16 activations), us: median [min .. max]; TB/s of the bytes each form moves; kept = fp4 TB/s / 16-bit TB/s:")
    for b in (1, 4, 16):
        for name, N, K in (("qkv", 3 * C, C), ("proj", C, C), ("p0", 4 * C, C), ("p1", C, 4 * C)):
            nbuf = max(2, -(-(1 << 30) // (N * K)))      # sized for the 16-bit form; the 4-bit form rotates over twice as many buffers, >= 1 GB too
            x = torch.randn(b, K, device="cuda").half()
            y = torch.empty(b, N, device="cuda")
            ws = [(torch.randn(N, K, device="cuda") / math.sqrt(K)) for _ in range(2)]
            w16s = [ws[i % 2].half() for i in range(-(-nbuf // 2))]
            q8, q4 = [], []
            for i in range(nbuf):
                q = (torch.empty(N, K, dtype=torch.uint8, device="cuda"), torch.empty(N, K // 32, dtype=torch.uint8, device="cuda"))
                _C.quantize_mxfp8(ws[i % 2], q[0], q[1])
                q8.append(q)
            for i in range(2 * nbuf):
                q = (torch.empty(N, K // 2, dtype=torch.uint8, device="cuda"), torch.empty(N, K // 32, dtype=torch.uint8, device="cuda"))
                _C.quantize_mxfp4(ws[i % 2], q[0], q[1])
                q4.append(q)
            io = 2 * b * K + 4 * b * N
            by16, by8, by4 = 2 * N * K + io, N * K + N * K // 32 + io, N * K // 2 + N * K // 32 + io
            d, e, f = alternate([lambda i: _C.skinny_gemm(x, w16s[i % len(w16s)], y), lambda i: _C.skinny_gemm_w8(x, *q8[i % nbuf], y),
                                 lambda i: _C.skinny_gemm_w4(x, *q4[i % (2 * nbuf)], y)], inner=100)
            t16, t8, t4 = by16 / d[1] / 1e9, by8 / e[1] / 1e9, by4 / f[1] / 1e9
            lines.append(f"  {name:>4} M={b:<2} N={N:<5} K={K:<5}: 16-bit {f1(d):>24} us {t16:5.2f} TB/s   fp8 {f1(e):>24} us {t8:5.2f} TB/s   "
                         f"fp4 {f1(f):>24} us {t4:5.2f} TB/s   time vs fp8 {e[1] / f[1]:5.2f}x   kept {t4 / t16:4.2f}")
            del ws, w16s, q8, q4
        torch.cuda.empty_cache()
    held = lambda w: sum(t.numel() * t.element_size() for W in m._sample_operands(dt, w)["layers"] for k in ("wqkv", "wproj", "w0", "w1") for t in W[k])
    ops16 = sum(W[k].numel() * 2 for W in m._operand_copies(dt)["layers"] for k in ("wqkv", "wproj", "w0", "w1"))
    lines.append(f"operand copies of the Blocks held by the process: {held('fp4') / 1e9:.2f} GB (fp4) against {held('fp8') / 1e9:.2f} GB (fp8) and "
                 f"{ops16 / 1e9:.2f} GB (16-bit)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def fp6_mode(m, L, out):
    """--weights fp6: the MXFP6-weight step against the 16-bit, the MXFP8-weight and the MXFP4-weight step, the four alternating in one process, and
    the four Block products alone in the four forms; writes profiles/gpt_sample_fp6.txt"""
    C, V, T, H = m.embed_dim, m.vocab_img_size, m.img_num_tokens, m.n_heads
    dt = torch.float16
    blocks = 12 * C * C * L
    wb = {"h16": (blocks + V * C) * 2, "fp8": blocks + blocks // 32 + V * C * 2, "fp6": blocks * 3 // 4 + blocks // 32 + V * C * 2,
          "fp4": blocks // 2 + blocks // 32 + V * C * 2}
    forms = ("h16", "fp8", "fp6", "fp4")
    lines = [f"stage-2 GPT sampling step, MXFP6 Block weights against 16-bit, MXFP8 and MXFP4 weights, on {torch.cuda.get_device_name(0)}: C={C} layers={L} "
             f"heads={H} V={V}, fp16 activations and caches; weights per step {wb['h16'] / 1e9:.2f} GB (16-bit) / {wb['fp8'] / 1e9:.2f} GB (fp8) / "
             f"{wb['fp6'] / 1e9:.2f} GB (fp6) / {wb['fp4'] / 1e9:.2f} GB (fp4: codes + scales + the 16-bit head)",
             "times: median [min .. max] of 7 rounds of alternating windows in one process; a step window is 10 steps, a kernel window is 100 launches over",
             "rotating operand buffers of >= 1 GB in all; kernel times are event times over back-to-back launches: they include the launch boundary (~1-2 us each)",
             f"{'batch':>5} {'cache':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'fp6 ms [min .. max]':>28} {'fp4 ms [min .. max]':>28} "
             f"{'fp8/fp6':>8} {'fp6/fp4':>8} {'not slower':>10} {'beyond fp8':>10} {'between':>8} {'fp6 GB':>7} {'fp6 TB/s':>8}"]
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    f1 = lambda v: f"{v[1] * 1e3:.1f} [{v[0] * 1e3:.1f} .. {v[2] * 1e3:.1f}]"
    for b in (1, 4, 16):
        sts = {w: m._decode_state(b, dt, "cuda", weights=w) for w in forms}
        codes = torch.randint(0, V, (b, T), device="cuda")
        for n in (1, 1024):
            t = n - 1

            def step(w):
                def run(i):
                    m._decode_step(sts[w], t, codes[:, t - 1] if t else codes[:, 0] % 1000)
                    _C.sample_logits(sts[w]["logits"], codes[:, t], top_k=None, top_p=None, seed=1, step=t)
                return run
            h, e, s, f = alternate([step(w) for w in forms], inner=10)
            moved = wb["fp6"] + 2 * L * b * n * C * 2 + L * b * C * (4 * 6 + 2 * 10)
            lines.append(f"{b:>5} {n:>5} {f3(h):>28} {f3(e):>28} {f3(s):>28} {f3(f):>28} {e[1] / s[1]:>8.3f} {s[1] / f[1]:>8.3f} "
                         f"{'yes' if s[2] <= e[2] else 'NO':>10} {'yes' if s[2] < e[0] else 'no':>10} {(e[1] - s[1]) / (e[1] - f[1]):>8.2f} "
                         f"{moved / 1e9:>7.2f} {moved / (s[1] * 1e-3) / 1e12:>8.2f}")
        del sts
        torch.cuda.empty_cache()
    lines.append("not slower: the slowest fp6 window is no slower than the slowest fp8 window of the same point; beyond fp8: the slowest fp6 window is faster")
    lines.append("than the fastest fp8 window; between: where the fp6 median lies on the way from the fp8 median (0) to the fp4 median (1); the bytes say 0.46")
    lines.append("kernels alone (fp16 activations), us: median [min .. max]; TB/s of the bytes each form moves:")
    for b in (1, 4, 16):
        for name, N, K in (("qkv", 3 * C, C), ("proj", C, C), ("p0", 4 * C, C), ("p1", C, 4 * C)):
            nbuf = max(2, -(-(1 << 30) // (N * K)))      # sized for the 16-bit form; the other forms rotate over as many buffers as make >= 1 GB too
            x = torch.randn(b, K, device="cuda").half()
            y = torch.empty(b, N, device="cuda")
            ws = [(torch.randn(N, K, device="cuda") / math.sqrt(K)) for _ in range(2)]
            w16s = [ws[i % 2].half() for i in range(-(-nbuf // 2))]
            q8, q6, q4 = [], [], []
            for i in range(nbuf):
                q = (torch.empty(N, K, dtype=torch.uint8, device="cuda"), torch.empty(N, K // 32, dtype=torch.uint8, device="cuda"))
                _C.quantize_mxfp8(ws[i % 2], q[0], q[1])
                q8.append(q)
            for i in range(-(-4 * nbuf // 3)):
                q = (torch.empty(N, _C.mxfp6_row_bytes(K), dtype=torch.uint8, device="cuda"), torch.empty(N, K // 32, dtype=torch.uint8, device="cuda"))
                _C.quantize_mxfp6(ws[i % 2], q[0], q[1])
                q6.append(q)
            for i in range(2 * nbuf):
                q = (torch.empty(N, K // 2, dtype=torch.uint8, device="cuda"), torch.empty(N, K // 32, dtype=torch.uint8, device="cuda"))
                _C.quantize_mxfp4(ws[i % 2], q[0], q[1])
                q4.append(q)
            io = 2 * b * K + 4 * b * N
            by16, by8, by6, by4 = 2 * N * K + io, N * K + N * K // 32 + io, N * K * 3 // 4 + N * K // 32 + io, N * K // 2 + N * K // 32 + io
            d, e, s, f = alternate([lambda i: _C.skinny_gemm(x, w16s[i % len(w16s)], y), lambda i: _C.skinny_gemm_w8(x, *q8[i % nbuf], y),
                                    lambda i: _C.skinny_gemm_w6(x, *q6[i % len(q6)], y), lambda i: _C.skinny_gemm_w4(x, *q4[i % (2 * nbuf)], y)], inner=100)
            t16, t8, t6, t4 = by16 / d[1] / 1e9, by8 / e[1] / 1e9, by6 / s[1] / 1e9, by4 / f[1] / 1e9
            lines.append(f"  {name:>4} M={b:<2} N={N:<5} K={K:<5}: 16-bit {f1(d):>22} us {t16:5.2f} TB/s   fp8 {f1(e):>22} us {t8:5.2f} TB/s   "
                         f"fp6 {f1(s):>22} us {t6:5.2f} TB/s   fp4 {f1(f):>22} us {t4:5.2f} TB/s   fp6 time vs fp8 {e[1] / s[1]:5.2f}x vs fp4 {f[1] / s[1]:5.2f}x")
            del ws, w16s, q8, q6, q4
        torch.cuda.empty_cache()
    held = lambda w: sum(t.numel() * t.element_size() for W in m._sample_operands(dt, w)["layers"] for k in ("wqkv", "wproj", "w0", "w1") for t in W[k])
    lines.append(f"operand copies of the Blocks held by the process: {held('fp6') / 1e9:.2f} GB (fp6) against {held('fp8') / 1e9:.2f} GB (fp8) and "
                 f"{held('fp4') / 1e9:.2f} GB (fp4)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def _fill_kv(kv, gen_scale=0.5):
    """random cache contents: 16-bit tensors N(0, 0.5); MXFP8 codes without the NaN code (bit 3 cleared) under scales around 2^-7"""
    if len(kv) == 2:
        for z in kv:
            z.normal_(0, gen_scale)
        return
    for codes, scales in (kv[:2], kv[2:]):
        codes.random_(0, 256).bitwise_and_(0xF7)
        scales.random_(118, 122)


def kv8_mode(m, L, out, weights):
    """--cache fp8: the step with MXFP8 caches against the step with 16-bit caches, and the decode attention alone; writes profiles/gpt_sample_kv8*.txt"""
    from enhancing.modules.stage2.prior import _kv_caches
    C, V, T, H = m.embed_dim, m.vocab_img_size, m.img_num_tokens, m.n_heads
    hs, dt = C // H, torch.float16
    blocks = 12 * C * C * L
    wb = {"h16": (blocks + V * C) * 2, "fp8": blocks + blocks // 32 + V * C * 2, "fp6": blocks * 3 // 4 + blocks // 32 + V * C * 2,
          "fp4": blocks // 2 + blocks // 32 + V * C * 2}[weights]
    kv16 = lambda b, n: 2 * L * b * n * C * 2
    kv8 = lambda b, n: 2 * L * b * n * (C + C // 32)
    lines = [f"stage-2 GPT sampling step, MXFP8 k / v caches against 16-bit caches, on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} V={V}, "
             f"fp16 activations, {dict(h16='16-bit', fp8='MXFP8', fp6='MXFP6', fp4='MXFP4')[weights]} Block weights ({wb / 1e9:.2f} GB per step)",
             f"caches held at T={T}, batch 64: {kv16(64, T) / 1e9:.1f} GB (16-bit) / {kv8(64, T) / 1e9:.1f} GB (fp8: codes + scales)",
             "times: median [min .. max] of 7 alternating windows in one process; a step window is 10 steps, a kernel window is 100 launches over 2 to 16",
             "rotating cache buffers (0.4 GB in all at batch 1, >= 1 GB from batch 4); kernel times are event times over back-to-back launches: they include the launch boundary (~1-2 us each)",
             f"{'batch':>5} {'cache':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'16-bit/fp8':>10} {'beyond spread':>13} {'kv GB 16':>8} {'kv GB fp8':>9}"]
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    f1 = lambda v: f"{v[1] * 1e3:.1f} [{v[0] * 1e3:.1f} .. {v[2] * 1e3:.1f}]"
    for b in (1, 4, 16, 64):
        sts = {c: m._decode_state(b, dt, "cuda", weights=weights, cache=c) for c in ("h16", "fp8")}
        for st in sts.values():
            for kv in st["caches"]:
                _fill_kv(kv)
        codes = torch.randint(0, V, (b, T), device="cuda")
        for n in (1, 512, 1024):
            t = n - 1

            def step(c):
                def run(i):
                    m._decode_step(sts[c], t, codes[:, t - 1] if t else codes[:, 0] % 1000)
                    _C.sample_logits(sts[c]["logits"], codes[:, t], top_k=None, top_p=None, seed=1, step=t)
                return run
            h, f = ab(step("h16"), step("fp8"), inner=10)
            lines.append(f"{b:>5} {n:>5} {f3(h):>28} {f3(f):>28} {h[1] / f[1]:>10.3f} {'yes' if f[2] < h[0] else 'no':>13} {kv16(b, n) / 1e9:>8.2f} "
                         f"{kv8(b, n) / 1e9:>9.2f}")
        del sts
        torch.cuda.empty_cache()
    lines.append("beyond spread: the slowest fp8 window is faster than the fastest 16-bit window of the same point")
    lines.append("decode attention alone (one layer, fp16 q), us: median [min .. max]; TB/s of the cache bytes each form reads; kept = fp8 TB/s / 16-bit TB/s:")
    for b in (1, 4, 16, 64):
        per16 = 2 * b * T * C * 2
        nbuf = max(2, min(16, -(-(1 << 30) // per16)))
        qkv = torch.randn(b, 3 * C, device="cuda").half()
        o = torch.empty(b, C, device="cuda").half()
        c16 = _kv_caches(nbuf, b, H, T, hs, dt, "cuda", "h16")
        c8 = _kv_caches(nbuf, b, H, T, hs, dt, "cuda", "fp8")
        for kv in c16 + c8:
            _fill_kv(kv)
        for n in (1, 512, 1024):
            by16, by8 = 2 * b * n * C * 2, 2 * b * n * (C + C // 32)
            d, f = ab(lambda i: _C.decode_attention(qkv, *c16[i % nbuf], n - 1, o), lambda i: _C.decode_attention_kv8(qkv, *c8[i % nbuf], n - 1, o), inner=100)
            t16, t8 = by16 / d[1] / 1e9, by8 / f[1] / 1e9
            lines.append(f"  decode_attention B={b:<2} len={n:<4}: 16-bit {f1(d):>24} us {by16 / 1e6:7.1f} MB {t16:5.2f} TB/s   fp8 {f1(f):>24} us {by8 / 1e6:7.1f} MB "
                         f"{t8:5.2f} TB/s   time {d[1] / f[1]:5.2f}x   kept {t8 / t16:4.2f}")
        del c16, c8
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def prefix_mode(m, L, out, prefixes, mx, reps=3):
    """--prefix: the prefill of P given codes against the forced loop over the same P positions, and the whole calls; writes
    profiles/gpt_sample_prefix.txt"""
    C, V, T, H = m.embed_dim, m.vocab_img_size, m.img_num_tokens, m.n_heads
    dt = torch.float16
    blocks = 12 * C * C * L
    wb = {"h16": blocks * 2, "fp8": blocks + blocks // 32, "fp6": blocks * 3 // 4 + blocks // 32, "fp4": blocks // 2 + blocks // 32}
    fs = lambda v: f"{v[1] / 1e3:.3f} [{v[0] / 1e3:.3f} .. {v[2] / 1e3:.3f}]"
    st3 = lambda v: (min(v), statistics.median(v), max(v))
    lines = [f"stage-2 GPT sampling, a batched prefill of P given codes against the forced loop over the same P positions, on {torch.cuda.get_device_name(0)}: "
             f"C={C} layers={L} heads={H} V={V} T={T}, fp16 activations; Block weights per pass {wb['h16'] / 1e9:.2f} GB (16-bit) / {wb[mx] / 1e9:.2f} GB ({mx})",
             f"prefill | loop: seconds, median [min .. max] of {reps} alternating windows in one process after a warm-up of both; a window is ONE prefill of all P",
             "positions (every layer's k / v rows into the caches; the last layer stops behind its fill) or ONE pass of the existing loop over positions 0 .. P - 1",
             "(a step and a draw per position).  whole: seconds, [min .. max] of 2 alternating calls of sample(prefix_codes=codes[:, :P]) and of",
             "sample(forced_codes=codes), top_k 100, no logits returned.  passes: how often the prefill reads the Block weights (16-bit: once, enh_gemm_h16 over all",
             f"rows; {mx}: once per piece of 64 rows, ceil(b P / 64) times); pass GB = passes x the Block weights",
             f"{'weights':>7} {'cache':>5} {'batch':>5} {'P':>4} {'rows':>5} {'passes':>6} {'pass GB':>8} {'prefill s [min .. max]':>26} {'loop s [min .. max]':>26} {'loop/prefill':>12} "
             f"{'beyond spread':>13} {'whole prefix s':>18} {'whole forced s':>18} {'forced/prefix':>13}"]
    med = {}
    for w in ("h16", mx):
        for c in ("h16", "fp8"):
            for b in (1, 4):
                st = m._decode_state(b, dt, "cuda", weights=w, cache=c)
                conds = torch.randint(0, 1000, (b,), device="cuda")
                codes = torch.randint(0, V, (b, T), device="cuda")
                drawn = torch.empty(b, T, dtype=torch.int64, device="cuda")
                for P in prefixes:
                    def prefill(i):
                        m._prefill(st, conds, codes[:, :P])

                    def loop(i):
                        for t in range(P):
                            m._decode_step(st, t, conds if t == 0 else codes[:, t - 1])
                            _C.sample_logits(st["logits"], drawn[:, t], top_k=100, top_p=None, seed=1, step=t)
                    a, l = ab(prefill, loop, inner=1, reps=reps)
                    med[w, c, b, P] = a[1]
                    kw = dict(top_k=100, seed=1, return_logits=False, weights=w, cache=c)
                    wp, wf = [], []
                    for _ in range(2):
                        wp.append(timed(lambda i: m.sample(conds.view(b, 1), prefix_codes=codes[:, :P], **kw), 1))
                        wf.append(timed(lambda i: m.sample(conds.view(b, 1), forced_codes=codes, **kw), 1))
                    passes = 1 if w == "h16" else -(-b * P // 64)
                    lines.append(f"{w:>7} {c:>5} {b:>5} {P:>4} {b * P:>5} {passes:>6} {passes * wb[w] / 1e9:>8.1f} {fs(a):>26} {fs(l):>26} {l[1] / a[1]:>12.1f} "
                                 f"{'yes' if a[2] < l[0] else 'no':>13} {f'{min(wp) / 1e3:.2f} .. {max(wp) / 1e3:.2f}':>18} {f'{min(wf) / 1e3:.2f} .. {max(wf) / 1e3:.2f}':>18} "
                                 f"{statistics.median(wf) / statistics.median(wp):>13.2f}")
                    print(lines[-1], flush=True)
                del st
                torch.cuda.empty_cache()
    lines.append("beyond spread: the slowest prefill window is faster than the fastest loop window of the same point")
    lines.append(f"what the re-reads cost: the {mx} prefill against the 16-bit prefill of the same point (medians), and the TB/s of its weight passes alone:")
    for c in ("h16", "fp8"):
        for b in (1, 4):
            for P in prefixes:
                passes = -(-b * P // 64)
                lines.append(f"  cache {c:>3} batch {b} P {P:>4}: {mx} {med[mx, c, b, P] / 1e3:.3f} s / 16-bit {med['h16', c, b, P] / 1e3:.3f} s = "
                             f"{med[mx, c, b, P] / med['h16', c, b, P]:.2f}x; {passes} passes of {wb[mx] / 1e9:.2f} GB in that time: "
                             f"{passes * wb[mx] / (med[mx, c, b, P] * 1e-3) / 1e12:.2f} TB/s")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--whole", type=int, default=1, help="also time a whole 1024-step sample at batch 4")
    ap.add_argument("--graph", action="store_true", help="instead of the tables: the eager loop against replays of one captured position "
                    "(profiles/gpt_sample_graph.txt)")
    ap.add_argument("--weights", choices=("h16", "fp8", "fp6", "fp4"), default="h16", help="fp8: instead of the tables, the MXFP8-weight step against the 16-bit "
                    "step and the products alone (profiles/gpt_sample_fp8.txt); fp4: the MXFP4-weight step against both, the three alternating "
                    "(profiles/gpt_sample_fp4.txt); fp6: the MXFP6-weight step against all three (profiles/gpt_sample_fp6.txt)")
    ap.add_argument("--cache", choices=("h16", "fp8"), default="h16", help="fp8: instead of the tables, the step with MXFP8 k / v caches against the step "
                    "with 16-bit caches under the weights of --weights, and the decode attention alone (profiles/gpt_sample_kv8.txt, with --weights fp8 "
                    "profiles/gpt_sample_kv8_w8.txt, with --weights fp6 profiles/gpt_sample_kv8_w6.txt, with --weights fp4 profiles/gpt_sample_kv8_w4.txt)")
    ap.add_argument("--prefix", type=int, nargs="+", default=None, metavar="P", help="instead of the tables: the batched prefill of P given codes against the forced "
                    "loop over the same positions, and the whole calls, under 16-bit weights and the MX format of --weights (default fp8) and under both caches "
                    "(profiles/gpt_sample_prefix.txt); the shipped points are --prefix 256 768")
    args = ap.parse_args()
    if args.out is None:
        name = ("gpt_sample_prefix.txt" if args.prefix else "gpt_sample_graph.txt" if args.graph else dict(h16="gpt_sample_kv8.txt", fp8="gpt_sample_kv8_w8.txt", fp6="gpt_sample_kv8_w6.txt", fp4="gpt_sample_kv8_w4.txt")[args.weights]
                if args.cache == "fp8" else dict(h16="gpt_sample.txt", fp8="gpt_sample_fp8.txt", fp6="gpt_sample_fp6.txt", fp4="gpt_sample_fp4.txt")[args.weights])
        args.out = os.path.join(ROOT, "profiles", name)
    C, H, V, T, L = 6144, 16, 8192, 1024, args.layers
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = GPT(vocab_cond_size=1000, vocab_img_size=V, embed_dim=C, cond_num_tokens=1, img_num_tokens=T, n_heads=H, n_layers=L)
        with torch.no_grad():
            m.pos_emb_code.normal_(0, 0.02)
    if args.prefix:
        if not all(0 < P < T for P in args.prefix):
            raise SystemExit(f"--prefix: every P must be in (0, {T})")
        return prefix_mode(m, L, args.out, args.prefix, "fp8" if args.weights == "h16" else args.weights)
    if args.graph:
        return graph_mode(m, L, args.out)
    if args.cache == "fp8":
        return kv8_mode(m, L, args.out, args.weights)
    if args.weights == "fp8":
        return fp8_mode(m, L, args.out)
    if args.weights == "fp4":
        return fp4_mode(m, L, args.out)
    if args.weights == "fp6":
        return fp6_mode(m, L, args.out)
    dt = torch.float16
    wbytes = (12 * C * C * L + V * C) * 2
    lines = [f"stage-2 sampling step on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} V={V}, fp16 operands; weights {wbytes / 1e9:.2f} GB per step",
             "times: median [min .. max] of 7 alternating windows; a step window is 10 steps (the 21.8 GB of weights pass once per step), a kernel window",
             "is 100 launches over rotating operand buffers of >= 1 GB in all, so no launch finds its weights or cache in the 256 MB last-level cache;",
             "kernel times are event times over back-to-back launches: they include the launch boundary (~1-2 us each)",
             f"{'batch':>5} {'cache':>5} {'device ms [min .. max]':>28} {'torch ms [min .. max]':>28} {'torch/dev':>9} {'GB moved':>9} {'TB/s':>6} {'of 6.29':>8}"]
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    f1 = lambda v: f"{v[1] * 1e3:.1f} [{v[0] * 1e3:.1f} .. {v[2] * 1e3:.1f}]"
    worst = 0.0
    for b in (4, 16):
        st = m._decode_state(b, dt, "cuda")
        codes = torch.randint(0, V, (b, T), device="cuda")
        ts = TorchStep(m, b, T)
        for n in (1, 512, 1024):
            t = n - 1
            tt = max(t, 1)      # the yardstick has no condition branch: its first step is timed as a one-slot code step

            def dev(i):
                m._decode_step(st, t, codes[:, t - 1] if t else codes[:, 0] % 1000)
                _C.sample_logits(st["logits"], codes[:, t], top_k=None, top_p=None, seed=1, step=t)

            def ref(i):
                ts(tt if n > 1 else 0, codes[:, tt - 1])
            d, r = ab(dev, ref, inner=10)
            moved = wbytes + 2 * L * b * n * C * 2 + L * b * C * (4 * 6 + 2 * 10)
            tbs = moved / (d[1] * 1e-3) / 1e12
            worst = max(worst, d[1] / r[1])
            lines.append(f"{b:>5} {n:>5} {f3(d):>28} {f3(r):>28} {r[1] / d[1]:>9.2f} {moved / 1e9:>9.2f} {tbs:>6.2f} {100 * tbs / COPY_TBS:>7.1f}%")
        del st, ts
        torch.cuda.empty_cache()
    lines.append(f"device / torch (medians), worst of the six points: {worst:.3f} (must be <= 1)")
    lines.append("kernels alone (fp16), us: median [min .. max]:")
    for b in (4, 16):
        for name, N, K in (("qkv", 3 * C, C), ("proj", C, C), ("p0", 4 * C, C), ("p1", C, 4 * C), ("head", V, C)):
            nbuf = max(2, -(-(1 << 30) // (2 * N * K)))
            x = torch.randn(b, K, device="cuda").half()
            ws = [torch.randn(N, K, device="cuda").half() for _ in range(nbuf)]
            out = torch.empty(b, N, device="cuda")
            d, r = ab(lambda i: _C.skinny_gemm(x, ws[i % nbuf], out), lambda i: torch.matmul(x, ws[i % nbuf].t()), inner=100)
            by = 2 * N * K + 2 * b * K + 4 * b * N
            lines.append(f"  skinny_gemm {name:>4} M={b:<2} N={N:<5} K={K:<5}: {f1(d):>24} us  {by / d[1] / 1e9:5.2f} TB/s ({100 * by / d[1] / 1e9 / COPY_TBS:4.1f}% of copy)   "
                         f"torch.matmul {f1(r):>24} us")
            del ws
        torch.cuda.empty_cache()
        for n in (1, 512, 1024):
            by = 2 * b * n * C * 2 + b * 4 * C * 2
            nbuf = max(2, min(16, -(-(1 << 30) // (2 * b * T * C * 2))))
            qkv = torch.randn(b, 3 * C, device="cuda").half()
            kvs = [(torch.randn(b, H, T, C // H, device="cuda").half(), torch.randn(b, H, T, C // H, device="cuda").half()) for _ in range(nbuf)]
            out = torch.empty(b, C, device="cuda").half()
            d, _ = ab(lambda i: _C.decode_attention(qkv, kvs[i % nbuf][0], kvs[i % nbuf][1], n - 1, out), lambda i: None, inner=100)
            lines.append(f"  decode_attention B={b:<2} len={n:<4}: {f1(d):>24} us  {by / d[1] / 1e9:5.2f} TB/s ({100 * by / d[1] / 1e9 / COPY_TBS:4.1f}% of copy)")
            del kvs
        torch.cuda.empty_cache()
    if args.whole:
        conds = torch.randint(0, 1000, (4, 1), device="cuda")
        m.sample(conds, top_k=100, seed=1, return_logits=False)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        m.sample(conds, top_k=100, seed=1, return_logits=False)
        e.record()
        torch.cuda.synchronize()
        lines.append(f"whole sample, batch 4, {T} steps, top_k 100: {s.elapsed_time(e) / 1e3:.2f} s ({s.elapsed_time(e) / T:.3f} ms per step)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
