"""Times the stage-2 RQTransformer's sampling loop at the shipped size (the transformer block of configs/imagenet_rqtransformer_rqvae_base.yaml:
C = 1536, 24 spatial and 4 depth layers, 12 heads of 128 in both, T = 1024, D = 4, V = 8192; random weights) and writes profiles/rq_sample.txt:
python tools/rq_sample_bench.py [--out FILE] [--spatial_layers N]

1. The depth transformer's decode attention alone at the shipped shape (batch x 12 heads of 128, a cache of D = 4 slots, the steps d = 0 .. 3 in
   turn), batch 1 and 4, fp16: enh_short_decode_attention against enh_decode_attention at Tmax = D in the same run, the outputs compared.
2. One position of the loop (fp16 operands), batch 1 and 4, at several fills of the spatial cache: the spatial step, the D depth steps with their
   draws (with either depth attention), and the same cached position in plain fp16 torch (torch.addmm, F.layer_norm, softmax, torch.multinomial)
   on the model's own operand copies; launches per position, the GEMM weight bytes a position must read over its time against the rate of a plain
   copy, and the seconds per image extrapolated from the fills.
Timing: HIP events around a window of back-to-back calls; median, minimum and maximum of 7 windows that alternate between the paths, after a warm-up
of every path.  Not 1024 positions: a few positions per fill.

--graph writes profiles/rq_sample_graph.txt instead: the eager loop against replays of one captured position (sample(graph=True)) at batch 1 and 4 and
the same fills (tools/sample_graph_bench.py), then one whole image through sample() both ways.

--weights fp8 writes profiles/rq_sample_fp8.txt instead: one position with MXFP8 Block weights in both stacks (sample(weights="fp8"), DESIGN.md
§3.13) against the 16-bit position at batch 1 and 4 and the same fills, alternating windows in this process.

--weights fp4 writes profiles/rq_sample_fp4.txt instead: the same position with MXFP4 Block weights (sample(weights="fp4")) against
the fp8 and the 16-bit position, the three alternating in this process.

--weights fp6 writes profiles/rq_sample_fp6.txt instead: the same position with MXFP6 Block weights (sample(weights="fp6")) against the
16-bit, the fp8 and the fp4 position, the four alternating in this process.

--cache fp8 writes profiles/rq_sample_kv8.txt instead: one position with MXFP8 spatial k / v caches (sample(cache="fp8")) against
the position with 16-bit caches at batch 1, 4 and 64 and the same fills, alternating windows in this process."""
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
from enhancing.modules.stage2.layers import RQTransformer  # noqa: E402
from enhancing.utils.general import get_config_from_file  # noqa: E402

COPY_TBS = 6.29


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(inner):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def alternate(fns, inner, reps=7):
    """[(min, median, max) ms per call] of every function of `fns`: `reps` rounds of one window of `inner` back-to-back calls per function, after
    a warm-up of each"""
    for fn in fns:
        fn(0)
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for v, fn in zip(ts, fns):
            v.append(timed(fn, inner))
    return [(min(v), statistics.median(v), max(v)) for v in ts]


class TorchPosition:
    """the yardstick: the same cached position (one spatial step, D depth steps, D draws) in plain fp16 torch on the operand copies of the model"""

    def __init__(self, m, b):
        self.m, self.b = m, b
        C, T, D = m.embed_dim, m.img_num_tokens, m.depth_num_tokens
        self.ops = m._operand_copies(torch.float16)
        h = lambda p: None if p is None else p.detach().half()
        self.small = {id(k): (h(k.ln1.weight), h(k.ln1.bias), h(k.ln2.weight), h(k.ln2.bias), h(k.attn.proj.bias), h(k.mlp.p0.bias), h(k.mlp.p1.bias))
                      for k in list(m.spatial_transformer) + list(m.depth_transformer)}
        self.lns, self.lnd = (h(m.ln_spatial.weight), h(m.ln_spatial.bias)), (h(m.ln_depth.weight), h(m.ln_depth.bias))
        self.emb, self.pos, self.pos_d = h(m.tok_emb_code.weight), h(m.pos_emb_code)[0], h(m.pos_emb_depth)[0]
        z = lambda H, n: torch.zeros(b * H, n, C // H, dtype=torch.float16, device="cuda")
        self.sp = [(z(m.spatial_n_heads, T), z(m.spatial_n_heads, T)) for _ in m.spatial_transformer]
        self.dp = [(z(m.depth_n_heads, D), z(m.depth_n_heads, D)) for _ in m.depth_transformer]

    def blocks(self, x, stack, ops, H, caches, t):
        b, C = x.shape
        hs = C // H
        for blk, W, (kc, vc) in zip(stack, ops, caches):
            w1, b1, w2, b2, bp, b0, bq = self.small[id(blk)]
            a = F.layer_norm(x, (C,), w1, b1) * W["time_mix"].half()
            qkv = torch.addmm(W["bqkv"].half(), a, W["wqkv"].t())
            q, k, v = (z.reshape(b * H, 1, hs) for z in qkv.split(C, dim=1))
            kc[:, t:t + 1], vc[:, t:t + 1] = k, v
            att = torch.softmax(torch.bmm(q, kc[:, :t + 1].transpose(1, 2)) * (1.0 / math.sqrt(hs)), dim=-1)
            x = x + torch.addmm(bp, torch.bmm(att, vc[:, :t + 1]).reshape(b, C), W["wproj"].t())
            hdn = torch.square(torch.relu(torch.addmm(b0, F.layer_norm(x, (C,), w2, b2), W["w0"].t())))
            x = x + torch.addmm(bq, hdn, W["w1"].t())
        return x

    @torch.no_grad()
    def __call__(self, t, codes):
        """position t >= 1 given codes [b, T, D]: draws its D codes"""
        m = self.m
        C, D = m.embed_dim, m.depth_num_tokens
        x = self.emb[codes[:, t - 1]].sum(1) + self.pos[t - 1]
        hidden = F.layer_norm(self.blocks(x, m.spatial_transformer, self.ops["spatial"], m.spatial_n_heads, self.sp, t), (C,), *self.lns)
        out = []
        for d in range(D):
            x = hidden if d == 0 else self.emb[codes[:, t, :d]].sum(1) + self.pos_d[d - 1]
            x = self.blocks(x, m.depth_transformer, self.ops["depth"], m.depth_n_heads, self.dp, d)
            logits = torch.matmul(F.layer_norm(x, (C,), *self.lnd), self.ops["head"].t()).float()
            out.append(torch.multinomial(torch.softmax(logits, -1), 1))
        return out


def launches_per_position(b, C, V, D, Ls, Ld, t):
    """kernel launches of one position at spatial slot t, from the code: a Block step is 7 library calls (2 LayerNorms, 4 products, the attention);
    a product whose plan splits K adds its slab pass, the spatial attention its merge once the cache is cut into pieces (past 64 slots)"""
    L = _C.lib()
    split = lambda N, K: 1 + int(L.enh_skinny_gemm_workspace_bytes(b, N, K) > 0)
    block = 2 + split(3 * C, C) + split(C, C) + split(4 * C, C) + split(C, 4 * C) + 1
    spatial = 1 + Ls * (block + int(t + 1 > 64)) + 1
    depth = (D - 1) + D * (Ld * block + 1 + split(V, C) + 1)
    return spatial, depth


def graph_mode(kw, out, whole: bool):
    """--graph: the eager loop against replays of one captured position (sample(graph=True)) at batch 1 and 4 and the cache fills
    of the table above, then one whole image through the public entry both ways; writes profiles/rq_sample_graph.txt"""
    import time
    import sample_graph_bench as SG
    C, V, T, D = kw["embed_dim"], kw["vocab_img_size"], kw["img_num_tokens"], kw["depth_num_tokens"]
    Ls, Ld = kw["spatial_n_layers"], kw["depth_n_layers"]
    dt, count = torch.float16, 10
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(**kw)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    wb = (12 * C * C * Ls + D * (12 * C * C * Ld + V * C)) * 2
    lines = [f"stage-2 RQTransformer sampling, eager loop against replays of one captured position, on {torch.cuda.get_device_name(0)}: C={C} "
             f"spatial layers={Ls} depth layers={Ld} T={T} D={D} V={V}, fp16 operands, top_k 100, logits returned",
             f"ms per position: mean [min .. max] of 5 windows of {count} consecutive positions per path, the paths alternating, after a warm-up window of "
             "both; host clock around work that ends in a device synchronise",
             f"GEMM weights read per position {wb / 1e9:.3f} GB: {wb / COPY_TBS / 1e9:.3f} ms at the {COPY_TBS} TB/s of a plain copy",
             f"{'batch':>5} {'slot':>5} {'eager ms [min .. max]':>28} {'graph ms [min .. max]':>28} {'eager/graph':>11} {'beyond spread':>13} {'capture ms':>10} "
             f"{'nodes':>6} {'launches':>8} {'bit-equal':>9}"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for b in (1, 4):
            st = m._decode_state(b, dt, "cuda")
            for kc, vc in st["spatial"] + st["depth"]:
                kc.normal_(0, 0.5)
                vc.normal_(0, 0.5)
            forced = torch.randint(0, V, (b, T, D), device="cuda")
            outs = {k: (torch.zeros(b, T, D, dtype=torch.int64, device="cuda"), torch.zeros(b, T, D, V, device="cuda")) for k in ("eager", "graph")}
            draw = dict(temperature=1.0, top_k=100, top_p=None, seed=1, call=0, row0=0)

            def eager(t):
                codes, logits = outs["eager"]
                m._spatial_step(st, t, forced[:, t - 1, :])
                for d in range(D):
                    m._depth_step(st, t, d, None if d == 0 else forced[:, t, :d], False, False)
                    _C.sample_logits(st["logits"], codes[:, t, d], step=t * D + d, logits_out=logits[:, t, d, :], **draw)

            def later(cursor):
                codes, logits = outs["graph"]
                m._spatial_step(st, None, forced, cursor=cursor)
                for d in range(D):
                    m._depth_step(st, None, d, None if d == 0 else forced, False, False, cursor=cursor)
                    _C.sample_logits_at(st["logits"], codes, cursor, step_mul=D, step_add=d, logits_out=logits, **draw)

            eager(1)      # warms the launches and their workspaces on this stream, as position 0 does in sample()
            g, cursor, cap_s, nodes = SG.capture_position(later, "cuda")
            for slot in (1, 256, 512, T - 1):
                first = min(slot, T - count)
                e, r = SG.eager_against_graph(eager, g, cursor, first, count)
                same = all(SG.same_bits(a[:, first:first + count], c[:, first:first + count]) for a, c in zip(outs["eager"], outs["graph"]))
                assert same, f"graph and eager differ at batch {b}, positions {first} .. {first + count - 1}"
                assert int(cursor.item()) == first + count
                n_sp, n_dp = launches_per_position(b, C, V, D, Ls, Ld, first + count - 1)
                lines.append(f"{b:>5} {slot:>5} {SG.fmt(e):>28} {SG.fmt(r):>28} {e[0] / r[0]:>11.3f} {'yes' if r[2] < e[1] else 'no':>13} {cap_s * 1e3:>10.1f} "
                             f"{'n/a' if nodes is None else nodes:>6} {n_sp + n_dp:>8} {'yes':>9}")
            del st, g, outs
            torch.cuda.empty_cache()
    torch.cuda.current_stream().wait_stream(side)
    lines += ["beyond spread: the slowest graph window is faster than the fastest eager window of the same point",
              "launches: the eager loop's kernel launches of a position at the window's last slot (the graph always holds the attention's merge node)"]
    if whole:
        conds = torch.randint(0, kw["vocab_cond_size"], (1, 1), device="cuda")
        res, secs = {}, {}
        for graph in (False, True, False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[graph] = m.sample(conds, top_k=100, seed=1, graph=graph)
            torch.cuda.synchronize()
            secs.setdefault(graph, []).append(time.perf_counter() - t0)
        assert SG.same_bits(res[False][1], res[True][1]) and SG.same_bits(res[False][0], res[True][0]), "whole image: graph and eager differ"
        lines.append(f"whole image through sample(), batch 1, {T} positions x {D} codes, top_k 100, two calls each, alternating: eager "
                     f"{secs[False][0]:.2f} s, {secs[False][1]:.2f} s; graph (with its capture) {secs[True][0]:.2f} s, {secs[True][1]:.2f} s; codes and logits bit-equal: yes")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def fp8_mode(kw, out):
    """--weights fp8: one position (the spatial step, the D depth steps, their draws) with MXFP8 Block weights against 16-bit weights"""
    C, V, T, D = kw["embed_dim"], kw["vocab_img_size"], kw["img_num_tokens"], kw["depth_num_tokens"]
    Ls, Ld = kw["spatial_n_layers"], kw["depth_n_layers"]
    dt = torch.float16
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(**kw)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    blocks = 12 * C * C * Ls + D * 12 * C * C * Ld
    w16, w8 = (blocks + D * V * C) * 2, blocks + blocks // 32 + D * V * C * 2
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    lines = [f"stage-2 RQTransformer sampling, MXFP8 Block weights against 16-bit weights, on {torch.cuda.get_device_name(0)}: C={C} spatial layers={Ls} "
             f"depth layers={Ld} T={T} D={D} V={V}, fp16 activations and caches",
             f"GEMM weights read per position {w16 / 1e9:.3f} GB (16-bit) / {w8 / 1e9:.3f} GB (fp8: codes + scales + the 16-bit head, read {D} times)",
             "ms per position (spatial step + the D depth steps with their draws): median [min .. max] of 7 alternating windows of 10 positions in one process",
             f"{'batch':>5} {'slot':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'16-bit/fp8':>10} {'beyond spread':>13} {'launches':>8}"]
    for b in (1, 4):
        sts = {w: m._decode_state(b, dt, "cuda", w) for w in ("h16", "fp8")}
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        for t in (1, 256, 512, T - 1):
            def position(w):
                def run(i):
                    m._spatial_step(sts[w], t, codes[:, t - 1, :])
                    for d in range(D):
                        m._depth_step(sts[w], t, d, None if d == 0 else codes[:, t, :d], False, False)
                        _C.sample_logits(sts[w]["logits"], codes[:, t, d], top_k=None, top_p=None, seed=1, step=t * D + d)
                return run
            h, f = alternate([position("h16"), position("fp8")], inner=10)
            n_sp, n_dp = launches_per_position(b, C, V, D, Ls, Ld, t)
            lines.append(f"{b:>5} {t:>5} {f3(h):>28} {f3(f):>28} {h[1] / f[1]:>10.3f} {'yes' if f[2] < h[0] else 'no':>13} {n_sp + n_dp:>8}")
        del sts
        torch.cuda.empty_cache()
    lines.append("beyond spread: the slowest fp8 window is faster than the fastest 16-bit window of the same point")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def fp4_mode(kw, out):
    """--weights fp4: one position (the spatial step, the D depth steps, their draws) with MXFP4 Block weights against MXFP8 and 16-bit weights, the
    three alternating"""
    C, V, T, D = kw["embed_dim"], kw["vocab_img_size"], kw["img_num_tokens"], kw["depth_num_tokens"]
    Ls, Ld = kw["spatial_n_layers"], kw["depth_n_layers"]
    dt = torch.float16
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(**kw)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    blocks = 12 * C * C * Ls + D * 12 * C * C * Ld
    w16, w8, w4 = (blocks + D * V * C) * 2, blocks + blocks // 32 + D * V * C * 2, blocks // 2 + blocks // 32 + D * V * C * 2
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    forms = ("h16", "fp8", "fp4")
    lines = [f"stage-2 RQTransformer sampling, MXFP4 Block weights against MXFP8 and 16-bit weights, on {torch.cuda.get_device_name(0)}: C={C} spatial "
             f"layers={Ls} depth layers={Ld} T={T} D={D} V={V}, fp16 activations and caches",
             f"GEMM weights read per position {w16 / 1e9:.3f} GB (16-bit) / {w8 / 1e9:.3f} GB (fp8) / {w4 / 1e9:.3f} GB (fp4: codes + scales + the 16-bit "
             f"head, read {D} times)",
             "ms per position (spatial step + the D depth steps with their draws): median [min .. max] of 7 rounds of alternating windows of 10 positions in "
             "one process",
             f"{'batch':>5} {'slot':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'fp4 ms [min .. max]':>28} {'16-bit/fp4':>10} {'fp8/fp4':>8} "
             f"{'beyond fp8':>10} {'beyond 16-bit':>13}"]
    for b in (1, 4):
        sts = {w: m._decode_state(b, dt, "cuda", w) for w in forms}
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        for t in (1, 256, 512, T - 1):
            def position(w):
                def run(i):
                    m._spatial_step(sts[w], t, codes[:, t - 1, :])
                    for d in range(D):
                        m._depth_step(sts[w], t, d, None if d == 0 else codes[:, t, :d], False, False)
                        _C.sample_logits(sts[w]["logits"], codes[:, t, d], top_k=None, top_p=None, seed=1, step=t * D + d)
                return run
            h, e, f = alternate([position(w) for w in forms], inner=10)
            lines.append(f"{b:>5} {t:>5} {f3(h):>28} {f3(e):>28} {f3(f):>28} {h[1] / f[1]:>10.3f} {e[1] / f[1]:>8.3f} {'yes' if f[2] < e[0] else 'no':>10} "
                         f"{'yes' if f[2] < h[0] else 'no':>13}")
        del sts
        torch.cuda.empty_cache()
    lines.append("beyond fp8 / 16-bit: the slowest fp4 window is faster than the fastest fp8 / 16-bit window of the same point")
    held = lambda w: sum(t.numel() * t.element_size() for k, st in m._sample_operands(dt, w).items() if k != "head" for W in st
                         for n in ("wqkv", "wproj", "w0", "w1") for t in W[n])
    lines.append(f"operand copies of the Blocks held by the process: {held('fp4') / 1e9:.3f} GB (fp4) against {held('fp8') / 1e9:.3f} GB (fp8)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def fp6_mode(kw, out):
    """--weights fp6: one position (the spatial step, the D depth steps, their draws) with MXFP6 Block weights against 16-bit, MXFP8 and MXFP4
    weights, the four alternating"""
    C, V, T, D = kw["embed_dim"], kw["vocab_img_size"], kw["img_num_tokens"], kw["depth_num_tokens"]
    Ls, Ld = kw["spatial_n_layers"], kw["depth_n_layers"]
    dt = torch.float16
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(**kw)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    blocks = 12 * C * C * Ls + D * 12 * C * C * Ld
    head = D * V * C * 2
    w16, w8, w6, w4 = blocks * 2 + head, blocks + blocks // 32 + head, blocks * 3 // 4 + blocks // 32 + head, blocks // 2 + blocks // 32 + head
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    forms = ("h16", "fp8", "fp6", "fp4")
    lines = [f"stage-2 RQTransformer sampling, MXFP6 Block weights against 16-bit, MXFP8 and MXFP4 weights, on {torch.cuda.get_device_name(0)}: C={C} spatial "
             f"layers={Ls} depth layers={Ld} T={T} D={D} V={V}, fp16 activations and caches",
             f"GEMM weights read per position {w16 / 1e9:.3f} GB (16-bit) / {w8 / 1e9:.3f} GB (fp8) / {w6 / 1e9:.3f} GB (fp6) / {w4 / 1e9:.3f} GB (fp4: codes + "
             f"scales + the 16-bit head, read {D} times)",
             "ms per position (spatial step + the D depth steps with their draws): median [min .. max] of 7 rounds of alternating windows of 10 positions in "
             "one process",
             f"{'batch':>5} {'slot':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'fp6 ms [min .. max]':>28} {'fp4 ms [min .. max]':>28} "
             f"{'fp8/fp6':>8} {'fp6/fp4':>8} {'not slower':>10} {'beyond fp8':>10}"]
    for b in (1, 4):
        sts = {w: m._decode_state(b, dt, "cuda", w) for w in forms}
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        for t in (1, T - 1):
            def position(w):
                def run(i):
                    m._spatial_step(sts[w], t, codes[:, t - 1, :])
                    for d in range(D):
                        m._depth_step(sts[w], t, d, None if d == 0 else codes[:, t, :d], False, False)
                        _C.sample_logits(sts[w]["logits"], codes[:, t, d], top_k=None, top_p=None, seed=1, step=t * D + d)
                return run
            h, e, s, f = alternate([position(w) for w in forms], inner=10)
            lines.append(f"{b:>5} {t:>5} {f3(h):>28} {f3(e):>28} {f3(s):>28} {f3(f):>28} {e[1] / s[1]:>8.3f} {s[1] / f[1]:>8.3f} "
                         f"{'yes' if s[2] <= e[2] else 'NO':>10} {'yes' if s[2] < e[0] else 'no':>10}")
        del sts
        torch.cuda.empty_cache()
    lines.append("not slower: the slowest fp6 window is no slower than the slowest fp8 window of the same point; beyond fp8: it is faster than the fastest fp8 window")
    held = lambda w: sum(t.numel() * t.element_size() for k, st in m._sample_operands(dt, w).items() if k != "head" for W in st
                         for n in ("wqkv", "wproj", "w0", "w1") for t in W[n])
    lines.append(f"operand copies of the Blocks held by the process: {held('fp6') / 1e9:.3f} GB (fp6) against {held('fp8') / 1e9:.3f} GB (fp8) and "
                 f"{held('fp4') / 1e9:.3f} GB (fp4)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def kv8_mode(kw, out):
    """--cache fp8: one position (the spatial step, the D depth steps, their draws) with MXFP8 spatial k / v caches against 16-bit caches"""
    C, V, T, D = kw["embed_dim"], kw["vocab_img_size"], kw["img_num_tokens"], kw["depth_num_tokens"]
    Ls, Ld = kw["spatial_n_layers"], kw["depth_n_layers"]
    dt = torch.float16
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(**kw)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    f3 = lambda v: f"{v[1]:.3f} [{v[0]:.3f} .. {v[2]:.3f}]"
    held = lambda b, per: 2 * Ls * b * T * per
    lines = [f"stage-2 RQTransformer sampling, MXFP8 spatial k / v caches against 16-bit caches, on {torch.cuda.get_device_name(0)}: C={C} spatial layers={Ls} "
             f"depth layers={Ld} T={T} D={D} V={V}, fp16 activations, 16-bit weights; the depth caches ({D} slots) are 16-bit in both",
             f"spatial caches held at batch 64: {held(64, 2 * C) / 1e9:.2f} GB (16-bit) / {held(64, C + C // 32) / 1e9:.2f} GB (fp8: codes + scales)",
             "ms per position (spatial step + the D depth steps with their draws): median [min .. max] of 7 alternating windows of 10 positions in one process",
             f"{'batch':>5} {'slot':>5} {'16-bit ms [min .. max]':>28} {'fp8 ms [min .. max]':>28} {'16-bit/fp8':>10} {'beyond spread':>13} {'launches':>8}"]
    for b in (1, 4, 64):
        sts = {c: m._decode_state(b, dt, "cuda", "h16", c) for c in ("h16", "fp8")}
        for kv in sts["h16"]["spatial"]:
            for z in kv:
                z.normal_(0, 0.5)
        for kv in sts["fp8"]["spatial"]:
            for codes8, scales in (kv[:2], kv[2:]):
                codes8.random_(0, 256).bitwise_and_(0xF7)      # no NaN code
                scales.random_(118, 122)
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        for t in (1, 256, 512, T - 1):
            def position(c):
                def run(i):
                    m._spatial_step(sts[c], t, codes[:, t - 1, :])
                    for d in range(D):
                        m._depth_step(sts[c], t, d, None if d == 0 else codes[:, t, :d], False, False)
                        _C.sample_logits(sts[c]["logits"], codes[:, t, d], top_k=None, top_p=None, seed=1, step=t * D + d)
                return run
            h, f = alternate([position("h16"), position("fp8")], inner=10)
            n_sp, n_dp = launches_per_position(b, C, V, D, Ls, Ld, t)
            lines.append(f"{b:>5} {t:>5} {f3(h):>28} {f3(f):>28} {h[1] / f[1]:>10.3f} {'yes' if f[2] < h[0] else 'no':>13} {n_sp + n_dp:>8}")
        del sts
        torch.cuda.empty_cache()
    lines.append("beyond spread: the slowest fp8 window is faster than the fastest 16-bit window of the same point")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--spatial_layers", type=int, default=None)
    ap.add_argument("--graph", action="store_true", help="instead of the tables: the eager loop against replays of one captured position "
                    "(profiles/rq_sample_graph.txt)")
    ap.add_argument("--whole", type=int, default=1, help="--graph: also draw one whole image through sample() both ways")
    ap.add_argument("--weights", choices=("h16", "fp8", "fp6", "fp4"), default="h16", help="fp8: instead of the tables, one position with MXFP8 Block weights "
                    "against 16-bit weights (profiles/rq_sample_fp8.txt); fp4: with MXFP4 Block weights against both (profiles/rq_sample_fp4.txt); "
                    "fp6: with MXFP6 Block weights against all three (profiles/rq_sample_fp6.txt)")
    ap.add_argument("--cache", choices=("h16", "fp8"), default="h16", help="fp8: instead of the tables, one position with MXFP8 spatial k / v caches "
                    "against 16-bit caches (profiles/rq_sample_kv8.txt)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "rq_sample_graph.txt" if args.graph else "rq_sample_kv8.txt" if args.cache == "fp8" else
                                dict(h16="rq_sample.txt", fp8="rq_sample_fp8.txt", fp6="rq_sample_fp6.txt", fp4="rq_sample_fp4.txt")[args.weights])
    kw = dict(get_config_from_file(os.path.join(ROOT, "configs", "imagenet_rqtransformer_rqvae_base.yaml")).model.params.transformer.params)
    if args.spatial_layers is not None:
        kw["spatial_n_layers"] = args.spatial_layers
    if args.graph:
        return graph_mode(kw, args.out, bool(args.whole))
    if args.cache == "fp8":
        return kv8_mode(kw, args.out)
    if args.weights == "fp8":
        return fp8_mode(kw, args.out)
    if args.weights == "fp4":
        return fp4_mode(kw, args.out)
    if args.weights == "fp6":
        return fp6_mode(kw, args.out)
    C, V, T, D = kw["embed_dim"], kw["vocab_img_size"], kw["img_num_tokens"], kw["depth_num_tokens"]
    Hs, Hd, Ls, Ld = kw["spatial_n_heads"], kw["depth_n_heads"], kw["spatial_n_layers"], kw["depth_n_layers"]
    dt = torch.float16
    f3 = lambda v, k=1.0: f"{v[1] * k:.3f} [{v[0] * k:.3f} .. {v[2] * k:.3f}]"
    f1 = lambda v: f"{v[1] * 1e3:.1f} [{v[0] * 1e3:.1f} .. {v[2] * 1e3:.1f}]"
    lines = [f"stage-2 RQTransformer sampling on {torch.cuda.get_device_name(0)}: C={C} spatial layers={Ls} depth layers={Ld} heads={Hs} x {C // Hs} | "
             f"{Hd} x {C // Hd} T={T} D={D} V={V}, fp16 operands",
             "times: median [min .. max] of 7 alternating windows of back-to-back calls, after a warm-up of every path",
             f"depth decode attention alone, batch x {Hd} heads of {C // Hd}, cache of {D} slots, steps d = 0 .. {D - 1} in turn: windows of 200 launches",
             f"{'batch':>5} {'short us [min .. max]':>28} {'general us [min .. max]':>28} {'general/short':>13} {'spread-free':>11} {'max |diff|':>10}"]
    all_faster = True
    for b in (1, 4):
        hs = C // Hd
        qkv = torch.randn(b, 3 * C, device="cuda").to(dt)
        ks, vs, kg, vg = (torch.zeros(b, Hd, D, hs, device="cuda", dtype=dt) for _ in range(4))
        o_s, o_g = torch.empty(b, C, device="cuda", dtype=dt), torch.empty(b, C, device="cuda", dtype=dt)
        s, g = alternate([lambda i: _C.short_decode_attention(qkv, ks, vs, i % D, o_s), lambda i: _C.decode_attention(qkv, kg, vg, i % D, o_g)], inner=200)
        _C.short_decode_attention(qkv, ks, vs, D - 1, o_s)
        _C.decode_attention(qkv, kg, vg, D - 1, o_g)
        faster = s[2] < g[0]      # the slowest window of the new kernel against the fastest of the old one: beyond the spread of both
        all_faster &= faster
        lines.append(f"{b:>5} {f1(s):>28} {f1(g):>28} {g[1] / s[1]:>13.2f} {'yes' if faster else 'NO':>11} {(o_s.float() - o_g.float()).abs().max().item():>10.1e}")
    lines.append(f"short kernel faster than the general kernel beyond the run-to-run spread at every point: {'yes' if all_faster else 'NO'}")
    torch.manual_seed(0)
    with torch.device("cuda"):
        m = RQTransformer(**kw)
        with torch.no_grad():
            for p in (m.pos_emb_cond, m.pos_emb_code, m.pos_emb_depth):
                p.normal_(0, 0.02)
    wb_spatial, wb_depth = 12 * C * C * Ls * 2, D * (12 * C * C * Ld + V * C) * 2
    lines += [f"one position, fp16 operands: windows of 10 positions; GEMM weights read per position {wb_spatial / 1e9:.3f} GB (spatial) + {wb_depth / 1e9:.3f} GB "
              f"({D} depth steps with the head) = {(wb_spatial + wb_depth) / 1e9:.3f} GB; a plain copy reaches {COPY_TBS} TB/s",
              f"(the depth stack and the head, {wb_depth / D / 1e6:.0f} MB, are re-read {D} times per position and fit the 256 MiB last-level cache: their rate can pass the HBM rate)",
              f"{'batch':>5} {'slot':>5} {'spatial ms [min .. max]':>28} {'depth ms, short [min .. max]':>30} {'depth ms, general [min .. max]':>31} {'position ms':>11} "
              f"{'torch ms [min .. max]':>28} {'torch/dev':>9} {'launches':>9} {'weights TB/s':>12} {'of copy':>8}"]
    per_image = {}
    for b in (1, 4):
        st = m._decode_state(b, dt, "cuda")
        codes = torch.randint(0, V, (b, T, D), device="cuda")
        tp = TorchPosition(m, b)
        pos_ms = []
        for t in (1, 256, 512, T - 1):
            def spatial(i):
                m._spatial_step(st, t, codes[:, t - 1, :])

            def depth(cache):
                def run(i):
                    for d in range(D):
                        m._depth_step(st, t, d, None if d == 0 else codes[:, t, :d], False, cache)
                        _C.sample_logits(st["logits"], codes[:, t, d], top_k=None, top_p=None, seed=1, step=t * D + d)
                return run
            sp, ds, dg, tr = alternate([spatial, depth(False), depth(True), lambda i: tp(t, codes)], inner=10)
            n_sp, n_dp = launches_per_position(b, C, V, D, Ls, Ld, t)
            pos = sp[1] + ds[1]
            pos_ms.append(pos)
            tbs = (wb_spatial + wb_depth) / (pos * 1e-3) / 1e12
            lines.append(f"{b:>5} {t:>5} {f3(sp):>28} {f3(ds):>30} {f3(dg):>31} {pos:>11.3f} {f3(tr):>28} {tr[1] / pos:>9.2f} {n_sp + n_dp:>9} {tbs:>12.2f} "
                         f"{100 * tbs / COPY_TBS:>7.1f}%")
        per_image[b] = statistics.mean(pos_ms) * T / 1e3
        del st, tp
        torch.cuda.empty_cache()
    n_sp, n_dp = launches_per_position(4, C, V, D, Ls, Ld, T - 1)
    lines.append(f"launches per position at batch 4, slot {T - 1}: {n_sp} (spatial step) + {n_dp} ({D} depth steps with their draws) = {n_sp + n_dp}")
    for b, s in per_image.items():
        lines.append(f"extrapolated whole image, batch {b}: mean position time of the four fills x {T} positions = {s:.2f} s ({s / b:.2f} s per image)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
