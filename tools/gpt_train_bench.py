"""Times the stage-2 optimizer step (engine/optim.py GPTAdam, csrc/gpt_adam.hip) at the shipped width (configs/imagenet_gpt_vitvq_base.yaml: C = 6144,
16 heads of 384, T = 1024, V = 8192; random weights, fp16 operands) and writes profiles/gpt_train.txt:
    python tools/gpt_train_bench.py [--out FILE] [--layers N] [--skip-torch]

--layers defaults to 2 (0.98 G parameters; seconds and ~25 GB).  24 is the shipped depth: 10.98 G parameters, p + g + m + v + the arena = 198 GB
before activations; --skip-torch then leaves out yardstick (a), whose own state does not fit beside it.

The optimizer step alone, against
  (a) what the tree could do before this kernel: torch.optim.Adam(fused=True) with the two parameter groups on the same f32 parameters and
      gradients, plus the rebuild of the GEMM operand copies the way GPT._operand_copies does it (torch.cat + .to(fp16) per layer);
  (b) the byte floor: the step's bytes (30 per parameter: p, g, m, v read, p, m, v and the 16-bit operand written; + 4 per parameter for the found-inf
      pass over g) over the copy bandwidth THIS run measures on this card with a large device-to-device copy_ (read + written bytes over time).
Then a whole training step (forward_backward with the device loss scale + step) at batch 1 and 4, the step's share of it, and the peak device memory.

Every time is a median [min .. max] of `--windows` windows of `--reps` back-to-back calls between two device events, after a warm-up; the two
optimizers alternate window by window.  The card's clocks are whatever the driver chose: the device name and the measured copy bandwidth are the
record of the state it ran in."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from enhancing import _C  # noqa: E402
from enhancing.engine.optim import GPTAdam, gpt_param_groups  # noqa: E402
from gpt_backward_bench import build  # noqa: E402


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timed(fns, windows, reps, warm=2):
    """{name: [ms per call of every window]}; the functions alternate window by window"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, reps))
    return out


def fmt(ts):
    return f"{statistics.median(ts):9.3f} [{min(ts):.3f} .. {max(ts):.3f}]"


def copy_bandwidth(windows, reps):
    n = 1 << 30      # 4 GiB of f32 each way: far beyond every cache
    src, dst = torch.empty(n, device="cuda").normal_(), torch.empty(n, device="cuda")
    ts = timed(dict(copy=lambda: dst.copy_(src)), windows, reps)["copy"]
    del src, dst
    return 8.0 * n / (statistics.median(ts) * 1e-3), ts


def rebuild_copies(m, dt):
    """the operand copies as GPT._operand_copies builds them"""
    cast = lambda w: w.detach().to(dt).contiguous()
    out = []
    for blk in m.blocks:
        a, f = blk.attn, blk.mlp
        out.append((cast(torch.cat([a.query.weight, a.key.weight, a.value.weight], 0)), torch.cat([a.query.bias, a.key.bias, a.value.bias]).detach().float(),
                    cast(a.proj.weight), cast(f.p0.weight), cast(f.p1.weight)))
    out.append(cast(m.head.weight))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_train.txt"))
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--append", action="store_true", help="add this run's lines to --out instead of replacing it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpt_train_bench: needs the GPU (a time taken anywhere else says nothing about it)")
    os.environ["ENH_PRECISION"] = "fp16"
    C, H, V, T, L = 6144, 16, 8192, 1024, args.layers
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"stage-2 optimizer step on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} x {C // H} T={T} V={V}, fp16 operands")
    say(f"times: median [min .. max] ms of {args.windows} windows of {args.reps} back-to-back calls, after a warm-up; alternating where two are compared")
    bw, ts = copy_bandwidth(args.windows, args.reps)
    say(f"copy bandwidth of this card, this run (4 GiB f32 copy_, read + written): {bw / 1e12:.2f} TB/s   ({fmt(ts)} ms)")
    m = build(L, C, H, V, T)
    n_par = sum(p.numel() for p in m.parameters())
    say(f"parameters: {n_par / 1e9:.3f} G in {len(list(m.parameters()))} tensors")
    res = {}
    if not args.skip_torch:
        decay, no_decay = gpt_param_groups(m)
        P = dict(m.named_parameters())
        for p in P.values():
            p.grad = torch.empty_like(p).normal_(0, 1e-3)
        topt = torch.optim.Adam([dict(params=[P[k] for k in decay], weight_decay=0.01), dict(params=[P[k] for k in no_decay], weight_decay=0.0)],
                                lr=1e-4, betas=(0.9, 0.96), fused=True)
        keep = []

        def torch_step():
            topt.step()
            keep[:] = rebuild_copies(m, torch.float16)
        res.update(timed(dict(torch_adam=topt.step, torch_total=torch_step), args.windows, args.reps))
        del topt, keep
        for p in P.values():
            p.grad = None
        torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    opt = GPTAdam(m, lr=1e-4)
    m.flat_grad.normal_(0, 1e-3).mul_(65536.0)
    n = opt.p.numel()
    sc = opt.scaler

    def kernel_only():
        _C.adam_step_segments(opt.p, m.flat_grad, opt.m, opt.v, opt.arena, opt.table, opt.state, lr=1e-4, skip_flag=sc.found_inf, loss_scale=sc.scale_t)
    res.update(timed(dict(step=opt.step, kernel=kernel_only), args.windows, args.reps))
    assert opt.state_dict is not None and float(sc.found_inf.item()) == 0.0, "the timed steps were dropped"
    by = lambda per: per * n
    med = lambda k: statistics.median(res[k])
    say("optimizer step alone                                       ms [min .. max]      bytes    rate      of the copy bandwidth")
    say(f"  GPTAdam.step (found-inf + step + scale update + biases) {fmt(res['step'])}  {by(34) / 1e9:7.1f} GB {by(34) / med('step') / 1e9:6.2f} TB/s  {by(34) / med('step') / 1e-3 / bw:6.1%}")
    say(f"  enh_adam_step_segments alone                            {fmt(res['kernel'])}  {by(30) / 1e9:7.1f} GB {by(30) / med('kernel') / 1e9:6.2f} TB/s  {by(30) / med('kernel') / 1e-3 / bw:6.1%}")
    say(f"  (b) byte floor at the copy bandwidth: step {by(34) / bw * 1e3:.3f} ms, kernel {by(30) / bw * 1e3:.3f} ms")
    if not args.skip_torch:
        say(f"  (a) torch.optim.Adam(fused=True), two groups            {fmt(res['torch_adam'])}")
        say(f"  (a) the same + operand copies by torch.cat + .to()      {fmt(res['torch_total'])}   (a) / GPTAdam.step = {med('torch_total') / med('step'):.2f}")
        assert med("step") < med("torch_total"), "acceptance: the step must be faster than (a)"
    else:
        say("  (a) torch.optim.Adam(fused=True) + copies: not measured in this run (--skip-torch)")
    for b in (1, 4):
        g = torch.Generator().manual_seed(b)
        codes, conds = torch.randint(0, V, (b, T), generator=g).cuda(), torch.randint(0, 1000, (b, 1), generator=g).cuda()

        def fb():
            m.forward_backward(codes, conds, loss_scale=opt.loss_scale)

        def whole():
            fb()
            opt.step()
        r = timed(dict(fb=fb, whole=whole), max(3, args.windows // 2), 2, warm=1)
        mf, mw = statistics.median(r["fb"]), statistics.median(r["whole"])
        say(f"training step, batch {b}: forward_backward {fmt(r['fb'])} ms, + optimizer step {fmt(r['whole'])} ms: the step is {(mw - mf) / mw:.1%} of the whole; "
            f"loss scale now {opt.loss_scale.item():g}")
    say(f"peak device memory since the optimizer was built: {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
