"""Times the stage-2 optimizer step (engine/optim.py GPTAdam, csrc/gpt_adam.hip) at the shipped width (configs/imagenet_gpt_vitvq_base.yaml: C = 6144,
16 heads of 384, T = 1024, V = 8192; random weights, fp16 operands) and writes profiles/gpt_train.txt:
    python tools/gpt_train_bench.py [--out FILE] [--layers N] [--skip-torch]
    python tools/gpt_train_bench.py --adam-state bf16 [--layers N] [--append]      (-> profiles/gpt_train_adam16.txt, see adam16() below)

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


def adam16(args, say):
    """--adam-state bf16: GPTAdam's f32 moments against its bf16 moments (state="bf16": enh_adam_step_segments_s16, 22 bytes per element against 30) in
    ONE process over ONE model, the two alternating window by window: the optimizer is built with f32 state, a second pair of (bf16) moment buffers is
    allocated beside it and the optimizer's `m`, `v` and `state_format` are pointed at one pair or the other before each call.  Reported: the launch
    alone, GPTAdam.step, the whole training step at batch 1 and 4, and the peak device memory of a whole batch-4 step with only one format's moments
    resident (f32 before the bf16 pair is allocated, bf16 after the f32 pair is freed)."""
    C, H, V, T, L = 6144, 16, 8192, 1024, args.layers
    say(f"stage-2 optimizer step, f32 moments against bf16 moments, on {torch.cuda.get_device_name(0)}: C={C} layers={L} heads={H} x {C // H} T={T} V={V}, fp16 operands")
    say(f"times: median [min .. max] ms of {args.windows} windows of {args.reps} back-to-back calls, after a warm-up; the two formats alternate window by window")
    bw, ts = copy_bandwidth(args.windows, args.reps)
    say(f"copy bandwidth of this card, this run (4 GiB f32 copy_, read + written): {bw / 1e12:.2f} TB/s   ({fmt(ts)} ms)")
    m = build(L, C, H, V, T)
    opt = GPTAdam(m, lr=1e-4, state="f32")
    n, sc = opt.p.numel(), opt.scaler
    say(f"parameters: {sum(p.numel() for p in m.parameters()) / 1e9:.3f} G; flat buffers of {n / 1e9:.3f} G elements")
    batch = {}
    for b in (1, 4):
        g = torch.Generator().manual_seed(b)
        batch[b] = (torch.randint(0, V, (b, T), generator=g).cuda(), torch.randint(0, 1000, (b, 1), generator=g).cuda())

    def whole(b):
        m.forward_backward(*batch[b], loss_scale=opt.loss_scale)
        opt.step()

    def peak(b=4):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        whole(b)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() / 2 ** 30
    whole(4)      # warm-up: the activations' allocations
    peak32 = peak()
    pair = dict(f32=(opt.m, opt.v), bf16=(torch.zeros(n, dtype=torch.bfloat16, device="cuda"), torch.zeros(n, dtype=torch.bfloat16, device="cuda")))

    def use(state):
        (opt.m, opt.v), opt.state_format = pair[state], state

    def step_of(state):
        def f():
            use(state)
            opt.step()
        return f

    def whole_of(state, b):
        def f():
            use(state)
            whole(b)
        return f
    m.flat_grad.normal_(0, 1e-3).mul_(65536.0)
    kw = dict(lr=1e-4, skip_flag=sc.found_inf, loss_scale=sc.scale_t)
    res = timed(dict(kernel_f32=lambda: _C.adam_step_segments(opt.p, m.flat_grad, *pair["f32"], opt.arena, opt.table, opt.state, **kw),
                     kernel_bf16=lambda: _C.adam_step_segments_s16(opt.p, m.flat_grad, *pair["bf16"], opt.arena, opt.table, opt.state, seed=0, **kw),
                     step_f32=step_of("f32"), step_bf16=step_of("bf16")), args.windows, args.reps)
    assert float(sc.found_inf.item()) == 0.0, "the timed steps were dropped"
    med = lambda k: statistics.median(res[k])
    rate = lambda k, per: per * n / (med(k) * 1e-3)
    say("                                                     ms [min .. max]      bytes    rate      of the copy bandwidth")
    say(f"  enh_adam_step_segments alone      (f32 moments, 30 B) {fmt(res['kernel_f32'])}  {30 * n / 1e9:7.1f} GB {rate('kernel_f32', 30) / 1e12:6.2f} TB/s  {rate('kernel_f32', 30) / bw:6.1%}")
    say(f"  enh_adam_step_segments_s16 alone (bf16 moments, 22 B) {fmt(res['kernel_bf16'])}  {22 * n / 1e9:7.1f} GB {rate('kernel_bf16', 22) / 1e12:6.2f} TB/s  {rate('kernel_bf16', 22) / bw:6.1%}")
    say(f"  the bf16-moment launch takes {med('kernel_bf16') / med('kernel_f32'):.3f} of the f32-moment launch's time (22 / 30 = {22 / 30:.3f} by bytes) and keeps "
        f"{rate('kernel_bf16', 22) / rate('kernel_f32', 30):.1%} of its bandwidth")
    say(f"  GPTAdam.step, f32 moments  (found-inf + step + scale update + biases, 34 B) {fmt(res['step_f32'])}")
    say(f"  GPTAdam.step, bf16 moments (the same, 26 B)                                 {fmt(res['step_bf16'])}")
    for b in (1, 4):
        r = timed(dict(f32=whole_of("f32", b), bf16=whole_of("bf16", b)), max(3, args.windows // 2), 2, warm=1)
        a, c = statistics.median(r["f32"]), statistics.median(r["bf16"])
        spread = max(max(r[k]) - min(r[k]) for k in r)
        say(f"training step (forward_backward + step), batch {b}: f32 moments {fmt(r['f32'])} ms, bf16 moments {fmt(r['bf16'])} ms: "
            f"difference of the medians {a - c:+.3f} ms ({(a - c) / a:+.1%}), widest window spread {spread:.3f} ms -> "
            f"{'beyond' if abs(a - c) > spread else 'within'} the spread")
    use("bf16")
    del pair["f32"]
    peak16 = peak()
    say(f"peak device memory of a whole batch-4 step with one format's moments resident: f32 {peak32:.1f} GiB, bf16 {peak16:.1f} GiB "
        f"(m and v: {8 * n / 2 ** 30:.1f} GiB against {4 * n / 2 ** 30:.1f} GiB); loss scale now {opt.loss_scale.item():g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/gpt_train.txt, or profiles/gpt_train_adam16.txt with --adam-state bf16")
    ap.add_argument("--adam-state", choices=("f32", "bf16"), default="f32",
                    help="bf16: compare GPTAdam(state='bf16') with the f32 state in alternating windows instead of the run described above")
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
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gpt_train_adam16.txt" if args.adam_state == "bf16" else "gpt_train.txt")
    if args.adam_state == "bf16":
        adam16(args, say)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")
        return
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
