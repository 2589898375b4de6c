"""Time and peak memory of one GumbelQuantizer forward + backward, the torch path (fused=False: the [M, K] logits, noise and softmaxes in HBM) beside the
fused kernels (fused=True: csrc/gumbel.hip), in one process.  Shapes: M = 8*1024 and 128*1024 tokens, K = 8192, d = 32, tau = 1, training mode (soft).
Each timed window is ITERS forward + backward passes between two device events, ending in a synchronise; the two paths alternate round by round, so a
drift of the device's clocks hits both alike.  Peak memory is torch.cuda.max_memory_allocated over one pass, above what was allocated before it
(inputs and parameters; the kernel library's workspace is allocated inside the pass and counted).  The fused pass is also split into its two library
calls by the project's per-call timer (enhancing._C.KernelTimer: device events around each call).  Run on the GPU; prints the table that profiles/gumbel_fused.txt holds."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
from enhancing import _C  # noqa: E402
from enhancing.modules.stage1.quantizers import GumbelQuantizer  # noqa: E402

K, D, TAU = 8192, 32, 1.0
SHAPES = [int(m) for m in os.environ.get("GB_M", "8192,131072").split(",")]
ROUNDS, WARM = 5, 2


def one_pass(q, z, g):
    z.grad = None
    q.embedding.weight.grad = None
    zq, loss, _ = q(z)
    ((zq * g).sum() + loss).backward()


def main() -> None:
    assert torch.cuda.is_available(), "needs the GPU: a CPU run cannot time a kernel"
    print(f"device {torch.cuda.get_device_name(0)}; K = {K}, d = {D}, tau = {TAU}, soft (training mode); forward + backward of one level")
    for M in SHAPES:
        iters = 20 if M <= 16384 else 3
        gen = torch.Generator("cuda").manual_seed(M)
        z = torch.randn(M, D, device="cuda", generator=gen).requires_grad_(True)
        g = torch.randn(M, D, device="cuda", generator=gen)
        torch.manual_seed(0)
        qs = {"torch": GumbelQuantizer(D, K, temp_init=TAU).cuda(), "fused": GumbelQuantizer(D, K, temp_init=TAU, fused=True, seed=1).cuda()}
        qs["fused"].embedding.weight.data.copy_(qs["torch"].embedding.weight.data)
        peak = {}
        for name, q in qs.items():
            for _ in range(WARM):
                one_pass(q, z, g)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            one_pass(q, z, g)
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated() - base
        times = {name: [] for name in qs}
        for _ in range(ROUNDS):
            for name, q in qs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(iters):
                    one_pass(q, z, g)
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) / iters)
        timer = _C.KernelTimer()
        _C.TIMER = timer
        try:
            for _ in range(iters):
                one_pass(qs["fused"], z, g)
        finally:
            _C.TIMER = None
        torch.cuda.synchronize()
        calls = {}
        for label, recs in timer.records.items():
            ms = sorted(s.elapsed_time(e) for s, e, _ in recs)
            calls[label.split(" ")[0]] = (ms[len(ms) // 2], recs[0][2])
        assert sorted(calls) == ["gumbel_backward", "gumbel_forward"], sorted(timer.records)
        print(f"\nM = {M} tokens ([M, K] fp32 = {M * K * 4 / 2 ** 30:.2f} GiB); {ROUNDS} alternating rounds of {iters} passes after {WARM} warm-up passes")
        med = {}
        for name in qs:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            print(f"  {name:5s} forward + backward: median {med[name]:9.3f} ms  min {t[0]:9.3f}  max {t[-1]:9.3f}   peak memory above the inputs {peak[name] / 2 ** 20:10.1f} MiB")
        flop = 9 * 2.0 * M * K * 32
        for label in ("gumbel_forward", "gumbel_backward"):
            ms, work = calls[label]
            print(f"  fused {label} call (all its kernels, median of {iters}): {ms:9.3f} ms   {work / 1e12:.3f} TFLOP of products -> {work / ms / 1e9:6.1f} TFLOP/s of the call")
        print(f"  fused: nine M x K x 32 products = {flop / 1e12:.3f} TFLOP -> {flop / med['fused'] / 1e9:.1f} TFLOP/s of the pass (exact-f32 MFMA peak 157.3): "
              f"an end-to-end rate, not a kernel's share of peak")
        print(f"  torch / fused: time {med['torch'] / med['fused']:.2f} x, memory {peak['torch'] / max(peak['fused'], 1):.1f} x")


if __name__ == "__main__":
    main()
