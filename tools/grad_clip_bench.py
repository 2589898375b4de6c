"""Times grad_sumsq_kernel (enh_grad_clip_coef's read pass) beside nonfinite_flag_kernel on the base model's flat gradient (170.66 M floats), in one process,
with the project's per-kernel timer (enhancing._C.KernelTimer: HIP events around each launch).  The two alternate launch by launch, so drift of the
device's clocks hits both alike.  Run on the GPU; prints the table that profiles/grad_clip.txt holds."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enhancing-transformers_amd"))
from enhancing import _C  # noqa: E402

N = int(os.environ.get("GC_N", 170_664_000))
ITERS, WARM = 50, 5


def main() -> None:
    assert torch.cuda.is_available(), "needs the GPU: a CPU run cannot time a kernel"
    g = torch.randn(N, device="cuda") * 0.01
    flag = torch.zeros(1, device="cuda")
    out = torch.zeros(2, device="cuda")
    scale = torch.full((1,), 65536.0, device="cuda")
    cases = {"nonfinite_flag_kernel": lambda: _C.nonfinite_flag(g, flag),
             "grad_sumsq_kernel": lambda: _C.grad_clip_coef(g, 1.0, 1.0, out, loss_scale=scale, found_inf=flag)}
    for _ in range(WARM):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    timer = _C.KernelTimer()
    _C.TIMER = timer
    try:
        for _ in range(ITERS):
            for fn in cases.values():
                fn()
    finally:
        _C.TIMER = None
    summ = timer.summary()
    ref = float(g.double().norm()) / 65536.0
    print(f"flat gradient: {N} f32 = {4 * N / 1e9:.3f} GB; {ITERS} alternating launches each after {WARM} warm-up; device {torch.cuda.get_device_name(0)}")
    for name in cases:
        ms = sorted(s.elapsed_time(e) for s, e, _ in timer.records[name])
        med = ms[len(ms) // 2]
        print(f"{name:24s} median {med:.4f} ms  min {ms[0]:.4f}  max {ms[-1]:.4f}  mean {summ[name]['avg_ms']:.4f}   {4 * N / med / 1e6:8.1f} GB/s (median)")
    a, b = (sorted(s.elapsed_time(e) for s, e, _ in timer.records[k])[ITERS // 2] for k in ("grad_sumsq_kernel", "nonfinite_flag_kernel"))
    print(f"grad_sumsq_kernel (incl. the one-workgroup finishing launch inside the event pair) / nonfinite_flag_kernel = {a / b:.3f}")
    print(f"total_norm {out[0].item():.9e} vs torch fp64 {ref:.9e} (rel {abs(out[0].item() - ref) / ref:.2e}); flag {flag.item()}")


if __name__ == "__main__":
    main()
