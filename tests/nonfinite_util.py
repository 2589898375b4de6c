"""What a non-finite value does on its way through a kernel: three assertions shared by the tests/test_nonfinite_*_gpu.py files (and proven on CPU
emulations, with injected faults, by tests/test_nonfinite_util_cpu.py).

fp16 training rests on ONE assumption: an overflow anywhere in a loss-scaled step reaches the flat gradient as an inf or a NaN, where
enh_nonfinite_flag / enh_grad_clip_coef see it and the step is dropped.  A kernel breaks it by turning the overflow back into a finite number (a
saturating pack, an fmax or a select that drops a NaN, a masked product that flushes it) or by letting it reach data it does not belong to (a clamped
row that reads the neighbouring image).  The references are plain float64 evaluations of each operation's formula ON THE POISONED INPUTS: IEEE
arithmetic does the propagating.

  assert_no_swallow  wherever the reference is non-finite, so is the kernel's output (inf and NaN are not told apart: which one a sum ends as depends
                     on its order).  Returns the number of SPURIOUS elements (kernel non-finite, reference finite): reported by the caller, not a fault.
  assert_isolated    outside the units that share data with the poisoned element (a GEMM row or column, a LayerNorm row, an (image, head) of
                     attention, a column of a column sum) the poisoned run equals the clean run bit for bit.
  check_overflow     fp16 results past 65520: +-inf exactly where the correctly rounded reference is +-inf, no NaN, no 65504 there, and the finite
                     part inside the bound the caller brings (exact=True); for a kernel with a 16-bit intermediate (exact=False) fp16(ref) = +-inf
                     implies non-finite, and whatever is finite stays inside the bound.

No tolerance is introduced here: every bound is the caller's (util.elem_bound, the 1.25 x floor of the loss-network tests, ...)."""
import math

import pytest
import torch

from util import assert_elementwise, floor16, rel

BF16, F16 = torch.bfloat16, torch.float16
_BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def _host(t):
    return t.detach().cpu()


@pytest.fixture(autouse=True)
def scrub_shared_buffers():
    """(imported by the GPU files: autouse there)  A poisoned launch leaves inf / NaN in the grow-only workspaces that enhancing._C shares among
    all callers of a process (split-K slabs, LayerNorm and column-sum partials, the attention backward's delta).  No kernel may read what it did not
    write there — but these tests are not the place to find out which later test would: the workspaces are zeroed after every test."""
    yield
    if torch.cuda.is_available():
        from enhancing import _C
        torch.cuda.synchronize()
        for ws in list(_C._WS.values()) + list(_C._GEMM_WS.values()):
            ws.zero_()
        torch.cuda.synchronize()


def nonfinite(t: torch.Tensor) -> torch.Tensor:
    return ~torch.isfinite(_host(t))


def assert_no_swallow(got: torch.Tensor, ref: torch.Tensor, what: str, dt=None) -> int:
    """`got`: the kernel's output (any dtype), `ref`: float64 on the poisoned inputs, same shape.  dt: the stored format the reference is rounded to
    first (default: got's own dtype when that is a 16-bit one; an f32 output is compared with the unrounded reference).  Returns the spurious count."""
    got, ref = _host(got), _host(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if dt is None and got.dtype in (BF16, F16):
        dt = got.dtype
    want = ~torch.isfinite(ref.to(dt) if dt is not None else ref)
    have = ~torch.isfinite(got)
    swallowed = want & ~have
    if bool(swallowed.any()):
        idx = tuple(int(v) for v in swallowed.nonzero()[0])
        raise AssertionError(f"{what}: {int(swallowed.sum())} of {int(want.sum())} non-finite reference elements came out finite, the first at {idx}: "
                             f"out {got[idx].item()!r}, ref {ref[idx].item()!r}")
    return int((have & ~want).sum())


def assert_isolated(got_poisoned: torch.Tensor, got_clean: torch.Tensor, unit_mask, what: str) -> None:
    """unit_mask: bool, broadcastable to the outputs; True inside the units that share data with the poisoned element.  Everything outside equals the
    clean run bit for bit."""
    p, c = _host(got_poisoned).contiguous(), _host(got_clean).contiguous()
    assert p.shape == c.shape and p.dtype == c.dtype, (what, p.shape, c.shape, p.dtype, c.dtype)
    bits = _BITS[p.element_size()]
    outside = ~torch.as_tensor(unit_mask, dtype=torch.bool).expand(p.shape)
    assert bool(outside.any()), f"{what}: the unit mask covers the whole output: nothing is checked"
    diff = (p.view(bits) != c.view(bits)) & outside
    if bool(diff.any()):
        idx = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} elements outside the poisoned unit differ from the clean run, the first at {idx}: "
                             f"{p[idx].item()!r} against {c[idx].item()!r}")


def pow2_scale(unit: torch.Tensor, target: float = 4e4) -> float:
    """the power of two that takes the rms of a result computed on unit-scale operands to ~target (4e4: ~10-30 % of the results past 65520); scaling an
    fp16 operand by it is exact"""
    return 2.0 ** round(math.log2(target / unit.double().pow(2).mean().sqrt().item()))


def floor_bound(limit: float = 1.25, dt=F16):
    """bound_fn of the loss-network tests: relative Frobenius error of the finite part <= limit x its rounding floor"""
    def fn(got, ref, what):
        return rel(got, ref) / floor16(ref, dt), limit, "x floor"
    return fn


def element_bound(bound: torch.Tensor):
    """bound_fn from a per-element bound (util.elem_bound) of the whole output: every finite element inside it"""
    bound = _host(bound).double()

    def fn(got, ref, what, sel):
        return assert_elementwise(got[sel], ref[sel], bound[sel], what), 1.0, "of the element bound"
    fn.wants_mask = True
    return fn


def check_overflow(got: torch.Tensor, ref: torch.Tensor, bound_fn, what: str, exact: bool = True) -> int:
    """got: the kernel's fp16 output (any layout; converted to f32 on the host), ref: the exact result in float64, same layout.  bound_fn(got, ref, what)
    -> (figure, limit, unit) judges the finite part, handed over as flat selections (floor_bound / element_bound).  Returns the spurious count (always 0 when exact)."""
    got, ref = _host(got).float(), _host(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    want = ref.to(F16)
    inf = torch.isinf(want)
    assert not torch.isnan(want).any(), f"{what}: the reference holds NaN"
    assert 0.001 <= inf.float().mean().item() <= 0.9, f"{what}: the case must overflow in part ({inf.float().mean().item():.4f})"
    if exact:
        assert not torch.isnan(got).any(), f"{what}: NaN"
        assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf].float()), f"{what}: +-inf must be exactly where fp16(ref) is"
        assert not (got.abs() == 65504.0)[inf].any()
        fin, spurious = ~inf, 0
    else:
        bad = inf & torch.isfinite(got)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {int(inf.sum())} overflowed results came out finite, the first {got[bad][0].item()!r}"
        fin = ~inf & torch.isfinite(got)
        spurious = int((~inf & ~torch.isfinite(got)).sum())
        assert bool(fin.any()), f"{what}: nothing finite is left to bound"
    # (a bound_fn marked wants_mask gets the whole tensors and the selection: a bound per element or per row needs the positions)
    e, limit, unit = bound_fn(got, ref, what, fin) if getattr(bound_fn, "wants_mask", False) else bound_fn(got[fin], ref[fin], what)
    print(f"overflow {what}: {inf.float().mean().item() * 100:.1f} % inf, finite part {e:.3f} {unit}" + ("" if exact else f", {spurious} spurious non-finite"))
    assert e <= limit, (what, e)
    return spurious


def assert_all_finite_within(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    """the bf16 twin of an fp16 overflow case: entirely finite and inside its element bound"""
    assert bool(torch.isfinite(_host(got).float()).all()), f"{what}: non-finite values in a format whose range holds the result"
    return assert_elementwise(got, ref, bound, what)
