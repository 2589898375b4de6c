"""enh_adam_step_segments_s16 (csrc/gpt_adam.hip) alone: Adam with bf16 moments, widened exactly, p updated from the unrounded f32 moments, the stored
moments rounded stochastically with Philox words of (seed, group of 4 elements, applied step count) — the contract of include/enh_hip.h.

Layout (the idea of tests/test_gpt_adam_kernel_gpu.py, restated): segment sizes 64, 128, 192, 1088, 6144 and 262208 with the decay alternating
0.01 / 0, so the bounds 64 and 192 fall inside one wave access, 384, 448 and 1536 inside the first 4096-element tile and 8192 on a tile edge; padding
(canaries) sits at 384, 7680 and behind the last segment.  Three consecutive 6144-element sources land as q | k | v in the arena; every second other
segment has no destination; the arena's head, a gap in its middle and its tail are no destination (canaries).  The small case has 290 k elements; the
large one adds 32 segments of 262208 elements: 2120 tiles against the 2048 workgroups of a 256-CU grid, so a workgroup's second tile crosses
segments.  Only the one-step check runs at that size.

Limits.  p: tests/gpt_train_util.py's rule (4 x torch's f32 error against fp64 + one f32 ulp) against the fp64 step from the decoded old moments.
Stored moments: bracketed by the truncated and the rounded-up image, one bf16 ulp apart, with the fp64 moment between them up to the f32 allowance of
the same rule.  Statistics: 6 sigma of the mean's own deviation, worked out in the tests."""
import pytest
import torch

import adam16_util as AU
import gpt_train_util as TU

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
LR = 1e-3
CANARY, CANARY16, ACANARY = 12345.0, 12288.0, 768.0      # 12288 = 1.5 x 2^13 is a bf16 value
SEED = 0x5EED0123456789AB


def _layout(extra):
    """(segments [(begin, end, dst16, wd)], n, arena_n)"""
    sizes = [64, 128, 192, "gap64", 1088, 6144, "gap512", 262208, 6144, 6144, 6144, 1088, "gap64", 64] + [262208] * extra
    segs, at, k = [], 0, 0
    for s in sizes:
        if isinstance(s, str):
            at += int(s[3:])
            continue
        segs.append([at, at + s, -1, TU.WD if k % 2 == 0 else 0.0])
        at += s
        k += 1
    n = at + 64
    assert [segs[i][0] for i in (1, 2, 3, 4, 5)] == [64, 192, 448, 1536, 8192] and segs[2][1] == 384
    d = 64
    for i in (7, 6, 8):                             # key, query, value in registration order -> q | k | v
        segs[i][2] = d
        d += 6144
    d += 128                                        # a gap no segment writes
    for i in [j for j in range(len(segs)) if j not in (6, 7, 8)][::-2]:
        segs[i][2] = d
        d += segs[i][1] - segs[i][0]
    return [tuple(s) for s in segs], n, d + 64


LAYOUTS = {"small": _layout(0), "large": _layout(32)}
assert LAYOUTS["small"][1] < 300_000 and LAYOUTS["large"][1] > 2048 * 4096
_DATA = {}


def _data(size):
    """f32 p and four gradients like the f32 kernel test's, bf16 moments: m ~ 1e-3, v >= 0 spanning (1e-3)^2, a slice near eps^2, exact zeros; drawn once.
    [512, 576) (inside the segment [448, 1536), which has no decay) has g = m = v = 0: every new moment there is exactly 0."""
    if size not in _DATA:
        n = LAYOUTS[size][1]
        g = torch.Generator().manual_seed(11)
        D = dict(p=(0.02 * torch.randn(n, generator=g)).float(), g=[])
        for _ in range(4):
            x = 1e-3 * torch.randn(n, generator=g)
            x[1536:3000] *= 1e-5
            x[3000:3500] = 0.0
            x[512:576] = 0.0
            D["g"].append(x.float())
        m = 1e-3 * torch.randn(n, generator=g)
        v = (1e-3 * torch.randn(n, generator=g)) ** 2
        m[1536:3000] *= 1e-5
        v[1536:3000] = 1e-16 * torch.rand(1464, generator=g)
        m[3000:3500] = 0.0
        v[3000:3500] = 0.0
        m[512:576] = 0.0
        v[512:576] = 0.0
        D["m"], D["v"] = m.bfloat16(), v.bfloat16()
        _DATA[size] = D
    return _DATA[size]


class Dev:
    """device buffers with canaries in the padding of p, m16, v16 and in the arena's non-destination elements"""

    def __init__(self, dt, size="small", moments=True):
        from enhancing import _C
        self.segs, self.n, self.arena_n = LAYOUTS[size]
        D = _data(size)
        self.dt = dt
        self.mask = torch.zeros(self.n, dtype=torch.bool)
        for b, e, _, _ in self.segs:
            self.mask[b:e] = True
        pad = ~self.mask
        p = D["p"].clone(); p[pad] = CANARY
        m = D["m"].clone() if moments else torch.zeros(self.n, dtype=torch.bfloat16)
        v = D["v"].clone() if moments else torch.zeros(self.n, dtype=torch.bfloat16)
        m[pad] = CANARY16; v[pad] = CANARY16
        self.p0, self.m0, self.v0 = p.clone(), m.clone(), v.clone()
        self.p, self.m, self.v = p.cuda(), m.cuda(), v.cuda()
        self.arena = torch.full((self.arena_n,), ACANARY, dtype=dt).cuda()
        self.amask = torch.zeros(self.arena_n, dtype=torch.bool)
        for b, e, d, _ in self.segs:
            if d >= 0:
                self.amask[d:d + e - b] = True
        self.table = _C.adam_segment_table(self.segs, self.n, self.arena_n, "cuda")
        self.state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).cuda()
        self.wd = torch.zeros(self.n, dtype=torch.float64)
        for b, e, _, w in self.segs:
            self.wd[b:e] = w

    def step(self, g, seed=SEED, **kw):
        from enhancing import _C
        _C.adam_step_segments_s16(self.p, g.cuda(), self.m, self.v, self.arena, self.table, self.state, lr=LR, beta1=TU.BETAS[0], beta2=TU.BETAS[1],
                                  eps=TU.EPS, seed=seed, **kw)

    def bits(self):
        view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}
        return [t.clone().view(view[t.dtype]).cpu() for t in (self.p, self.m, self.v, self.arena, self.state)]

    def check_canaries_and_arena(self):
        pad = ~self.mask
        assert bool((self.p.cpu()[pad] == CANARY).all()), "the padding of p was written"
        for name, t in (("m16", self.m), ("v16", self.v)):
            assert bool((t.cpu()[pad].float() == CANARY16).all()), f"the padding of {name} was written"
        assert bool((self.arena.cpu()[~self.amask].float() == ACANARY).all()), "an arena element that is no destination was written"
        want = self.p.to(self.dt)       # round-to-nearest-even of the device's new p
        for b, e, d, _ in self.segs:
            if d >= 0:
                assert torch.equal(self.arena[d:d + e - b].view(torch.int16), want[b:e].view(torch.int16)), f"arena image of segment [{b}, {e})"


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _one_step_refs(dev, g):
    """the step t = 1 from the decoded old moments in fp64 and, for the allowance, in f32 with torch's operations: (p, m, v) each"""
    m0, v0 = AU.decode16(AU.bf16_bits(dev.m0)), AU.decode16(AU.bf16_bits(dev.v0))
    r64 = AU.adam_step_from(dev.p0.double(), g.double(), m0, v0, 1, LR, dev.wd)
    r32 = AU.adam_step_from(dev.p0.float(), g.float(), m0.float(), v0.float(), 1, LR, dev.wd.float())
    return r64, r32


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("size", ["small", "large"])
def test_one_step_from_bf16_moments(size, fmt):
    g = _data(size)["g"][0]
    dev = Dev(DT[fmt], size)
    dev.step(g)
    (p64, m64, v64), (p32, m32, v32) = _one_step_refs(dev, g)
    live = dev.mask
    r = TU.check_limit(dev.p.cpu()[live], p32[live], p64[live], f"{size} {fmt} p")
    print(f"{size} {fmt}: p error / limit (norm, worst element) {r[0]:.3f} {r[1]:.3f}")
    # the stored moments: within one bf16 ulp (+ the f32 allowance) of the fp64 moments
    for name, t, r64, r32 in (("m16", dev.m, m64, m32), ("v16", dev.v, v64, v32)):
        h = AU.bf16_bits(t)[live]
        assert bool(((h & 0x7F80) != 0x7F80).all()), f"{name}: non-finite values"
        err = (AU.decode16(h) - r64[live]).abs()
        ulp16 = TU.ulp32(r64[live]) * 65536.0
        assert bool((err <= ulp16 + AU.f32_allowance(r32[live], r64[live])).all()), f"{name}: more than one bf16 ulp from the fp64 moment"
    dev.check_canaries_and_arena()
    assert dev.state.cpu().tolist() == [1.0, TU.BETAS[0], TU.BETAS[1], 0.0]


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_bracketing_with_injected_words_and_the_counter_layout(fmt):
    g = _data("small")["g"][0]
    n = LAYOUTS["small"][1]
    words = dict(zero=torch.zeros(n, dtype=torch.int32), ones=torch.full((n,), -1, dtype=torch.int32), philox=AU.philox_words(SEED, 1, n), none=None)
    runs = {}
    for k, w in words.items():
        dev = Dev(DT[fmt])
        dev.step(g, sr_words=None if w is None else w.cuda())
        runs[k] = dev.bits()
        dev.check_canaries_and_arena()
    assert _same(runs["none"], runs["philox"]), "the kernel's own words are not philox4x32_10(seed, {G, t}) with word k for element 4G + k"
    for k in ("ones", "philox"):
        assert torch.equal(runs[k][0], runs["zero"][0]) and torch.equal(runs[k][3], runs["zero"][3]), "the rounding words reached p or the arena"
    (_, m64, v64), (_, m32, v32) = _one_step_refs(dev, g)
    live = dev.mask
    assert dict((b, w) for b, _, _, w in dev.segs)[448] == 0.0
    for name, i, r64, r32 in (("m16", 1, m64, m32), ("v16", 2, v64, v32)):
        lo, ph, hi = (runs[k][i].to(torch.int64)[live] & 0xFFFF for k in ("zero", "philox", "ones"))
        # one sign per element, so the bit patterns order like the magnitudes
        assert bool(((lo <= ph) & (ph <= hi)).all()), f"{name}: stored(philox) outside [stored(0), stored(0xFFFF)]"
        assert bool(((hi - lo) >= 0).all()) and bool(((hi - lo) <= 1).all()), f"{name}: the two images are more than one bf16 ulp apart"
        z = torch.zeros(n, dtype=torch.bool); z[512:576] = True
        assert bool((hi == lo)[z[live]].all()) and bool((hi != lo).any()), f"{name}: a representable value (0) must not move; others must"
        dlo, dhi, allow = AU.decode16(lo), AU.decode16(hi), AU.f32_allowance(r32[live], r64[live])
        x = r64[live]
        assert bool(((x >= torch.minimum(dlo, dhi) - allow) & (x <= torch.maximum(dlo, dhi) + allow)).all()), f"{name}: the fp64 moment is outside [lo, hi]"
        # where the two images differ the f32 value's low half is not zero: the word decides, up iff low + r carries.  So philox picks hi for a
        # share of the elements near the mean low half / 2^16 ~ 1/2
        differ = hi != lo
        share = (ph == hi)[differ].double().mean().item()
        print(f"{fmt} {name}: {int(differ.sum())} of {int(live.sum())} elements between two bf16 values, {share:.4f} of them stored up")
        assert 0.45 < share < 0.55


def _one_segment(n, m16, v16, g, beta1, beta2, launches=1, seed=SEED):
    """lr = 0, no decay, one segment, no arena: the stored moments after `launches` steps"""
    from enhancing import _C
    p = torch.zeros(n, device="cuda")
    m = torch.full((n,), m16, dtype=torch.bfloat16, device="cuda")
    v = torch.full((n,), v16, dtype=torch.bfloat16, device="cuda")
    gd = torch.full((n,), g, device="cuda")
    table = _C.adam_segment_table([(0, n, -1, 0.0)], n, 0, "cuda")
    state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).cuda()
    for _ in range(launches):
        _C.adam_step_segments_s16(p, gd, m, v, None, table, state, lr=0.0, beta1=beta1, beta2=beta2, eps=TU.EPS, seed=seed, dtype=torch.bfloat16)
    assert state[0].item() == launches and bool((p == 0).all())
    return AU.decode16(AU.bf16_bits(m)), AU.decode16(AU.bf16_bits(v))


def test_stored_rounding_is_unbiased_and_not_round_to_nearest():
    """2^20 elements whose exact new moment sits a known fraction of a bf16 ulp above a grid point.  The mean of (stored - exact) / ulp over the
    elements must be within 3e-3 of 0: the per-element variance is <= 1/4 ulp^2, so the mean's sigma is <= 0.5 / 1024 = 4.9e-4 and the limit is 6
    sigma.  Round-to-nearest and truncation give -0.25 for the 1/4-ulp offset (rounding up +0.75); round-to-nearest gives +0.25 for the 3/4-ulp one."""
    n = 1 << 20
    # m: m16 = 1 (ulp 2^-7 in [1, 2)), beta1 = 0.5, g = 1 + 2^-8: m + (g - m) (1 - beta1) = 1 + 2^-9 = 1 + ulp / 4, every operation exact in f32
    b1, g, ulp = 0.5, 1.0 + 2.0 ** -8, 2.0 ** -7
    assert float(torch.tensor(g, dtype=torch.float32)) == g and float(torch.tensor(1.0 - b1, dtype=torch.float32)) == 0.5
    exact_m = 1.0 + (g - 1.0) * (1.0 - b1)
    assert exact_m == 1.0 + ulp / 4 and float(torch.tensor(exact_m, dtype=torch.float32)) == exact_m
    m, _ = _one_segment(n, 1.0, 0.0, g, b1, 0.96)
    assert set(m.unique().tolist()) == {1.0, 1.0 + ulp}, "a stored value is neither neighbour of the exact one"
    mean_m = ((m - exact_m) / ulp).mean().item()
    # v: v16 = 1, g = 0, beta2 = 1 - 2^-10: v beta2 + g g (1 - beta2) = 1 - 2^-10 = (1 - 2^-8) + 3/4 ulp with ulp = 2^-8 in [0.5, 1); exact in f32
    b2, ulp_v = 1.0 - 2.0 ** -10, 2.0 ** -8
    assert float(torch.tensor(b2, dtype=torch.float32)) == b2 and float(torch.tensor(1.0 - b2, dtype=torch.float32)) == 2.0 ** -10
    exact_v = 1.0 * b2 + 0.0 * (1.0 - b2)
    assert exact_v == (1.0 - ulp_v) + 0.75 * ulp_v
    _, v = _one_segment(n, 0.0, 1.0, 0.0, 0.9, b2)
    assert set(v.unique().tolist()) == {1.0 - ulp_v, 1.0}
    mean_v = ((v - exact_v) / ulp_v).mean().item()
    print(f"mean (stored - exact) / ulp over 2^20 elements: m (1/4-ulp offset) {mean_m:+.2e}, v (3/4-ulp offset) {mean_v:+.2e}; limit 3e-3")
    assert abs(mean_m) <= 3e-3 and abs(mean_v) <= 3e-3


def test_v_does_not_stall_where_round_to_nearest_would():
    """g = 1, v16 = 0.5, beta2 = 0.999: the first increment is 5e-4 against a half-ulp of 1.95e-3 in [0.5, 1), so round-to-nearest stays at 0.5 for
    ever.  After 200 launches the exact v is 1 - 0.5 x 0.999^200 = 0.5907; the mean of the stored v over 65536 elements must be within 5e-3 of it (the
    accumulated rounding noise of the mean is ~1e-4)."""
    launches, b2 = 200, 0.999
    exact = 1.0 - 0.5 * b2 ** launches
    assert abs(exact - 0.5907) < 1e-4
    _, v = _one_segment(65536, 0.0, 0.5, 1.0, 0.9, b2, launches=launches)
    print(f"stored v after {launches} launches: mean {v.mean().item():.5f} (exact {exact:.5f}), min {v.min().item():.4f}, max {v.max().item():.4f}")
    assert abs(v.mean().item() - exact) <= 5e-3


def test_drift_over_eight_steps_stays_inside_the_derived_bound():
    """8 steps (the four gradients twice) from zero moments against torch.optim.Adam in fp64.  A stored rounding error is under one bf16 ulp
    (<= 2^-7 of the value) and decays by beta per step, so elementwise |m16_t - m64_t| <= 2^-7 max_k |m64_k| / (1 - beta1) + the f32 allowance, and
    the same for v with beta2.  Derived, not measured; the worst ratio is printed."""
    D = _data("small")
    segs = LAYOUTS["small"][0]
    split = lambda flat: [flat[b:e] for b, e, _, _ in segs]
    cat = lambda parts: torch.cat([t.reshape(-1) for t in parts]).double()
    refs = {dt: TU.TorchAdam(split(D["p"]), [w for _, _, _, w in segs], LR, dt) for dt in (torch.float64, torch.float32)}
    dev = Dev(torch.bfloat16, moments=False)
    max_m = max_v = None
    for t in range(8):
        g = D["g"][t % 4]
        dev.step(g)
        for r in refs.values():
            r.step(split(g))
        m64, v64 = cat(refs[torch.float64].m()), cat(refs[torch.float64].v())
        max_m = m64.abs() if max_m is None else torch.maximum(max_m, m64.abs())
        max_v = v64 if max_v is None else torch.maximum(max_v, v64)
    m32, v32 = cat(refs[torch.float32].m()), cat(refs[torch.float32].v())
    live = dev.mask
    worst = []
    for name, t, r64, r32, mx, beta in (("m", dev.m, m64, m32, max_m, TU.BETAS[0]), ("v", dev.v, v64, v32, max_v, TU.BETAS[1])):
        err = (AU.decode16(AU.bf16_bits(t))[live] - r64).abs()
        bound = 2.0 ** -7 * mx / (1.0 - beta) + AU.f32_allowance(r32, r64)
        worst.append((err / bound).max().item())
        assert bool((err <= bound).all()), f"{name}16 after 8 steps: {worst[-1]:.3f} x the bound"
    print(f"8 steps: worst |x16 - x64| / bound  m {worst[0]:.3f}  v {worst[1]:.3f}")
    dev.check_canaries_and_arena()
    assert dev.state[0].item() == 8.0


def test_a_dropped_step_writes_nothing_and_consumes_no_randomness():
    D = _data("small")
    flag = torch.zeros(1, device="cuda")
    a = Dev(torch.float16)
    a.step(D["g"][0], skip_flag=flag)
    before = a.bits()
    bad = D["g"][3].clone()
    bad[5000] = float("inf")
    flag.fill_(1.0)
    a.step(bad, skip_flag=flag)
    assert _same(before, a.bits()), "a dropped step wrote something (p, m16, v16, the arena or the step state)"
    flag.zero_()
    a.step(D["g"][1], skip_flag=flag)
    b = Dev(torch.float16)              # the same two steps with no drop between them
    b.step(D["g"][0])
    b.step(D["g"][1])
    assert _same(a.bits(), b.bits()), "the step after a dropped one differs from a step with no drop before it"
    assert a.state[0].item() == 2.0
    a.check_canaries_and_arena()


def test_seeds_and_repeatability():
    D = _data("small")
    runs = []
    for seed in (SEED, SEED, SEED + 1):
        dev = Dev(torch.bfloat16)
        dev.step(D["g"][0], seed=seed)
        first = dev.bits()
        dev.step(D["g"][1], seed=seed)
        runs.append((first, dev.bits()))
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "the same seed gave different bits"
    assert not torch.equal(runs[0][0][1], runs[2][0][1]) and not torch.equal(runs[0][0][2], runs[2][0][2]), "another seed stored the same moments"
    assert torch.equal(runs[0][0][0], runs[2][0][0]) and torch.equal(runs[0][0][3], runs[2][0][3]), "p of a step saw that step's own rounding"
    assert not torch.equal(runs[0][1][0], runs[2][1][0]), "the second step must read the stored moments"


def test_a_nan_gradient_without_skip_lands_in_both_moments_only_there():
    D = _data("small")
    clean = Dev(torch.bfloat16)
    clean.step(D["g"][0])
    g = D["g"][0].clone()
    at = [5000, 270400 + 77]
    g[at] = float("nan")
    dev = Dev(torch.bfloat16)
    dev.step(g)
    other = torch.ones(dev.n, dtype=torch.bool); other[at] = False
    for name, i in (("m16", 1), ("v16", 2)):
        got, want = dev.bits()[i], clean.bits()[i]
        assert bool(torch.isnan(got.view(torch.bfloat16)[at].float()).all()), f"{name} is not nan where g is"
        assert torch.equal(got[other], want[other]), f"{name} changed away from the nan"
