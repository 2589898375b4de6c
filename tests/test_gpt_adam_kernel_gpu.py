"""enh_adam_step_segments (csrc/gpt_adam.hip) alone, against torch.optim.Adam on the CPU in fp64 with two parameter groups fed the same f32 gradients.
The limit is tests/gpt_train_util.py's: 4 x the error of torch.optim.Adam in f32 on the CPU against that fp64 run, plus one f32 ulp of the value, per
tensor (p, m, v) and for the worst element.

The segment table (_layout): sizes 64, 128, 192, 1088, 6144 and 262208 with the decay alternating 0.01 / 0.  A thread handles 4 consecutive elements (a
lane pair 8), a wave 256 in each of its four accesses to a tile, a workgroup's tile 4096: the bounds 64 and 192 fall inside one wave access, 384, 448
and 1536 inside the first tile, 8192 on a tile edge, 270400 = 66 x 4096 + 64 inside a wave access again; padding (canaries) sits at 384, 7680 and
behind the last segment.  Forty more 262208-element segments bring the buffer to 2632 tiles: more than the 2048 workgroups of a 256-CU grid, so a
workgroup takes a second tile 8.4 M elements on and moves its segment cursor over the segments between.  Three consecutive
6144-element sources (key, query, value in registration order) land as q | k | v in the arena; every second other segment has no destination; the
arena's first 64 elements, a gap in its middle and its tail are no destination (canaries)."""
import pytest
import torch

import gpt_train_util as TU

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
LR = 1e-3
CANARY = 12345.0


def _layout():
    """(segments [(begin, end, dst16, wd)], n, arena_n)"""
    sizes = [64, 128, 192, "gap64", 1088, 6144, "gap512", 262208, 6144, 6144, 6144, 1088, "gap64", 64] + [262208] * 40
    segs, at, k = [], 0, 0
    for s in sizes:
        if isinstance(s, str):
            at += int(s[3:])
            continue
        segs.append([at, at + s, -1, TU.WD if k % 2 == 0 else 0.0])
        at += s
        k += 1
    n = at + 64
    assert segs[5][0] == 8192 and segs[3][0] == 448 and segs[4][0] == 1536 and segs[6][0] == 270400
    # destinations: the three 6144s (indices 6, 7, 8 = key, query, value) as q | k | v; of the rest every second one, placed in reverse order
    d = 64
    for i in (7, 6, 8):
        segs[i][2] = d
        d += 6144
    d += 128                                        # a gap no segment writes
    for i in [j for j in range(len(segs)) if j not in (6, 7, 8)][::-2]:
        segs[i][2] = d
        d += segs[i][1] - segs[i][0]
    return [tuple(s) for s in segs], n, d + 64


SEGS, N, ARENA_N = _layout()
_DATA = {}


def _data():
    """p0, m0 = v0 = 0 and four f32 gradients on the CPU, drawn once"""
    if not _DATA:
        g = torch.Generator().manual_seed(11)
        _DATA["p"] = (0.02 * torch.randn(N, generator=g)).float()
        # gradients span the range a GPT's do: most ~1e-3, a slice ~1e-8 (at eps), a slice exactly zero
        gs = []
        for _ in range(4):
            x = 1e-3 * torch.randn(N, generator=g)
            x[1536:3000] *= 1e-5
            x[3000:3500] = 0.0
            gs.append(x.float())
        _DATA["g"] = gs
    return _DATA


def _split(flat):
    return [flat[b:e] for b, e, _, _ in SEGS]


_REFS = {}


def _reference(key, grads, keep, **clip):
    """(fp64 run, f32 run) of torch.optim.Adam over the segments: {step index in `keep`: (p, m, v)} as flat tensors of the segments' elements"""
    if key not in _REFS:
        D = _data()
        out = []
        for dtype in (torch.float64, torch.float32):
            opt = TU.TorchAdam(_split(D["p"]), [w for _, _, _, w in SEGS], LR, dtype)
            snaps = {}
            for i, g in enumerate(grads):
                opt.step(_split(g), **clip)
                if i in keep:
                    snaps[i] = tuple(torch.cat([t.reshape(-1) for t in part()]).clone() for part in (opt.p, opt.m, opt.v))
            out.append(snaps)
        _REFS[key] = out
    return _REFS[key]


def _live(flat):
    """the elements inside segments, concatenated (what _reference returns)"""
    return torch.cat(_split(flat))


class Dev:
    """device buffers with canaries in the padding of p, m, v and in the arena's non-destination elements"""

    def __init__(self, dt):
        from enhancing import _C
        D = _data()
        self.dt = dt
        self.mask = torch.zeros(N, dtype=torch.bool)
        for b, e, _, _ in SEGS:
            self.mask[b:e] = True
        pad = ~self.mask
        p = D["p"].clone(); p[pad] = CANARY
        z = torch.zeros(N); z[pad] = CANARY
        self.p, self.m, self.v = p.cuda(), z.clone().cuda(), z.clone().cuda()
        self.arena = torch.full((ARENA_N,), 768.0, dtype=dt).cuda()
        self.amask = torch.zeros(ARENA_N, dtype=torch.bool)
        for b, e, d, _ in SEGS:
            if d >= 0:
                self.amask[d:d + e - b] = True
        self.table = _C.adam_segment_table(SEGS, N, ARENA_N, "cuda")
        self.state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64).cuda()

    def step(self, g, **kw):
        from enhancing import _C
        _C.adam_step_segments(self.p, g.cuda(), self.m, self.v, self.arena, self.table, self.state, lr=LR, beta1=TU.BETAS[0], beta2=TU.BETAS[1], eps=TU.EPS, **kw)

    def bits(self):
        return [t.clone().view(torch.int32 if t.dtype == torch.float32 else (torch.int64 if t.dtype == torch.float64 else torch.int16))
                for t in (self.p, self.m, self.v, self.arena, self.state)]

    def check_canaries_and_arena(self):
        pad = ~self.mask
        for name, t in (("p", self.p), ("m", self.m), ("v", self.v)):
            assert bool((t.cpu()[pad] == CANARY).all()), f"the padding of {name} was written"
        a = self.arena.cpu()
        assert bool((a[~self.amask].float() == 768.0).all()), "an arena element that is no destination was written"
        want = self.p.to(self.dt)       # the device's own rounding of the device's p
        for b, e, d, _ in SEGS:
            if d >= 0:
                assert torch.equal(self.arena[d:d + e - b].view(torch.int16), want[b:e].view(torch.int16)), f"arena image of segment [{b}, {e})"


def _check(dev, ref64, ref32, what):
    ratios = []
    for name, t, r64, r32 in zip("pmv", (dev.p, dev.m, dev.v), ref64, ref32):
        ratios.append(TU.check_limit(_live(t.cpu()), r32, r64, f"{what} {name}"))
    print(f"{what}: error / limit (norm, worst element) p {ratios[0][0]:.3f} {ratios[0][1]:.3f}  m {ratios[1][0]:.3f} {ratios[1][1]:.3f}  "
          f"v {ratios[2][0]:.3f} {ratios[2][1]:.3f}")


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_one_and_three_steps_against_fp64(fmt):
    D = _data()
    r64, r32 = _reference("plain", D["g"][:3], (0, 2))
    dev = Dev(DT[fmt])
    for t in range(3):
        dev.step(D["g"][t])
        if t in (0, 2):
            _check(dev, r64[t], r32[t], f"{fmt} step {t + 1}")
            dev.check_canaries_and_arena()
    assert dev.state.cpu().tolist() == [3.0, 0.9 * 0.9 * 0.9, 0.96 * 0.96 * 0.96, 0.0]


def test_a_skipped_step_writes_nothing_and_does_not_count():
    D = _data()
    r64, r32 = _reference("plain", D["g"][:3], (0, 2))
    dev = Dev(torch.float16)
    flag = torch.zeros(1, device="cuda")
    dev.step(D["g"][0], skip_flag=flag)
    before = dev.bits()
    bad = D["g"][3].clone()
    bad[5000] = float("inf")
    flag.fill_(1.0)
    dev.step(bad, skip_flag=flag)
    assert all(torch.equal(a, b) for a, b in zip(before, dev.bits())), "a dropped step wrote something (p, m, v, arena or the step count)"
    flag.zero_()
    dev.step(D["g"][1], skip_flag=flag)
    dev.step(D["g"][2], skip_flag=flag)
    assert dev.state[0].item() == 3.0
    _check(dev, r64[2], r32[2], "steps 1, 2 (dropped), 3, 4")
    dev.check_canaries_and_arena()


def test_loss_scale_is_exact_and_runs_repeat():
    D = _data()
    runs = []
    for S in (None, 65536.0, None):
        dev = Dev(torch.float16)
        for t in range(2):
            if S is None:
                dev.step(D["g"][t], grad_scale=0.5)
            else:
                dev.step(D["g"][t] * S, grad_scale=0.5, loss_scale=torch.full((1,), S, device="cuda"))
        runs.append(dev.bits())
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[2])), "two runs differ"
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "a power-of-two loss scale changed the bits"


@pytest.mark.parametrize("how", ["norm", "value"])
def test_clipping_against_torch_on_the_host(how):
    from enhancing import _C
    D = _data()
    grads = D["g"][:2]
    dev = Dev(torch.bfloat16)
    if how == "norm":
        max_norm = 0.5 * torch.cat(_split(grads[0])).double().norm().item()       # clips both steps by about half
        r64, r32 = _reference("norm", grads, (1,), clip_norm=max_norm)
        out = torch.zeros(2, device="cuda")
        for g in grads:
            gd = g.clone()
            gd[~dev.mask] = 0.0         # the norm pass reads the whole flat buffer: its padding is zero in GPT._flat_grads' layout
            _C.grad_clip_coef(gd.cuda(), max_norm, 1.0, out)
            assert 0.3 < out[1].item() < 0.7
            dev.step(gd, clip_coef=out[1:])
    else:
        r64, r32 = _reference("value", grads, (1,), clip_value=1e-3)      # one standard deviation: about a third of the elements are clamped
        for g in grads:
            dev.step(g, clip_value=1e-3)
    _check(dev, r64[1], r32[1], f"clip by {how}, 2 steps")
    dev.check_canaries_and_arena()


def test_indices_beyond_2_to_the_31():
    """2^31 + 1088 elements (p, g, m, v 8.6 GB each, the fp16 arena 4.3 GB): the first segment ends 6144 elements before 2^31, the second straddles 2^31
    and the third begins 64 elements behind it; all three have a destination, so element and byte offsets pass 2^31 / 2^32 in every buffer.  Windows
    of 4096 elements at the start, around 2^31 and at the end against the fp64 step; everything is made on the device."""
    from enhancing import _C
    T31 = 1 << 31
    n = T31 + 1088
    segs = [(0, T31 - 6144, 0, TU.WD), (T31 - 6144, T31 + 64, T31 - 6144, 0.0), (T31 + 64, n, T31 + 64, TU.WD)]
    torch.manual_seed(5)
    p = torch.empty(n, device="cuda").normal_(0.0, 0.02)
    g = torch.empty(n, device="cuda").normal_(0.0, 1e-3)
    m = torch.empty(n, device="cuda").normal_(0.0, 1e-3)
    v = torch.empty(n, device="cuda").uniform_(0.0, 1e-6)
    arena = torch.zeros(n, dtype=torch.float16, device="cuda")
    t0 = 5
    state = torch.tensor([float(t0), 0.9 ** t0, 0.96 ** t0, 0.0], dtype=torch.float64, device="cuda")
    wins = [(0, 4096), (T31 - 6144 - 2048, T31 - 6144 + 2048), (n - 4096, n)]      # the last one spans 2^31 (n - 4096 = 2^31 - 3008) and the end
    old = [[t[a:b].double().cpu() for t in (p, g, m, v)] for a, b in wins]
    table = _C.adam_segment_table(segs, n, n, "cuda")
    _C.adam_step_segments(p, g, m, v, arena, table, state, lr=LR, beta1=0.9, beta2=0.96, eps=TU.EPS)
    assert state[0].item() == t0 + 1
    for (a, b), (p0, g0, m0, v0) in zip(wins, old):
        idx = torch.arange(a, b)
        wd = torch.zeros(b - a, dtype=torch.float64)
        for sb, se, _, w in segs:
            wd[(idx >= sb) & (idx < se)] = w
        # the fp64 step and the same step in f32 with torch's operations (the reference's own error for the limit)
        p64, m64, v64 = p0.clone(), m0.clone(), v0.clone()
        TU.adam_step64(p64, g0, m64, v64, t0 + 1, LR, wd)
        p32, m32, v32 = p0.float(), m0.float(), v0.float()
        TU.adam_step64(p32, g0.float(), m32, v32, t0 + 1, LR, wd.float())
        for name, dev_t, r32, r64 in (("p", p, p32, p64), ("m", m, m32, m64), ("v", v, v32, v64)):
            TU.check_limit(dev_t[a:b], r32, r64, f"window [{a}, {b}) {name}")
        assert torch.equal(arena[a:b].view(torch.int16), p[a:b].half().view(torch.int16)), f"arena window [{a}, {b})"
