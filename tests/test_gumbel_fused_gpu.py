"""GumbelQuantizer(fused=True): the fused gfx950 Gumbel-softmax quantizer (csrc/gumbel.hip) against this repository's torch GumbelQuantizer (pinned
to the reference by tests/golden/gumbel.npz) with F.gumbel_softmax patched to consume the kernel's own dumped noise ``fused_noise(call, M)``.  The
torch module is evaluated on the CPU in fp64 (the truth) and in fp32 (the yardstick's own error).

Margins (every measured ratio is printed):
  util.rel(ours, truth)      <= max(4 x util.rel(fp32 torch, truth), 1e-5)   1e-5 = the project's F32_TOL; 4 x covers the hardware exp2 / log2, another
                                                                            summation order over K, and the online rescale
  worst util.row_err(ours)   <= 8 x worst util.row_err(fp32 torch)           single rows do not average
  idx = fp64 argmax of l + g; a token may differ only where the fp64 gap between the two candidates is below (6 d + 12) 2^-24 max(1, |zn|^2) (the
  project's near-tie bound), and at most 0.1 % of the tokens may use that exemption.

Measured on an MI355X over the 16 cases, soft and hard (worst case of each; idx: 0 mismatches in every case):
  z_q  rel <= 3.3e-6 (all below the 1e-5 floor; at most 4.0 x fp32 torch)        worst row 4.6 x fp32 torch's (M=4096 K=1024 d=16 tau=1 norm)
  loss rel <= 5.5e-6 (all below the floor; fp32 torch is at 4e-7 there, ratio up to 16: the floor decides, not the 4 x)
  dz   rel <= 1.9e-5, 1.12 x fp32 torch wherever it is above the floor           worst row 6.6 x (M=257 K=8192 d=32 tau=1 norm: 1.5e-5 against 2.3e-6)
  dE   rel <= 1.9e-5, 1.08 x fp32 torch wherever it is above the floor           worst row 5.3 x (M=257 K=8192 d=32 tau=1 norm, hard: 6.2e-6 against 1.2e-6)
The rows nearest the 8 x margin are the K = 8192, tau = 1 gradients, where y is spread over thousands of codes and a token's dz is a small residue of
cancelling terms; the kernel takes delta = g_zq . z_q from the STORED f32 z_q (torch's softmax backward sums y dy directly), which is the candidate term,
not isolated by a measurement."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import rel, row_err

pytestmark = pytest.mark.gpu

SEED = 20240607
SHAPES = [(1000, 500, 32), (257, 8192, 32), (4096, 1024, 16), (1, 128, 8)]
CASES = [(M, K, d, tau, un) for (M, K, d) in SHAPES for tau in (1.0, 0.1) for un in (True, False)]


def _patched(queue):
    """F.gumbel_softmax with its draw replaced by the next tensor of `queue` (torch/nn/functional.py: gumbels = (logits + gumbels) / tau; softmax;
    hard: y_hard - y.detach() + y)"""
    def f(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        g = queue.pop(0).to(logits.dtype).view_as(logits)
        y = ((logits + g) / tau).softmax(dim)
        if hard:
            one = torch.zeros_like(y).scatter_(dim, y.argmax(dim, keepdim=True), 1.0)
            y = one - y.detach() + y
        return y
    return f


def _torch_quantizer(E, noises, z, g_zq, dtype, train, monkeypatch, tau, **kw):
    """the torch GumbelQuantizer (fused=False) on the CPU in `dtype`, fed `noises`, forward + backward with grad_out (g_zq, 1)"""
    from enhancing.modules.stage1.quantizers import GumbelQuantizer
    K, d = E.shape
    q = GumbelQuantizer(d, K, temp_init=tau, **kw).to(dtype)
    q.embedding.weight.data.copy_(E.to(dtype))
    q.train(train)
    zt = z.to(dtype).clone().requires_grad_(True)
    monkeypatch.setattr(F, "gumbel_softmax", _patched([n.cpu() for n in noises]))
    zq, loss, idx = q(zt)
    (zq * g_zq.to(dtype)).sum().add(loss).backward()
    monkeypatch.undo()
    return dict(zq=zq.detach(), loss=loss.detach(), idx=idx, dz=zt.grad, dE=q.embedding.weight.grad)


def _fused(E, z, g_zq, train, tau, seed=SEED, **kw):
    from enhancing.modules.stage1.quantizers import GumbelQuantizer
    K, d = E.shape
    q = GumbelQuantizer(d, K, temp_init=tau, fused=True, seed=seed, **kw).cuda()
    q.embedding.weight.data.copy_(E)
    q.train(train)
    zt = z.cuda().requires_grad_(True)
    call = q.noise_call
    zq, loss, idx = q(zt)
    (zq * g_zq.cuda()).sum().add(loss).backward()
    torch.cuda.synchronize()
    depth = q.noise_call - call
    M = z.reshape(-1, d).shape[0]
    noises = [q.fused_noise(call + i, M) for i in range(depth)]
    return q, dict(zq=zq.detach(), loss=loss.detach(), idx=idx, dz=zt.grad, dE=q.embedding.weight.grad), noises


class _MP:
    """monkeypatch stand-in for the cached reference (a pytest fixture cannot be held by a cache)"""

    def __init__(self):
        self.saved = None

    def setattr(self, obj, name, val):
        self.saved = (obj, name, getattr(obj, name))
        setattr(obj, name, val)

    def undo(self):
        obj, name, val = self.saved
        setattr(obj, name, val)


@functools.lru_cache(maxsize=None)
def _case(M, K, d, tau, use_norm):
    """inputs, the fused results and the two torch evaluations of one case, soft (train) and hard (eval), computed once"""
    import vitvq_oracle as O
    z, E, g = O.make_vq_inputs(41 + M % 7 + K % 5, M, K, d)
    out = dict(z=z, E=E, g=g)
    for mode, train in (("soft", True), ("hard", False)):
        _, ours, noises = _fused(E, z, g, train, tau, use_norm=use_norm)
        out[mode] = dict(ours=ours, noise=noises[0].cpu(),
                         t64=_torch_quantizer(E, noises, z, g, torch.float64, train, _MP(), tau, use_norm=use_norm),
                         t32=_torch_quantizer(E, noises, z, g, torch.float32, train, _MP(), tau, use_norm=use_norm))
    return out


def _check_idx(idx, z, E, noise, use_norm, what):
    """idx against the fp64 argmax of l + g, with the near-tie exemption.  Returns the number of exempted tokens."""
    d = z.shape[-1]
    zn = F.normalize(z.double(), dim=-1) if use_norm else z.double()
    en = F.normalize(E.double(), dim=-1) if use_norm else E.double()
    s = 2.0 * zn @ en.t() - zn.pow(2).sum(1, keepdim=True) - en.pow(2).sum(1) + noise.double()
    ref = s.argmax(-1)
    idx = idx.cpu().reshape(-1)
    assert idx.dtype == torch.int64 and idx.shape == ref.shape, (what, idx.dtype, idx.shape)
    bad = (idx != ref).nonzero().reshape(-1)
    gap = s[bad, ref[bad]] - s[bad, idx[bad]]
    lim = (6 * d + 12) * 2.0 ** -24 * zn.pow(2).sum(1)[bad].clamp_min(1.0)
    print(f"{what}: idx mismatches {bad.numel()} of {idx.numel()}; smallest fp64 top-2 gap {float((s.topk(2, -1).values @ torch.tensor([1.0, -1.0], dtype=torch.float64)).min()):.2e}")
    assert bool((gap < lim).all()), (what, "idx differs beyond the near-tie bound", gap.max().item())
    assert bad.numel() <= 1e-3 * idx.numel(), (what, bad.numel())
    return bad.numel()


def _check_margin(what, ours, t32, t64, width=None):
    """rel <= max(4 x fp32 torch, 1e-5); worst row <= 8 x fp32 torch's worst row"""
    assert bool(torch.isfinite(ours).all()), what
    e, e32 = rel(ours, t64), rel(t32, t64)
    msg = f"{what}: rel {e:.2e} (fp32 torch {e32:.2e}, ratio {e / max(e32, 1e-300):.2f})"
    ok = e <= max(4 * e32, 1e-5)
    if width is not None:
        r, r32 = row_err(ours, t64, width).max().item(), row_err(t32, t64, width).max().item()
        msg += f"; worst row {r:.2e} (fp32 torch {r32:.2e}, ratio {r / max(r32, 1e-300):.2f})"
        ok = ok and r <= 8 * r32
    print(msg)
    return ok, msg


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. noise
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_noise_is_a_function_of_seed_call_token_code():
    from enhancing import _C
    dev = torch.device("cuda")
    a = _C.gumbel_noise(SEED, 3, 1000, 8192, dev)
    assert bool(torch.isfinite(a).all())
    b = _C.gumbel_noise(SEED, 3, 2000, 8192, dev)
    assert torch.equal(a, b[:1000])                                           # not a function of M
    assert torch.equal(a[:, :500], _C.gumbel_noise(SEED, 3, 1000, 500, dev))   # ... nor of K (a ragged last group of four included)
    assert torch.equal(a[:, :1], _C.gumbel_noise(SEED, 3, 1000, 1, dev))
    assert torch.equal(a, _C.gumbel_noise(SEED, 3, 1000, 8192, dev))
    assert not torch.equal(a, _C.gumbel_noise(SEED, 4, 1000, 8192, dev)) and not torch.equal(a, _C.gumbel_noise(SEED + 1, 3, 1000, 8192, dev))
    assert not torch.equal(a, _C.gumbel_noise(SEED + (1 << 32), 3, 1000, 8192, dev))      # the seed's high word is part of the key
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[:, 0], a[:, 4])
    # Gumbel(0, 1): mean gamma, variance pi^2 / 6, P(g <= 0) = 1 / e; limits at 5 standard errors for n = 1000 x 8192
    x = a.double().cpu().reshape(-1)
    mean, var, p0 = x.mean().item(), x.var().item(), (x <= 0).double().mean().item()
    print(f"noise: n {x.numel()} mean {mean:.5f} var {var:.5f} (pi^2/6 {math.pi ** 2 / 6:.5f}) P(g<=0) {p0:.5f} (1/e {math.exp(-1):.5f}) min {x.min():.3f} max {x.max():.3f}")
    assert abs(mean - 0.57722) <= 2.2e-3
    assert abs(var - math.pi ** 2 / 6) <= 6e-3
    assert abs(p0 - math.exp(-1)) <= 8.4e-4


def test_module_dump_is_the_kernels_noise():
    from enhancing import _C
    from enhancing.modules.stage1.quantizers import GumbelQuantizer
    q = GumbelQuantizer(32, 500, fused=True, seed=SEED).cuda()
    assert torch.equal(q.fused_noise(2, 300), _C.gumbel_noise(SEED, 2, 300, 500, torch.device("cuda")))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. forward   3. backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,d,tau,use_norm", CASES)
def test_forward(M, K, d, tau, use_norm):
    c = _case(M, K, d, tau, use_norm)
    what = f"fwd M={M} K={K} d={d} tau={tau} norm={use_norm}"
    fails = []
    for mode in ("soft", "hard"):
        r = c[mode]
        _check_idx(r["ours"]["idx"], c["z"], c["E"], r["noise"], use_norm, f"{what} {mode}")
        assert r["ours"]["zq"].shape == (M, d) and r["ours"]["loss"].shape == ()
        for name, width in (("zq", d), ("loss", None)):
            ok, msg = _check_margin(f"{what} {mode} {name}", r["ours"][name].cpu(), r["t32"][name], r["t64"][name], width)
            if not ok:
                fails.append(msg)
    en = F.normalize(c["E"], dim=-1) if use_norm else c["E"]
    hard = c["hard"]["ours"]
    worst = (hard["zq"].cpu() - en[hard["idx"].cpu()]).abs().max().item()
    print(f"{what}: hard |z_q - n(E)[idx]| max {worst:.2e}")
    assert worst <= 1e-6
    assert not fails, fails


@pytest.mark.parametrize("M,K,d,tau,use_norm", CASES)
def test_backward(M, K, d, tau, use_norm):
    c = _case(M, K, d, tau, use_norm)
    what = f"bwd M={M} K={K} d={d} tau={tau} norm={use_norm}"
    fails = []
    for mode in ("soft", "hard"):
        r = c[mode]
        assert r["ours"]["dz"].shape == (M, d) and r["ours"]["dE"].shape == (K, d)
        for name in ("dz", "dE"):
            ok, msg = _check_margin(f"{what} {mode} {name}", r["ours"][name].cpu(), r["t32"][name], r["t64"][name], d)
            if not ok:
                fails.append(msg)
    assert not fails, fails


@pytest.mark.parametrize("M,K,d", [(1000, 500, 32), (4096, 1024, 16)])
@pytest.mark.parametrize("hard", [False, True])
def test_backward_accumulates_and_repeats_bit_for_bit(M, K, d, hard):
    import vitvq_oracle as O
    from enhancing import _C
    z, E, g = (t.cuda() for t in O.make_vq_inputs(5, M, K, d))
    gl = torch.ones(1, device="cuda")
    runs = []
    for _ in range(2):
        zq, zq_soft, idx, loss, stats = _C.gumbel_forward(z, E, 0.7, hard, True, SEED, 9)
        dE = torch.zeros_like(E)
        dz = _C.gumbel_backward(z, E, zq_soft, stats, g, 1.0, gl, 0.7, hard, idx, True, SEED, 9, dE)
        runs.append((zq, zq_soft, idx, loss, stats, dz, dE))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    zq, zq_soft, idx, loss, stats, dz, dE = runs[0]
    assert (zq_soft is zq) != hard
    base = torch.from_numpy(np.random.RandomState(3).standard_normal((K, d)).astype(np.float32)).cuda()
    acc = base.clone()
    _C.gumbel_backward(z, E, zq_soft, stats, g, 1.0, gl, 0.7, hard, idx, True, SEED, 9, acc)
    assert float(dE.abs().max()) > 0 and torch.equal(acc, base + dE)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. module
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_residual_module_against_the_torch_module(monkeypatch):
    import vitvq_oracle as O
    z, E, g = O.make_vq_inputs(17, 2 * 150, 1024, 32)
    z, g = z.view(2, 150, 32), g.view(2, 150, 32)
    kw = dict(use_residual=True, num_quantizers=2)
    q, ours, noises = _fused(E, z, g, True, 1.0, **kw)
    assert len(noises) == 2 and q.noise_call == 2 and not torch.equal(noises[0], noises[1])      # one call index per level per forward
    t64 = _torch_quantizer(E, noises, z, g, torch.float64, True, monkeypatch, 1.0, **kw)
    t32 = _torch_quantizer(E, noises, z, g, torch.float32, True, monkeypatch, 1.0, **kw)
    assert ours["zq"].shape == (2, 150, 32) and ours["idx"].shape == t64["idx"].shape == (2, 150, 2) and ours["idx"].dtype == torch.int64
    assert ours["loss"].shape == ()
    assert ours["dz"] is None and t64["dz"] is None          # the residual loop starts from z.detach() (quantizers.py:43)
    mism = int((ours["idx"].cpu() != t64["idx"]).sum())
    print(f"residual module: idx mismatches {mism} of {ours['idx'].numel()}")
    assert mism <= 1e-3 * ours["idx"].numel()
    fails = []
    for name, width in (("zq", 32), ("loss", None), ("dE", 32)):
        ok, msg = _check_margin(f"residual module {name}", ours[name].cpu(), t32[name], t64[name], width)
        if not ok:
            fails.append(msg)
    assert not fails, fails
    # not residual: z receives a gradient
    _, plain, _ = _fused(E, z, g, True, 1.0)
    assert plain["dz"] is not None and plain["dz"].shape == z.shape and float(plain["dz"].abs().max()) > 0
    assert plain["idx"].shape == (2, 150)
    # lookup = n(E[code]) summed over the levels (vitvqgan.py:82-87)
    en = F.normalize(E, dim=-1)
    assert (q.lookup(ours["idx"]).cpu() - en[ours["idx"].cpu()].sum(-2)).abs().max().item() <= 2e-6


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. memory
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_no_m_by_k_tensor_is_allocated():
    from enhancing.modules.stage1.quantizers import GumbelQuantizer
    M, K = 16384, 8192
    q = GumbelQuantizer(32, K, fused=True, seed=SEED).cuda()
    z = torch.randn(M, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(1)).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    zq, loss, idx = q(z)
    (zq.sum() + loss).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"fused Gumbel forward + backward at M={M} K={K}: max_memory_allocated rose by {rise / 2 ** 20:.1f} MiB (one [M,K] fp32 matrix: {M * K * 4 / 2 ** 20:.0f} MiB)")
    assert rise < M * K * 4
    assert bool(torch.isfinite(z.grad).all()) and bool(torch.isfinite(q.embedding.weight.grad).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. model
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_vitvq_gumbel_fused_training_step_vs_oracle(monkeypatch):
    """tests/test_gumbel_gpu.py's training step with `fused: True`: the oracle towers with the patched torch quantizer on the dumped noise in between"""
    import vitvq_oracle as O
    from enhancing.modules.stage1.quantizers import GumbelQuantizer
    from enhancing.modules.stage1.vitvqgan import ViTVQGumbel
    from enhancing.utils.general import AttrDict
    cfg = O.TINY_CFG
    P = O.make_params(cfg, seed=11)
    x = O.make_images(5, 2, cfg["image_size"])
    loss = {"target": "enhancing.losses.vqperceptual.VQLPIPS",
            "params": dict(codebook_weight=0.5, loglaplace_weight=0.0, loggaussian_weight=1.0, perceptual_weight=0.0)}
    qcfg = dict(embed_dim=32, n_embed=512, temp_init=0.9)
    tsched = {"target": "enhancing.utils.scheduler.ExponentialDecayScheduler", "params": dict(start=0.9, end=0.1, decay_every_step=1, scale_factor=1e-3)}
    m = ViTVQGumbel("image", cfg["image_size"], cfg["patch_size"], AttrDict.wrap(cfg["encoder"]), AttrDict.wrap(cfg["decoder"]),
                    AttrDict.wrap(dict(qcfg, fused=True, seed=77)), AttrDict.wrap(loss), temperature_scheduler=AttrDict.wrap(tsched))
    assert isinstance(m.quantizer, GumbelQuantizer) and m.quantizer.fused
    m.load_state_dict(P, strict=True)
    m.train()
    call = m.quantizer.noise_call
    out = m.training_step({"image": x}, 0, 0)
    torch.cuda.synchronize()
    assert m.quantizer.noise_call == call + 1
    assert abs(m.logged["temperature"] - 0.9) < 1e-6
    noise = m.quantizer.fused_noise(call, 2 * 64).cpu()
    leaves = {k: v.detach().clone().requires_grad_(not k.endswith("pos_embedding")) for k, v in P.items()}
    q = GumbelQuantizer(**qcfg)
    q.temperature = 0.9
    q.train()
    q.embedding.weight = torch.nn.Parameter(leaves["quantizer.embedding.weight"])
    h = O.encoder(x, leaves, cfg) @ leaves["pre_quant.weight"].t() + leaves["pre_quant.bias"]
    monkeypatch.setattr(F, "gumbel_softmax", _patched([noise]))
    quant, qloss, idx = q(h)
    monkeypatch.undo()
    xrec = O.decoder(quant @ leaves["post_quant.weight"].t() + leaves["post_quant.bias"], leaves, cfg)
    o_loss = (xrec - x).pow(2).mean() + 0.5 * qloss
    o_loss.backward()
    grads = {k: (q.embedding.weight.grad if k == "quantizer.embedding.weight" else v.grad) for k, v in leaves.items()}
    grads = {k: g for k, g in grads.items() if g is not None}
    assert abs(float(out) - float(o_loss)) <= 1e-2 * abs(float(o_loss)), (float(out), float(o_loss))
    m.engine.unscale_grads()
    errs = {k: rel(p.grad, grads[k]) for k, p in m.named_parameters() if k in grads}
    worst = max(errs, key=errs.get)
    print(f"ViTVQGumbel fused train step: loss {float(out):.5f} vs oracle {float(o_loss):.5f}; grads median rel {np.median(list(errs.values())):.2e}, worst {worst} {errs[worst]:.2e}")
    assert set(errs) == set(grads) and errs[worst] <= 3e-2, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    # inference API: eval mode quantises hard, the codes are the noisy argmax
    m.eval()
    call = m.quantizer.noise_call
    hq = m.pre_quant_tokens(x, "bf16")
    codes = m.encode_codes(x, precision="bf16")
    assert codes.shape == (2, 64) and codes.dtype == torch.int64 and m.quantizer.noise_call == call + 1
    _check_idx(codes, hq.reshape(-1, 32).cpu(), m.quantizer.embedding.weight.detach().cpu(), m.quantizer.fused_noise(call, 128).cpu(), True, "encode_codes")
    rec = m.decode_codes(codes)
    assert rec.shape == x.shape and bool(torch.isfinite(rec).all())
