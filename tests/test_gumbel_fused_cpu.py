"""GumbelQuantizer(fused=True), the parts that need no GPU: the switch's default, the widths it accepts, the error on host tensors, and that the
switch changes neither the module's parameters nor what its construction draws from torch's generator (init parity with the reference, which
tests/test_host_cpu.py pins for the torch path)."""
import pytest
import torch

from enhancing.modules.stage1.quantizers import GumbelQuantizer


def test_fused_defaults_to_false():
    q = GumbelQuantizer(32, 64)
    assert q.fused is False
    assert GumbelQuantizer(32, 64, fused=True).fused is True


@pytest.mark.parametrize("embed_dim", [40, 64])
def test_fused_refuses_wide_codes(embed_dim):
    with pytest.raises(ValueError, match="embed_dim"):
        GumbelQuantizer(embed_dim, 64, fused=True)
    GumbelQuantizer(embed_dim, 64)      # the torch path takes any width


def test_fused_on_a_host_tensor_raises():
    q = GumbelQuantizer(32, 64, fused=True, seed=1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        q(torch.zeros(2, 5, 32))
    with pytest.raises(RuntimeError, match="ROCm device"):
        q.quantize(torch.zeros(7, 32))
    assert q.noise_call == 0      # a refused call consumes no noise index


def test_state_dict_is_the_references():
    for kw in (dict(), dict(use_residual=True, num_quantizers=3)):
        assert list(GumbelQuantizer(32, 64, fused=True, **kw).state_dict()) == ["embedding.weight"]
        assert list(GumbelQuantizer(32, 64, fused=True, seed=5, **kw).state_dict()) == list(GumbelQuantizer(32, 64, **kw).state_dict())


def test_construction_draws_what_the_unfused_constructor_draws():
    states, weights = [], []
    for kw in (dict(), dict(fused=True), dict(fused=True, seed=9)):
        torch.manual_seed(123)
        q = GumbelQuantizer(32, 64, **kw)
        states.append(torch.get_rng_state())
        weights.append(q.embedding.weight.detach().clone())
    assert torch.equal(states[0], states[1]) and torch.equal(states[0], states[2])
    assert torch.equal(weights[0], weights[1]) and torch.equal(weights[0], weights[2])
    # seed=None takes its key from torch.initial_seed() without drawing
    torch.manual_seed(123)
    q = GumbelQuantizer(32, 64, fused=True)
    before = torch.get_rng_state()
    assert q.noise_seed() == 123 and torch.equal(before, torch.get_rng_state())
    assert GumbelQuantizer(32, 64, fused=True, seed=9).noise_seed() == 9
