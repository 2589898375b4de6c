"""bf16 Adam moments, what needs no GPU and no library kernel: the stored-rounding rule of include/enh_hip.h (enh_adam_step_segments_s16) on constructed
bit patterns, the Philox4x32-10 restatement of tests/adam16_util.py against the published Random123 known-answer vectors, and GPTAdam's argument
handling as far as it runs without a device."""
import struct

import numpy as np
import pytest
import torch

import adam16_util as AU


def _u(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _round(u, r):
    return AU.stored_round(torch.tensor(u, dtype=torch.int64), r).tolist()


# f32 patterns: finite normals of both signs with zero and non-zero low halves
PATTERNS = [_u(1.0), _u(-1.0), _u(1.0) | 0x0001, _u(-1.0) | 0x8000, _u(3.1415927), _u(-2.7182817e-12), 0x3F80FFFF, 0xBF807FFF, 0x00800001, 0x7F000001]


def test_zero_word_truncates_and_full_word_rounds_up_unless_exact():
    assert _round(PATTERNS, 0) == [u >> 16 for u in PATTERNS]
    assert _round(PATTERNS, 0xFFFF) == [(u >> 16) + (1 if u & 0xFFFF else 0) for u in PATTERNS]


def test_a_representable_value_is_a_fixed_point_for_every_word():
    exact = [u & 0xFFFF0000 for u in PATTERNS] + [0x00000000, 0x80000000, 0x00010000, 0x7F7F0000, 0xFF7F0000]
    r = torch.arange(0x10000, dtype=torch.int64)
    for u in exact:
        assert bool((AU.stored_round(torch.full((0x10000,), u, dtype=torch.int64), r) == (u >> 16)).all()), hex(u)


def test_the_probability_of_rounding_up_is_the_low_half():
    """over all 2^16 words a value is rounded up exactly (low half) times: the rule is unbiased by construction"""
    r = torch.arange(0x10000, dtype=torch.int64)
    for u in (0x3F804000, 0xBF80C000, 0x3F800001, 0x0000FFFF):
        up = (AU.stored_round(torch.full((0x10000,), u, dtype=torch.int64), r) == (u >> 16) + 1).sum().item()
        assert up == (u & 0xFFFF), hex(u)


def test_the_largest_finite_value_never_becomes_inf():
    for top in (0x7F7F0000, 0xFF7F0000):
        for low in (0x0001, 0x8000, 0xFFFF):
            for r in (0, 1, 0x7FFF, 0xFFFF):
                assert _round([top | low], r) == [top >> 16]
    assert AU.decode16(torch.tensor([0x7F7F])).item() == float(torch.finfo(torch.bfloat16).max)


def test_nan_and_inf_are_preserved():
    for r in (0, 0x8000, 0xFFFF):
        assert _round([0x7F800000, 0xFF800000], r) == [0x7F80, 0xFF80]
        for nan in (0x7FC00000, 0xFFC00001, 0x7F800001, 0xFF80FFFF, 0x7FFFFFFF):      # the payload of the last three sits in the low half only
            h = _round([nan], r)[0]
            assert (h & 0x7F80) == 0x7F80 and (h & 0x007F) != 0 and (h & 0x8000) == (nan >> 16 & 0x8000), hex(nan)
            assert torch.isnan(AU.decode16(torch.tensor([h]))).all()


def test_subnormals_move_by_integer_steps():
    # f32 subnormals and bf16 subnormals: the rule is (u + r) >> 16 with no special case, up to and across the smallest normal
    for u in (0x00000001, 0x00008000, 0x0000FFFF, 0x00012345, 0x007FFFFF, 0x80000001, 0x807FFFFF):
        for r in (0, 1, 0x8000, 0xFFFF):
            assert _round([u], r) == [(u + r) >> 16], (hex(u), hex(r))
    assert _round([0x007FFFFF], 0xFFFF) == [0x0080]      # the largest subnormal rounds up into the smallest normal bf16
    assert _round([0x00000001], 0xFFFF) == [0x0001] and _round([0x00000001], 0xFFFE) == [0x0000]


# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, output)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = AU.philox4x32_10(key, np.array([ctr], dtype=np.uint32))[0].tolist()
        assert got == list(want), [hex(x) for x in got]
    both = AU.philox4x32_10(KAT[0][1], np.array([KAT[0][0], (1, 0, 0, 0)], dtype=np.uint32))      # vectorised over counters
    assert both[0].tolist() == list(KAT[0][2]) and both[1].tolist() != both[0].tolist()


def test_philox_words_layout():
    """element e takes word e % 4 of the call for group e / 4 with counter (G, 0, t, 0) and key (seed lo, seed hi)"""
    seed, t = 0x0123456789ABCDEF, 7
    w = AU.philox_words(seed, t, 32).to(torch.int64) & 0xFFFFFFFF
    for G in (0, 5):
        one = AU.philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), np.array([(G, 0, t, 0)], dtype=np.uint32))[0].tolist()
        assert w[4 * G:4 * G + 4].tolist() == one
    rm, rv = AU.word_halves(AU.philox_words(seed, t, 32))
    assert torch.equal(rm, w & 0xFFFF) and torch.equal(rv, w >> 16)
    assert not torch.equal(AU.philox_words(seed, t + 1, 32), AU.philox_words(seed, t, 32))


def test_a_bad_state_value_is_a_value_error(monkeypatch):
    from enhancing.engine.optim import GPTAdam
    monkeypatch.delenv("ENH_ADAM_STATE", raising=False)
    with pytest.raises(ValueError, match="fp8"):
        GPTAdam(None, lr=1e-3, state="fp8")          # refused before the GPT or the device is looked at
    assert GPTAdam._state_format(None) == "f32" and GPTAdam._state_format("bf16") == "bf16" and GPTAdam._state_format("f32") == "f32"


def test_the_environment_switch_is_read_and_checked(monkeypatch):
    from enhancing.engine.optim import GPTAdam
    monkeypatch.setenv("ENH_ADAM_STATE", "nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        GPTAdam(None, lr=1e-3)
    assert GPTAdam._state_format("bf16") == "bf16", "an explicit keyword does not read the environment"
    monkeypatch.setenv("ENH_ADAM_STATE", "bf16")
    assert GPTAdam._state_format(None) == "bf16"


def test_a_checkpoint_without_state_format_is_f32():
    from enhancing.engine.optim import GPTAdam
    old = dict(step=1, m=torch.zeros(64), v=torch.zeros(64))
    assert GPTAdam._checkpoint_format(old) == "f32"
    new = dict(old, m=old["m"].bfloat16(), v=old["v"].bfloat16(), state_format="bf16", state_seed=3)
    assert GPTAdam._checkpoint_format(new) == "bf16"
    with pytest.raises(ValueError, match="bfloat16"):
        GPTAdam._checkpoint_format(dict(old, m=old["m"].bfloat16()))      # a dict that calls itself f32 and holds bf16 moments
    with pytest.raises(ValueError, match="fp8"):
        GPTAdam._checkpoint_format(dict(old, state_format="fp8"))


def test_main_has_the_switch():
    import main
    p = main.build_parser()
    assert p.parse_args(["-c", "x"]).adam_state is None and p.parse_args(["-c", "x", "--adam_state", "bf16"]).adam_state == "bf16"
    with pytest.raises(SystemExit):
        p.parse_args(["-c", "x", "--adam_state", "fp8"])
