"""The attention stress helper has teeth (tests/attn_stress_ref.py; no device, no library).

1. Every score profile does what its row in the helper's table says - on the constructed inputs, after rounding to each cache type,
   in float64 and in float32.
2. The fp32 emulation of the chunked online softmax passes the gate on every profile, length and chunk size.
3. Every mutant of the emulation fails the gate (or leaves a NaN / inf) on at least one profile - and `no_max`, the emulation without
   any max subtraction, PASSES on N(0, 1) scores at every length, which is why the stress tests exist."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_stress_ref as R  # noqa: E402

D = 96
CACHES = ["f32", "f16", "kv8"]
LENS = [1, 2, 3, 17, 129, 257, 2051, 6049]
CHUNKS = [32, 128, 256]
ATOL, RTOL = R.TOL_DECODE


def scores_of(name, n, cache, seed=0, H=2):
    """float64 scores [H, n] of the stored values of a constructed decode row"""
    q, k, v = R.decode_row(name, n, H, D, cache, R.gen(seed))
    ks, vs = R.from_cache(k), R.from_cache(v)
    assert bool(torch.isfinite(ks).all()) and bool(torch.isfinite(vs).all()) and bool(torch.isfinite(q).all())
    return (ks.double() * q.double()[:, None, :]).sum(-1) / math.sqrt(D)


def exp32(x):
    return torch.exp(x.float())


# ---------------------------------------------------------------------------------------------- 1. the profiles
@pytest.mark.parametrize("cache", CACHES)
def test_offsets_overflow_and_underflow_without_the_maximum(cache):
    for n in (1, 17, 2051):
        hi, lo = scores_of("offset_hi", n, cache), scores_of("offset_lo", n, cache)
        assert bool(torch.isinf(exp32(hi.max(-1).values)).all()), "exp(max score) must overflow fp32"
        assert float(hi.min()) > 80 and float(hi.max()) < 100
        assert float(exp32(lo).sum()) == 0.0, "every exp(score) must be exactly 0 in fp32"
        assert float(lo.min()) > -120
        for s in (hi, lo):                                    # and the row itself is an ordinary softmax row
            assert float((s.max(-1).values - s.min(-1).values).max()) < 12


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("name", ["rising", "falling"])
def test_ramps_move_the_maximum_in_every_chunk(name, cache):
    for n in (257, 2051, 6049):
        s = scores_of(name, n, cache)
        if name == "falling":
            s = s.flip(-1)
        tops = torch.stack([c.max(-1).values for c in s.split(128, dim=-1)], dim=-1)          # [H, chunks]
        assert bool((tops[:, 1:] > tops[:, :-1]).all()), "every 128-key chunk must bring a new maximum"
        if n >= 2051:
            assert float(exp32(tops[:, 0] - tops[:, -1]).max()) == 0.0, "the far end's mass must be exactly 0 in fp32 next to the near end's"


@pytest.mark.parametrize("cache", CACHES)
def test_spikes_hold_the_mass(cache):
    for n in (1, 2, 17, 257, 2051):
        for name in ("spike_first", "spike_last"):
            for dt in (torch.float64, torch.float32):
                p = torch.softmax(scores_of(name, n, cache).to(dt), dim=-1)
                assert float(p[:, R.spike_keys(name, n)[0]].min()) > 1 - 1e-6, (name, n, dt)
        p = torch.softmax(scores_of("two_spikes", n, cache), dim=-1)
        keys = R.spike_keys("two_spikes", n)
        assert float(p[:, keys].sum(-1).min()) > 1 - 1e-6
        assert float(p[:, keys].min()) > (0.25 if n > 1 else 0.99), "two spikes of comparable weight"


@pytest.mark.parametrize("cache", CACHES)
def test_flat_tail_holds_a_tenth_of_the_mass(cache):
    for dt in (torch.float64, torch.float32):
        p = torch.softmax(scores_of("flat_tail", 2051, cache).to(dt), dim=-1)
        tail = 1.0 - p[:, 0]
        assert 0.05 < float(tail.min()) and float(tail.max()) < 0.20, tail


@pytest.mark.parametrize("cache", CACHES)
def test_dead_chunks_are_exactly_dead(cache):
    for n in (129, 257, 2051):
        s = scores_of("dead_chunks", n, cache)
        chunks = s.split(R.DEAD_PERIOD, dim=-1)
        top = s.max(-1).values
        for c in chunks[1::2]:
            assert float(exp32(c.max(-1).values - top).max()) == 0.0, "a negative chunk's mass must be exactly 0 in fp32"
        for c in chunks[0::2]:
            assert float(exp32(c.max(-1).values - top).min()) > 1e-4, "a positive chunk is live"


@pytest.mark.parametrize("cache", CACHES)
def test_zero_q_scores_are_exactly_zero(cache):
    s = scores_of("zero_q", 257, cache)
    assert float(s.abs().max()) == 0.0
    c = R.decode_case(["zero_q"], [257], 2, D, cache)
    assert float((c.ref64[0] - c.expect[0]).abs().max()) < 1e-14


def test_decode_case_poisons_the_tail_and_keeps_the_rest_finite():
    for cache in CACHES:
        c = R.decode_case(list(R.PROFILES), [17] * len(R.PROFILES), 2, D, cache, seed=3)
        assert c.Lcap == 64 and c.kc.shape == (len(R.PROFILES), 2, 64, D)
        if cache == "kv8":
            assert bool(((c.kc[:, :, 17:] & 0x7F) == 0x7F).all()) and bool(((c.vc[:, :, 17:] & 0x7F) == 0x7F).all())
            assert not bool(((c.kc[:, :, :17] & 0x7F) == 0x7F).any())
        else:
            assert bool(torch.isnan(c.kc[:, :, 17:].float()).all()) and bool(torch.isnan(c.vc[:, :, 17:].float()).all())
            assert bool(torch.isfinite(c.kc[:, :, :17].float()).all())
        assert bool(torch.isfinite(c.ref64).all()) and bool(torch.isfinite(c.plain32).all())
        for b, name in enumerate(c.names):                     # the references agree with what the profile promises
            if c.expect[b] is not None:
                assert float((c.ref64[b] - c.expect[b]).abs().max()) < 1e-12, name


@pytest.mark.parametrize("rounding", ["none", "kv16", "qkv16"])
def test_flash_case_masks_its_spike_for_the_first_half_of_the_queries(rounding):
    N, M = 70, 200
    c = R.flash_case(["masked_spike"], 1, 2, N, M, D, True, seed=5, rounding=rounding)
    jstar = R.spike_keys("masked_spike", M, N)[0]
    assert jstar == (M - N) + N // 2
    s = c.qh.double() @ c.kh.double().transpose(-1, -2) / math.sqrt(D)            # [1, H, N, M], unmasked
    for i in range(N):
        if c.a[i] != 1.0:
            continue
        assert bool((s[0, :, i].argmax(-1) == jstar).all())
        assert bool(c.visible[i, jstar]) == (i >= N // 2)
        # masked: the visible scores sit so far below the masked maximum that exp(s - max) is exactly 0 in fp32
        if i < N // 2:
            vis = s[0, :, i, : i + (M - N) + 1]
            assert float(exp32(vis.max(-1).values - s[0, :, i, jstar]).max()) == 0.0
    assert bool(torch.isfinite(c.ref64).all()) and bool(torch.isfinite(c.plain32).all())
    rows, mean = R.flash_uniform_rows(c)
    assert float((c.ref64[:, :, rows] - mean).abs().max()) < 1e-12, "a = 0 queries give the mean of their visible V rows"


def test_softmax_case_references():
    for causal, cols in ((True, 300), (False, 1000)):
        c = R.softmax_case(300, cols, 1008, causal)
        assert bool(torch.isfinite(c.s).all()) and bool(torch.isfinite(c.ref64).all()) and bool(torch.isfinite(c.plain32).all())
        assert float((c.ref64.sum(-1) - 1).abs().max()) < 1e-12 and float(c.ref64[~c.valid].abs().max() if (~c.valid).any() else 0.0) == 0.0
        assert float(c.s[:, cols:].min()) == 70.0


# ---------------------------------------------------------------------------------------------- 2. the emulation passes
@functools.lru_cache(maxsize=None)
def one_head(name, n, cache="f32", seed=11):
    """(q [D], k, v [n, D] stored values fp32, ref64 [D], plain32 [D], visible or None) of one constructed head"""
    g = R.gen(seed + n)
    if name == "normal":                                       # what every other attention test feeds
        q, k, v = R.randn(g, 1, D).float(), R.randn(g, 1, n, D).float(), R.randn(g, 1, n, D).float()
    else:
        q, k, v = R.decode_row(name, n, 1, D, cache, g)
    q, k, v = q[0], R.from_cache(k)[0], R.from_cache(v)[0]
    visible = None
    if name == "masked_spike":                                 # the causal form: a query that sees the keys in front of the spike only
        visible = torch.arange(n) < max(1, R.spike_keys(name, n)[0])
    vis2 = None if visible is None else visible[None, :]
    return q, k, v, R.ref64(q[None], k, v, vis2)[0], R.plain32(q[None], k, v, vis2)[0], visible


def emu_ratio(name, n, chunk, mutant=None, cache="f32"):
    q, k, v, r64, p32, visible = one_head(name, n, cache)
    return R.ratio(R.emulate(q, k, v, chunk, mutant, visible), r64, p32, ATOL, RTOL)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_emulation_is_inside_the_gate(chunk):
    worst = (-1.0, ())
    for name in R.PROFILES + ("masked_spike", "normal"):
        for n in LENS:
            finite, r = emu_ratio(name, n, chunk)
            assert finite and r <= 1.0, (name, n, chunk, finite, r)
            worst = max(worst, (r, (name, str(n))))
    for cache in ("f16", "kv8"):
        for name in R.PROFILES:
            finite, r = emu_ratio(name, 257, chunk, cache=cache)
            assert finite and r <= 1.0, (name, cache, chunk, finite, r)
            worst = max(worst, (r, (name, cache)))
    print(f"emulation, chunk {chunk}: worst err / gate {worst[0]:.3f} at {worst[1]}")


def test_the_emulation_is_inside_the_rigorous_fp32_bound():
    """The worst case an fp32 kernel may reach (helper: fp32_score_bound) holds the emulation with room, and is far wider than the
    gate - it is the bound a kernel that misses the gate by a small factor is judged against, not the gate."""
    for name in ("offset_hi", "offset_lo", "rising", "dead_chunks"):
        q, k, v, r64, p32, _ = one_head(name, 257)
        err = float((R.emulate(q, k, v, 128).double() - r64).abs().max())
        assert err <= R.fp32_score_bound(q, k, v), name
        assert R.fp32_score_bound(q, k, v) > R.gate_of(r64, p32, ATOL, RTOL), name


# ---------------------------------------------------------------------------------------------- 3. every mutant fails
MUT_LENS = [17, 257, 2051]
MUT_CHUNKS = [128, 256]


@functools.lru_cache(maxsize=None)
def caught_by(mutant):
    """the (profile, n, chunk) cases on which a mutant misses the gate or leaves a NaN / inf"""
    out = []
    for name in R.PROFILES + ("masked_spike",):
        for n in MUT_LENS:
            for chunk in MUT_CHUNKS:
                finite, r = emu_ratio(name, n, chunk, mutant)
                if not finite or r > 1.0:
                    out.append((name, n, chunk))
    return out


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails_on_some_profile(mutant):
    caught = caught_by(mutant)
    print(f"mutant {mutant}: caught by {sorted({c[0] for c in caught})}")
    assert caught, f"mutant {mutant} passes the gate on every stress profile"


def test_no_max_is_invisible_to_normal_scores():
    """The reason this file exists: without ANY max subtraction the emulation passes on N(0, 1) scores at every length and chunk
    size, and the stress profiles catch it."""
    for n in LENS:
        for chunk in CHUNKS:
            finite, r = emu_ratio("normal", n, chunk, "no_max")
            assert finite and r <= 1.0, (n, chunk, finite, r)
    names = {c[0] for c in caught_by("no_max")}
    assert {"offset_hi", "offset_lo"} <= names, names


def test_the_classic_mutants_are_visible_to_normal_scores():
    """...while a dropped key, a key counted twice and merge weights of 1 are caught by N(0, 1) scores already."""
    for mutant in ("drop_last", "double_count", "merge_w1"):
        bad = [(n, chunk) for n in MUT_LENS for chunk in MUT_CHUNKS if (lambda fr: not fr[0] or fr[1] > 1.0)(emu_ratio("normal", n, chunk, mutant))]
        assert bad, mutant


def test_the_rescale_and_mask_mutants_need_their_profiles():
    assert "rising" in {c[0] for c in caught_by("skip_rescale")}
    assert {c[0] for c in caught_by("mask_after_max")} == {"masked_spike"}
    assert caught_by("empty_nan")
