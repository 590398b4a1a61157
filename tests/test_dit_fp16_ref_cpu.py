"""The yardstick of tests/test_gpu_dit_fp16.py, checked without a GPU (tests/dit_fp16_ref.py; no device, no library).

The GPU test bounds the device's distance to the float64 reference of the fp16 route by MARGIN x d_ref, where d_ref is the distance
between that reference and the oracle's fp32 emulation of the same roundings - two restatements of one rounded arithmetic that differ
in what a kernel may legitimately differ in (fp32 or float64 sums, the final or the per-tile running maximum in the softmax).  Here,
per forward case and from the references alone:

  d_ref < drift / 2     drift = reference vs the UNROUNDED float64 forward, i.e. everything fp16 storage costs: the two restatements
                        must be closer to each other than to the unrounded forward, or the yardstick measures nothing;
  every applicable deliberately wrong variant of the reference (wrong_gate_row, shared_timestep, unmasked_pad, layer0_cross_kv) lies
  more than 2 x MARGIN x d_ref from the correct one, in max abs AND in rms: a device that computed the variant could then not be
  within MARGIN x d_ref of the correct reference even if the reference itself were MARGIN x d_ref off.

d_ref is recomputed in every run and printed, never a committed constant."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dit_fp16_ref as R  # noqa: E402

MARGIN = R.MARGIN
VARIANTS = ("wrong_gate_row", "shared_timestep", "unmasked_pad", "layer0_cross_kv")


def applicable(variant, case):
    layers, N, M, B = case
    return {"wrong_gate_row": B > 1, "shared_timestep": B > 1, "unmasked_pad": M % 64 != 0, "layer0_cross_kv": layers > 1}[variant]


@pytest.mark.parametrize("case", R.FORWARD_CASES, ids=R.case_id)
def test_yardstick_and_wrong_variants(case):
    layers, N, M, B = case
    opt, sd, sd64 = R.case_weights(layers, N)
    x, ch, t = R.case_inputs(case)
    y = R.case_yardstick(case)
    d_max, d_rms = y["d_ref"]
    with torch.no_grad():
        sdu = R.weights64(sd, rounded=False)
        plain = R.forward(sdu, x, R.zero_row(case, R.project_cond(sdu, ch, R.ident)), t, opt.dit_num_heads, fp16=False)
        cond = R.zero_row(case, R.project_cond(sd64, ch))
        far = {v: R.dist(R.forward(sd64, x, cond, t, opt.dit_num_heads, **{v: True}), y["ref"]) for v in VARIANTS if applicable(v, case)}
    drift = R.dist(y["ref"], plain)
    print(f"{R.case_id(case)}: d_ref max {d_max:.3e} rms {d_rms:.3e}; drift max {drift[0]:.3e} rms {drift[1]:.3e} "
          f"(d_ref / drift {d_max / drift[0]:.2f} / {d_rms / drift[1]:.2f}); bar 2 x MARGIN x d_ref = {2 * MARGIN * d_max:.3e} / {2 * MARGIN * d_rms:.3e}")
    for v, (vm, vr) in far.items():
        print(f"    {v:16s} max {vm:.3e} ({vm / d_max:6.1f} x d_ref)  rms {vr:.3e} ({vr / d_rms:6.1f} x d_ref)")
    assert 0 < d_max < drift[0] / 2 and 0 < d_rms < drift[1] / 2
    assert far, "a case in which no wrong variant applies shows nothing"
    for v, (vm, vr) in far.items():
        assert vm > 2 * MARGIN * d_max and vr > 2 * MARGIN * d_rms, v


def test_unrounded_mode_is_the_oracle_forward():
    """With every rounding off the restatement is DiT.forward: it must agree with arae_oracle.dit_forward in float64 to the rounding
    of the one float32 quantity the oracle keeps (its sinusoid is evaluated in float32: <= 6e-8 per entry)."""
    import arae_oracle as O
    case = (2, 128, 65, 3)
    opt, sd, _ = R.case_weights(case[0], case[1])
    x, ch, t = R.case_inputs(case)
    sdu = R.weights64(sd, rounded=False)
    orig = O.timestep_embedding
    O.timestep_embedding = lambda tt, *a, **k: orig(tt, *a, **k).double()
    try:
        with torch.no_grad():
            want = O.dit_forward(sdu, x.double(), O.dit_project_cond(sdu, ch.double()), t.double(), opt.dit_num_heads)
            got = R.forward(sdu, x, R.project_cond(sdu, ch, R.ident), t, opt.dit_num_heads, fp16=False)
    finally:
        O.timestep_embedding = orig
    err = R.dist(got, want)[0]
    print(f"unrounded restatement vs the oracle in float64: max abs {err:.3e}")
    assert err < 1e-6


def test_attention_tiles_equal_plain_softmax_without_rounding():
    """The tile walk (running maximum, rescaled partial sums, masked tail) is the softmax when nothing is rounded, at every tile edge."""
    g = torch.Generator().manual_seed(3)
    for M in (1, 63, 64, 65, 257, 300):
        q, k, v = (torch.randn(2, 3, n, 64, generator=g, dtype=torch.float64) * s for n, s in ((70, 2.0), (M, 2.0), (M, 1.0)))
        want = torch.softmax((q @ k.transpose(-1, -2)) / 8.0, dim=-1) @ v
        got = R.attention(q, k, v, rnd=lambda p: p)
        assert float((got - want).abs().max()) < 1e-13, M
        # the fp16 P moves every p by at most 2^-11 of itself (5 % spare for the subnormal ones), the row sum is over the unrounded p
        assert float((R.attention(q, k, v) - want).abs().max()) < 2.0 ** -11 * float(v.abs().max()) * 1.05


def test_sample_restates_the_oracle_loop_and_both_prediction_types():
    """`sample` with the float64 reference as its forward is arae_oracle.mdit_run with that forward (v-prediction, from noise and
    img2img) up to the float32 scheduler coefficients of the latter; epsilon follows the CPU DDIM of tests/test_gpu_dit_loss.py."""
    import arae_oracle as O
    g = torch.Generator().manual_seed(9)
    cond = torch.randn(2, 5, 8, generator=g, dtype=torch.float64)
    noise = torch.randn(2, 6, 4, generator=g, dtype=torch.float64)
    lat0 = torch.randn(2, 6, 4, generator=g, dtype=torch.float64)
    w = torch.randn(4, 4, generator=g, dtype=torch.float64) * 0.5

    def fwd(x, c, t):                    # any deterministic map of (x, c, t) will do
        return torch.tanh(x @ w) + 0.1 * c.mean(dim=(1, 2), keepdim=True) + 1e-3 * t.view(-1, 1, 1).to(x.dtype) * x
    for kw in (dict(), dict(latents=lat0, strength=0.5), dict(latents=lat0, strength=0.0)):
        want = O.mdit_run({}, cond, noise, 1, num_inference_steps=4, guidance_scale=3.0, forward_fn=fwd, **kw)
        got = R.sample(fwd, cond, noise, 4, 3.0, "v_prediction", **kw)
        assert float((got - want).abs().max()) < 5e-6           # fp32 square roots of the table in mdit_run
    steps, gs = 5, 7.5
    ts, ac, final = O.ddim_schedule(steps)
    ac, x = ac.double(), noise.clone()
    c2 = torch.cat([torch.zeros_like(cond), cond])
    for t in ts:
        u, c = fwd(torch.cat([x, x]), c2, torch.tensor([float(t)] * 4, dtype=torch.float64)).chunk(2)
        e = u + gs * (c - u)
        a_t, a_p = ac[t], (ac[t - 1000 // steps] if t - 1000 // steps >= 0 else ac[0])
        x = a_p ** 0.5 * ((x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5) + (1 - a_p) ** 0.5 * e
    assert float((R.sample(fwd, cond, noise, steps, gs, "epsilon") - x).abs().max()) < 1e-12
    assert R.timesteps(4) == O.ddim_schedule(4)[0] and R.timesteps(3) == O.ddim_schedule(3)[0]


@pytest.mark.parametrize("name", sorted(R.SAMPLER_CASES))
def test_sampler_yardstick(name):
    """The sampler's d_ref exists and is small against the latents it measures (O(1)); printed for the record."""
    y = R.sampler_yardstick(name)
    d_max, d_rms = y["d_ref"]
    rms = float(y["ref"].pow(2).mean().sqrt())
    print(f"sampler {name}: d_ref max {d_max:.3e} rms {d_rms:.3e}; latents rms {rms:.3f}")
    assert 0 < d_rms < d_max < 0.05 * rms
