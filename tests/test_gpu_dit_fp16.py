"""The fp16 DiT forward's matrix-core route (`hh == true` in csrc/er_dit.h, dit_forward_impl: fp16 activations handed from producer to
consumer, V leaving the q/k/v product as V^T, cross K / V^T zero-padded per condition length) as a COMPOSITION, against the float64
restatement of that route, tests/dit_fp16_ref.py.

The bound comes from the references alone: d_ref is the distance between the float64 reference and the oracle's fp32 emulation of the
same roundings (arae_oracle.dit_forward under linear_input_rounding), recomputed in every run; the device may lie at most
MARGIN = 4 x d_ref from the float64 reference, in max abs and in rms.  tests/test_dit_fp16_ref_cpu.py shows without a GPU that d_ref is
less than half of what fp16 storage costs altogether and that a forward with the wrong batch row's gate, row 0's timestep for every row,
an unmasked padded key or layer 0's cross K / V in every layer lies more than 2 x MARGIN x d_ref away in every case where it applies.

Cases (layers, N, M, B), different timesteps per row: tests/dit_fp16_ref.py, FORWARD_CASES.  N = 100 takes the fallback route (fused
fp32-operand attention + register-staged GEMMs), whose roundings are the same values; B * N = 29 * 64 is the first size at which a
layer's product leaves the 64- / 128-row tiles (the feed-forward-in GEGLU product on the 256 x 256 tile), 31 * 64 the first at which
the feed-forward-out product streams.

Bit-exact properties (torch.equal): a batch row alone equals the row in its batch; the order of calls with other condition lengths and
batch sizes on one context changes nothing, and a fresh context agrees.

Measured on an MI355X, device error / d_ref (max abs, rms; d_ref itself moves by up to 40 % in max abs with the CPU that forms the
emulation's fp32 sums):
    forward L2-N64-M1-B1      2.43  2.38      (d_ref is small here: one key, the cross-attention has nothing to round)
    forward L2-N128-M63-B2    1.07  1.06
    forward L2-N128-M64-B3    1.43  1.23
    forward L2-N128-M65-B3    1.23  1.39
    forward L3-N192-M257-B2   1.27  1.28
    forward L2-N128-M300-B2   1.51  1.25
    forward L2-N100-M65-B2    1.43  1.18      (fallback route)
    forward L1-N64-M65-B29    1.24  1.14      (256 x 256 GEGLU tile)
    forward L1-N64-M65-B31    1.21  1.14      (+ streamed feed-forward-out)
    loss prediction           0.99  1.20
    sampler cfg3_repeat2      1.17  1.10
    sampler epsilon2          1.81  2.11
    sampler img2img4          1.00  0.65
All three bit-exact properties hold.  The device's absolute error is 2.7e-4 .. 3.4e-4 max, 5.0e-5 .. 8.1e-5 rms on every forward case
(outputs of rms 0.58): a third of what fp16 storage costs (1e-3 / 2.4e-4).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dit_fp16_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = R.MARGIN
_MODELS = {}


def model(layers, N, pred="v_prediction", fresh=False):
    """An fp16 MDiT per (layers, N, prediction type) on the case's weights; fresh: one more, not kept."""
    from edgerunner_amd.models_dit import MDiT
    key = (layers, N, pred)
    if fresh or key not in _MODELS:
        _, sd, _ = R.case_weights(layers, N)
        m = MDiT(R.case_options(layers, N, pred), DEV, clip_layers=0, precision="fp16")
        m.load_state_dict(sd, strict=True)
        if fresh:
            return m
        _MODELS[key] = m
    return _MODELS[key]


def check(what, got, y):
    """got within MARGIN x d_ref of the float64 reference, in max abs and in rms; all four numbers and both ratios printed first."""
    e_max, e_rms = R.dist(got, y["ref"])
    d_max, d_rms = y["d_ref"]
    print(f"{what}: device vs float64 max {e_max:.3e} rms {e_rms:.3e}; d_ref max {d_max:.3e} rms {d_rms:.3e}; "
          f"ratio max {e_max / d_max:.2f} rms {e_rms / d_rms:.2f} (bound {MARGIN:g})")
    assert torch.isfinite(got).all()
    assert e_max <= MARGIN * d_max, (what, e_max, d_max)
    assert e_rms <= MARGIN * d_rms, (what, e_rms, d_rms)


def device_forward(m, case, x, ch, t):
    cond = R.zero_row(case, m.get_cond(ch.to(DEV)))
    return m.dit(x.to(DEV), cond, t)


# ------------------------------------------------------------------ 1. the forward against the float64 reference
@pytest.mark.parametrize("case", R.FORWARD_CASES, ids=R.case_id)
def test_forward_vs_float64_reference(case):
    layers, N, M, B = case
    x, ch, t = R.case_inputs(case)
    got = device_forward(model(layers, N), case, x, ch, t)
    assert tuple(got.shape) == (B, N, 64)
    check(f"forward {R.case_id(case)}", got, R.case_yardstick(case))


# ------------------------------------------------------------------ 2. bit-exact properties
def test_batch_rows_are_independent():
    """Every launch of the route is row-independent: a row of the (2, 128, 65, 3) case run alone at B = 1 (its own timestep, its own
    condition - row 0's is the zero condition) gives the bits it had in the batch of three."""
    case = (2, 128, 65, 3)
    m = model(2, 128)
    x, ch, t = R.case_inputs(case)
    cond = R.zero_row(case, m.get_cond(ch.to(DEV)))
    full = m.dit(x.to(DEV), cond, t).clone()
    for b in range(3):
        alone = m.dit(x[b:b + 1].to(DEV), cond[b:b + 1].contiguous(), t[b:b + 1])
        diff = float((alone - full[b:b + 1]).abs().max())
        assert torch.equal(alone, full[b:b + 1]), f"row {b} alone differs from the row in its batch by {diff:.3e}"


def test_call_order_on_one_context_changes_nothing():
    """One context (2 layers, N = 128) through M = 257, B = 2 -> 63, 2 -> 65, 3 -> 300, 2 -> 257, 2 -> 63, 2: the cross K / V^T are
    prepared and zero-padded per call (257 and 300 share the padded length 320; 63 follows longer ones, so a stale pad would be read),
    the scratch only grows.  The repeats equal their first runs and the M = 63 result a fresh context's."""
    m = model(2, 128)
    seq = [(2, 128, 257, 2), (2, 128, 63, 2), (2, 128, 65, 3), (2, 128, 300, 2), (2, 128, 257, 2), (2, 128, 63, 2)]
    first = {}
    for case in seq:
        got = device_forward(m, case, *R.case_inputs(case)).clone()
        assert torch.isfinite(got).all()
        if case in first:
            diff = float((got - first[case]).abs().max())
            assert torch.equal(got, first[case]), f"{R.case_id(case)} after other shapes differs from its first run by {diff:.3e}"
        else:
            first[case] = got
    fresh = model(2, 128, fresh=True)
    try:
        case = (2, 128, 63, 2)
        want = device_forward(fresh, case, *R.case_inputs(case))
        assert torch.equal(first[case], want), "M = 63 after M = 257 differs from a fresh context's"
    finally:
        fresh.close()


def test_loss_prediction_in_fp16():
    """MDiT.forward(..., return_pred=True) in fp16 (er_dit_loss: add_noise on the device, then the same route): `pred` within the forward
    bound of the reference applied to sa * x0 + sb * noise with the host's coefficients, and equal to MDiT.dit at that input bit for bit."""
    import arae_oracle as O
    from edgerunner_amd.models_dit import dit_loss_coefficients
    case = (2, 128, 65, 3)
    opt, sd, sd64 = R.case_weights(2, 128)
    m = model(2, 128)
    x0, ch, t = R.case_inputs(case)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(41))
    sa, sb, _ = dit_loss_coefficients(t.long(), "v_prediction")
    xt = sa.view(-1, 1, 1) * x0 + sb.view(-1, 1, 1) * noise
    with torch.no_grad():
        ref = R.forward(sd64, xt, R.project_cond(sd64, ch), t, opt.dit_num_heads)
        sd_h = O.round_linear_weights(sd)
        with O.linear_input_rounding(torch.float16):
            emu = O.dit_forward(sd_h, xt, O.dit_project_cond(sd_h, ch), t, opt.dit_num_heads)
    out = m.forward({"cond": ch, "latents": x0}, noise=noise, timesteps=t.long(), return_pred=True)
    check("loss prediction L2-N128-M65-B3", out["pred"], dict(ref=ref, d_ref=R.dist(emu, ref)))
    assert torch.equal(out["pred"], m.dit(xt.to(DEV), m.get_cond(ch.to(DEV)), t))
    assert out["loss"].isfinite() and out["mse"].isfinite().all()


# ------------------------------------------------------------------ 3. the sampler against dit_fp16_ref.sample
@pytest.mark.parametrize("name", sorted(R.SAMPLER_CASES))
def test_sampler_vs_float64_reference(name):
    """MDiT.run in fp16 (er_dit_sample: CFG over [zero condition | cond], DDIM) at N = 128, M = 257, 2 layers: guidance 7.5 over three
    steps with two inputs and num_repeat = 2 (device batch 8), img2img from strength 0.5 over four steps, epsilon prediction over two."""
    c = R.SAMPLER_CASES[name]
    m = model(R.SAMPLER_LAYERS, R.SAMPLER_N, c["pred"])
    ch, noise, lat0 = R.sampler_inputs(name)
    kw = dict(latents=lat0.to(DEV), strength=c["strength"]) if c["img2img"] else {}
    got = m.run(ch.to(DEV), num_inference_steps=c["steps"], guidance_scale=c["guidance"], num_repeat=c["num_repeat"],
                noise=noise.to(DEV), **kw)
    assert tuple(got.shape) == tuple(noise.shape)
    check(f"sampler {name}", got, R.sampler_yardstick(name))
