"""Plain-torch float64 restatement of the fp16 DiT forward's matrix-core route (`hh == true` in csrc/er_dit.h, dit_forward_impl),
launch by launch, for tests/test_dit_fp16_ref_cpu.py and tests/test_gpu_dit_fp16.py.  No device, no library, and not a wrapper of
oracle/arae_oracle.py: written from dit_forward_impl, dit_cross_kv, dit_time_embed and er_dit_project_cond.

All arithmetic is float64.  A value passes through torch.float16 (`h16`) exactly where the device stores fp16:

  every Linear's input (the x16 copies ln_modulate and the gated out-proj epilogue write, the attention outputs, the GEGLU output;
      the fp32 activations of proj_in, the time embedding, proj_cond and the cross k / v projections are rounded on their way into
      the GEMM), against weights rounded as arae_oracle.round_linear_weights rounds them (`weights64`);
  q, k and V as the q/k/v product leaves them (qkv16, V as V^T), the cross-attention q, K and V (dit_cross_kv);
  the attention outputs (att16) and the GEGLU output (g16).

The residual of both attentions is the MODULATED input (core/transformer/dit.py:133-135), kept in fp32 on the device: unrounded here.

The attention is fa_softmax_exp2 (csrc/k_flash_lanes.h): key tiles of FA_KT = 64, the running maximum over the scaled scores of the
tiles seen so far, the probabilities of a tile rounded to fp16 RELATIVE TO THAT running maximum for P.V, the row sum over the unrounded
probabilities, earlier partial sums and outputs rescaled when the maximum moves, keys >= M masked to -inf.

One input is formed in float32, as on the device and in diffusers: the sinusoid's argument t * exp(-ln(10000) k / 128) (the rounding
of a product near 1000 moves its sine by up to 6e-5, which is not an error of the code under test); the sine itself is float64.

`forward` takes four keyword switches that turn it into a deliberately WRONG forward, each off by default.  They exist so that the
CPU test can show that the bound the GPU test asserts separates the correct forward from these (reference side only; no code path of
the library knows them):

  wrong_gate_row    batch row 0's adaLN gates (gate_msa, gate_mlp) for every row
  shared_timestep   row 0's timestep for every row
  unmasked_pad      the keys [M, ceil64(M)) of the cross-attention attend as zero keys with zero V instead of being masked
  layer0_cross_kv   every layer reads layer 0's cross-attention K / V
"""
import math

import torch

FA_KT = 64
MARGIN = 4.0                  # the project's convention (tests/test_gpu_prefill_extend.py): a bound is MARGIN x the references' own distance
TRAIN_STEPS = 1000


def h16(x):
    """Through fp16 and back: what a store to an fp16 buffer keeps."""
    return x.to(torch.float16).to(torch.float64)


def ident(x):
    return x


def weights64(sd, rounded=True):
    """The state dict in float64.  rounded: every >= 2-D '.weight' through fp16 first (the fp16 copies WeightTable::half keeps; the rule
    of arae_oracle.round_linear_weights); biases, tables and norm vectors stay fp32 values."""
    def is_linear(k, v):
        return k.endswith(".weight") and v.dim() >= 2 and "position_embedding" not in k
    return {k: (h16(v) if rounded and is_linear(k, v) else v.to(torch.float64)) for k, v in sd.items()}


def num_layers(sd, prefix="dit"):
    n = 0
    while f"{prefix}.layers.{n}.scale_shift_table" in sd:
        n += 1
    return n


def linear(sd, prefix, x, rnd=h16):
    """A Linear on the fp16-input matrix cores: the activation rounded, the sum exact."""
    y = rnd(x) @ sd[f"{prefix}.weight"].transpose(0, 1)
    b = sd.get(f"{prefix}.bias")
    return y if b is None else y + b


def layer_norm(x, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


def silu(x):
    return x / (1.0 + torch.exp(-x))


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def timestep_embedding(t, half=128):
    """timestep_embed_kernel (csrc/k_dit.h): [sin(t w_k), cos(t w_k)], w_k = exp(-ln(10000) k / half); the argument in float32."""
    w = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    a = (t.to(torch.float32)[:, None] * w[None, :]).to(torch.float64)
    return torch.cat([torch.sin(a), torch.cos(a)], dim=-1)


def time_embed(sd, t, rnd=h16, prefix="dit"):
    """dit_time_embed: t [B] -> t_emb [B, C], t_adaln [B, 6, C]."""
    e = timestep_embedding(t)
    t_emb = linear(sd, f"{prefix}.timestep_proj.linear_2", silu(linear(sd, f"{prefix}.timestep_proj.linear_1", e, rnd)), rnd)
    t_adaln = linear(sd, f"{prefix}.adaln_linear", silu(t_emb), rnd)
    return t_emb, t_adaln.view(t.shape[0], 6, -1)


def project_cond(sd, clip_hidden, rnd=h16):
    """er_dit_project_cond: norm_cond(proj_cond(clip_hidden)), LayerNorm eps 1e-5 with weight and bias."""
    y = linear(sd, "proj_cond", clip_hidden.to(torch.float64), rnd)
    return layer_norm(y, 1e-5) * sd["norm_cond.weight"] + sd["norm_cond.bias"]


def attention(q, k, v, rnd=h16, unmasked_pad=False):
    """flash_attn_hh_kernel: q [B, H, N, D], k / v [B, H, M, D], values already as stored (fp16) -> [B, H, N, D], not yet rounded.
    rnd = ident: the plain softmax (the unrounded forward)."""
    D, M = q.shape[-1], k.shape[-2]
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    if rnd is ident:
        return torch.softmax(s, dim=-1) @ v
    if unmasked_pad and M % FA_KT:
        pad = FA_KT - M % FA_KT                     # the zero-padded rows of K / V^T, scored (q . 0 = 0) instead of masked
        s = torch.cat([s, s.new_zeros(s.shape[:-1] + (pad,))], dim=-1)
        v = torch.cat([v, v.new_zeros(v.shape[:-2] + (pad, D))], dim=-2)
    m_run = s.new_full(s.shape[:-1] + (1,), -math.inf)
    l_run = s.new_zeros(s.shape[:-1] + (1,))
    o = s.new_zeros(q.shape)
    for k0 in range(0, s.shape[-1], FA_KT):
        st = s[..., k0:k0 + FA_KT]                  # the last tile holds only the keys < M: the others are masked to -inf, p = 0
        m_new = torch.maximum(m_run, st.amax(dim=-1, keepdim=True))
        alpha = torch.exp(m_run - m_new)            # the first tile: exp(-inf) = 0
        p = torch.exp(st - m_new)
        l_run = l_run * alpha + p.sum(dim=-1, keepdim=True)
        o = o * alpha + rnd(p) @ v[..., k0:k0 + FA_KT, :]
        m_run = m_new
    return o / l_run


def heads(x, H):
    B, N, C = x.shape
    return x.view(B, N, H, C // H).transpose(1, 2)


def unheads(x):
    B, H, N, D = x.shape
    return x.transpose(1, 2).reshape(B, N, H * D)


def cross_kv(sd, cond, H, rnd=h16, prefix="dit"):
    """dit_cross_kv: per layer the cross-attention K and V of the condition, as stored (fp16), [B, H, M, D] each."""
    return [(heads(rnd(linear(sd, f"{prefix}.layers.{i}.attn2.k_proj", cond, rnd)), H),
             heads(rnd(linear(sd, f"{prefix}.layers.{i}.attn2.v_proj", cond, rnd)), H)) for i in range(num_layers(sd, prefix))]


def forward(sd, x, cond, t, num_heads, fp16=True, wrong_gate_row=False, shared_timestep=False, unmasked_pad=False,
            layer0_cross_kv=False, prefix="dit"):
    """DiT.forward on the hh route: x [B, N, latent_dim], cond [B, M, C] (projected), t [B] -> [B, N, latent_dim], float64.
    sd: `weights64(state_dict)`.  fp16 = False: no rounding anywhere (with `weights64(state_dict, rounded=False)`: the unrounded
    float64 forward)."""
    rnd = h16 if fp16 else ident
    H = num_heads
    x, cond, t = x.to(torch.float64), cond.to(torch.float64), t.to(torch.float64)
    B = x.shape[0]
    if shared_timestep:
        t = t[:1].expand(B).clone()
    t_emb, t_adaln = time_embed(sd, t, rnd, prefix)
    kv = cross_kv(sd, cond, H, rnd, prefix)
    # x = proj_in(x) + pos_embed                                                     dit.py:177-180
    x = linear(sd, f"{prefix}.proj_in", x, rnd) + sd[f"{prefix}.pos_embed"].view(1, x.shape[1], -1)
    C = x.shape[-1]
    for i in range(num_layers(sd, prefix)):
        L = f"{prefix}.layers.{i}"
        mod = sd[f"{L}.scale_shift_table"][None] + t_adaln                       # [B, 6, C]: shift, scale, gate (msa), the same (mlp)
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = (mod[:, j:j + 1] for j in range(6))
        if wrong_gate_row:
            g_a, g_m = g_a[:1], g_m[:1]
        # ln_modulate: x (fp32) and x16
        x = layer_norm(x, 1e-6) * (1 + sc_a) + sh_a
        # q/k/v product: q, k leave in fp16, V as V^T in fp16; self-attention over the N latent tokens (no padding: 64 | N)
        qkv = rnd(linear(sd, f"{L}.attn1.qkv_proj", x, rnd))
        q, k, v = (heads(u, H) for u in qkv.chunk(3, dim=-1))
        att = rnd(unheads(attention(q, k, v, rnd)))
        # out-proj with the gate and the residual in its epilogue; its fp16 copy feeds the cross-attention query projection
        x = x + g_a * linear(sd, f"{L}.attn1.out_proj", att, rnd)
        q2 = heads(rnd(linear(sd, f"{L}.attn2.q_proj", x, rnd)), H)
        k2, v2 = kv[0 if layer0_cross_kv else i]
        att = rnd(unheads(attention(q2, k2, v2, rnd, unmasked_pad)))
        x = x + linear(sd, f"{L}.attn2.out_proj", att, rnd)
        x = layer_norm(x, 1e-6) * (1 + sc_m) + sh_m
        # feed-forward in + GEGLU in one launch: value * gelu(gate) leaves in fp16
        u, g = linear(sd, f"{L}.ff.net.0", x, rnd).chunk(2, dim=-1)
        x = x + g_m * linear(sd, f"{L}.ff.net.2", rnd(u * gelu(g)), rnd)
    # final modulate (scale_shift_table [2, C] + t_emb) and proj_out                 dit.py:190-194
    mod = sd[f"{prefix}.scale_shift_table"][None] + t_emb[:, None]
    x = layer_norm(x, 1e-6) * (1 + mod[:, 1:2]) + mod[:, 0:1]
    return linear(sd, f"{prefix}.proj_out", x, rnd)


# ------------------------------------------------------------------------------------------------ the sampler (MDiT.run)
def alphas_cumprod():
    """diffusers' DDIMScheduler table for the reference's configuration (scaled_linear betas 0.00085 .. 0.012, 1000 steps), formed in
    float32 as diffusers forms it; every use of it below is float64."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, TRAIN_STEPS, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).to(torch.float64)


def timesteps(steps):
    """'leading' spacing with steps_offset 1, descending."""
    ratio = TRAIN_STEPS // steps
    return [(steps - 1 - i) * ratio + 1 for i in range(steps)]


def ddim_step(sample, pred, t, ratio, ac, prediction_type):
    """DDIMScheduler.step, eta 0, no clipping, set_alpha_to_one False (the final alpha is ac[0])."""
    a_t = float(ac[t])
    a_p = float(ac[t - ratio]) if t - ratio >= 0 else float(ac[0])
    if prediction_type == "epsilon":
        eps = pred
        x0 = (sample - math.sqrt(1 - a_t) * eps) / math.sqrt(a_t)
    elif prediction_type == "v_prediction":
        x0 = math.sqrt(a_t) * sample - math.sqrt(1 - a_t) * pred
        eps = math.sqrt(a_t) * pred + math.sqrt(1 - a_t) * sample
    else:
        raise ValueError(prediction_type)
    return math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * eps


def sample(forward_fn, cond, noise, steps, guidance, prediction_type="v_prediction", latents=None, strength=0.5):
    """MDiT.run (core/models_dit.py:184-229) after get_cond / repeat_interleave: classifier-free guidance over [zero condition | cond]
    and DDIM, in float64.  forward_fn(x [2B, N, L], c [2B, M, C], t [2B]) -> the DiT's prediction.  `latents` given: the img2img branch
    (noise added at timesteps[int(steps * strength)], the loop over the timesteps from there on)."""
    cond, noise = cond.to(torch.float64), noise.to(torch.float64)
    ac, ts, ratio = alphas_cumprod(), timesteps(steps), TRAIN_STEPS // steps
    B = cond.shape[0]
    if latents is None:
        init, lat = 0, noise.clone()
    else:
        init = int(steps * strength)
        a_t = float(ac[ts[init]])
        lat = math.sqrt(a_t) * latents.to(torch.float64) + math.sqrt(1 - a_t) * noise
    c2 = torch.cat([torch.zeros_like(cond), cond], dim=0)
    for t in ts[init:]:
        pred = forward_fn(torch.cat([lat, lat], dim=0), c2, torch.full((2 * B,), float(t), dtype=torch.float64)).to(torch.float64)
        u, c = pred.chunk(2)
        lat = ddim_step(lat, u + guidance * (c - u), t, ratio, ac, prediction_type)
    return lat


# ------------------------------------------------------------------------------------------------ distances
def dist(a, b):
    """(max abs, rms) of a - b in float64."""
    d = a.detach().cpu().to(torch.float64) - b.detach().cpu().to(torch.float64)
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------ the cases both test files use
# (layers, N, M, B): rows of the issue's table.  N = 100 is the fallback route (fused fp32-operand attention + register-staged GEMMs:
# the same values are rounded there).  The last row is the smallest B * N at which the launch rule of the fp16 GEMMs leaves the
# 64- / 128-row tiles for one of a layer's products: gemm_hh_use_256 (csrc/k_gemm.h) wants ceil(R / 256) * ceil(Nout / 256) >= 256,
# which the feed-forward-in product (Nout = 8 C = 8192: 32 tile columns) reaches first, at R = B * N > 7 * 256, i.e. 29 * 64 = 1856 rows
# (q/k/v, Nout = 3072, needs R > 5376; the streamed form of the feed-forward-out product, gemm_hh_use_stream, R > 1920).  29 batch
# rows of 64 tokens keep the attention small and put four batch rows - four gate rows, four timesteps - into every 256-row tile.
# One more row than the table asks for: 31 * 64 = 1984 rows, the first size at which the feed-forward-out product takes the streamed
# form as well (its epilogue carries the gate and the residual).
FORWARD_CASES = [(2, 64, 1, 1), (2, 128, 63, 2), (2, 128, 64, 3), (2, 128, 65, 3), (3, 192, 257, 2), (2, 128, 300, 2), (2, 100, 65, 2),
                 (1, 64, 65, 29), (1, 64, 65, 31)]
ZERO_COND_ROW = {(2, 128, 65, 3): 0}        # this case's projected condition has one row set to zero (the CFG half's input)
T_ROWS = (801.0, 41.0, 999.0)
SEED = 5
# One padded key of 64 is a small effect.  With independent CLIP tokens the cross-attention output is a mean of 63 unrelated values, an
# eighth of their size, and unmasked_pad at M = 63 lies only 8 to 10 x d_ref (max abs) from the reference, whatever the seed or the
# timesteps - at the bar of 2 x MARGIN = 8, and d_ref's max abs moves by up to 40 % with the CPU that forms the fp32 sums.  Real CLIP tokens
# share a large common part; with one of the noise's own size in this case the output keeps its size and the variant lies 24 to 36 x d_ref
# away (14 seeds), d_ref / drift at 0.31 to 0.41.  (In every case it makes d_ref larger, 0.35 to 0.4 of drift: the other cases keep
# independent tokens.)  (seed, size of the common part); every other case: the formula in case_inputs and none.
CASE_INPUT = {(2, 128, 63, 2): (11, 1.0)}


def case_id(case):
    return "L{}-N{}-M{}-B{}".format(*case)


def case_options(layers, N, pred="v_prediction"):
    import dataclasses
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy", cond_mode="point_latent",
                               dit_num_layers=layers, point_latent_size=N, noise_scheduler_predtype=pred)


_WEIGHTS = {}


def case_weights(layers, N):
    """(options, fp32 state dict, its rounded float64 copy) per (layers, N), made once."""
    from edgerunner_amd import weights as W
    if (layers, N) not in _WEIGHTS:
        opt = case_options(layers, N)
        sd = W.make_dit_state_dict(opt, SEED, "perturbed")
        _WEIGHTS[(layers, N)] = (opt, sd, weights64(sd))
    return _WEIGHTS[(layers, N)]


def case_timesteps(B):
    """Different per row; beyond three rows a spread over the whole table."""
    if B <= len(T_ROWS):
        return torch.tensor(T_ROWS[:B])
    return torch.tensor([float((37 * b * b + 801 * (b + 1)) % TRAIN_STEPS) for b in range(B)])


def case_inputs(case):
    """x [B, N, 64], CLIP hidden states [B, M, 1280], t [B]: float32, from the case's own seed."""
    layers, N, M, B = case
    seed, common = CASE_INPUT.get(case, (1000 * layers + 7 * N + 13 * M + B, 0.0))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, 64, generator=g)
    clip_hidden = torch.randn(B, M, 1280, generator=g)
    if common:
        clip_hidden = clip_hidden + common * torch.randn(B, 1, 1280, generator=g)
    return x, clip_hidden, case_timesteps(B)


def zero_row(case, cond):
    if case in ZERO_COND_ROW:
        cond = cond.clone()
        cond[ZERO_COND_ROW[case]] = 0
    return cond


_YARD = {}


def case_yardstick(case):
    """Per case, made once: the float64 reference of the forward (`ref`), the oracle's fp32 emulation of the same roundings (`emu`:
    arae_oracle.dit_forward under linear_input_rounding - the final row maximum in its softmax, fp32 sums) and d_ref = dist(emu, ref):
    how far two restatements of the same rounded arithmetic lie apart.  The bound on the device is MARGIN x d_ref."""
    import arae_oracle as O
    if case not in _YARD:
        layers, N, M, B = case
        opt, sd, sd64 = case_weights(layers, N)
        x, ch, t = case_inputs(case)
        with torch.no_grad():
            ref = forward(sd64, x, zero_row(case, project_cond(sd64, ch)), t, opt.dit_num_heads)
            sd_h = O.round_linear_weights(sd)
            with O.linear_input_rounding(torch.float16):
                emu = O.dit_forward(sd_h, x, zero_row(case, O.dit_project_cond(sd_h, ch)), t, opt.dit_num_heads)
        _YARD[case] = dict(ref=ref, emu=emu, d_ref=dist(emu, ref))
    return _YARD[case]


# ------------------------------------------------------------------------------------------------ the sampler cases
# N = 128, M = 257, 2 layers; guidance 7.5 (the amplifier of MDiT.run's default).  inputs x num_repeat = the batch, twice that on the device.
SAMPLER_LAYERS, SAMPLER_N, SAMPLER_M = 2, 128, 257
SAMPLER_CASES = {
    "cfg3_repeat2": dict(steps=3, guidance=7.5, inputs=2, num_repeat=2, pred="v_prediction", img2img=False),     # device batch 8
    "img2img4": dict(steps=4, guidance=7.5, inputs=2, num_repeat=1, pred="v_prediction", img2img=True, strength=0.5),
    "epsilon2": dict(steps=2, guidance=7.5, inputs=1, num_repeat=1, pred="epsilon", img2img=False),
}


def sampler_inputs(name):
    """CLIP hidden states [inputs, M, 1280], noise [B, N, 64] and, for img2img, the latents to start from [B, N, 64]."""
    c = SAMPLER_CASES[name]
    g = torch.Generator().manual_seed(sorted(SAMPLER_CASES).index(name) + 77)
    B = c["inputs"] * c["num_repeat"]
    ch = torch.randn(c["inputs"], SAMPLER_M, 1280, generator=g)
    noise = torch.randn(B, SAMPLER_N, 64, generator=g)
    lat0 = 0.5 * torch.randn(B, SAMPLER_N, 64, generator=g) if c["img2img"] else None
    return ch, noise, lat0


def sampler_yardstick(name):
    """As case_yardstick, for MDiT.run: `emu` = the sampling loop over the oracle's fp32 emulation, `ref` = the same loop over the
    float64 reference.  v-prediction: arae_oracle.mdit_run both times (with forward_fn = the reference); epsilon, which mdit_run does
    not have: `sample` both times (with forward_fn = the emulation)."""
    import arae_oracle as O
    key = ("sampler", name)
    if key not in _YARD:
        c = SAMPLER_CASES[name]
        opt, sd, sd64 = case_weights(SAMPLER_LAYERS, SAMPLER_N)
        H = opt.dit_num_heads
        ch, noise, lat0 = sampler_inputs(name)
        sd_h = O.round_linear_weights(sd)
        ref_fwd = lambda x, cc, t: forward(sd64, x, cc, t, H)
        with torch.no_grad():
            cond64 = project_cond(sd64, ch).repeat_interleave(c["num_repeat"], dim=0)
            with O.linear_input_rounding(torch.float16):
                cond32 = O.dit_project_cond(sd_h, ch).repeat_interleave(c["num_repeat"], dim=0)
                if c["pred"] == "v_prediction":
                    kw = dict(num_inference_steps=c["steps"], guidance_scale=c["guidance"])
                    if c["img2img"]:
                        kw.update(latents=lat0, strength=c["strength"])
                    emu = O.mdit_run(sd_h, cond32, noise, H, **kw)
                    if c["img2img"]:
                        kw.update(latents=lat0.double())
                    ref = O.mdit_run(sd_h, cond64, noise.double(), H, forward_fn=ref_fwd, **kw)
                else:
                    emu_fwd = lambda x, cc, t: O.dit_forward(sd_h, x.float(), cc.float(), t.float(), H)
                    emu = sample(emu_fwd, cond32, noise, c["steps"], c["guidance"], c["pred"])
                    ref = sample(ref_fwd, cond64, noise, c["steps"], c["guidance"], c["pred"])
        _YARD[key] = dict(ref=ref, emu=emu, d_ref=dist(emu, ref))
    return _YARD[key]
