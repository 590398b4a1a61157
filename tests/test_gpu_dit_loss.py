"""DiT eval loss on the GPU: ``MDiT.forward`` (core/models_dit.py:119-181 in eval mode) through er_dit_loss / er_dit_point_latent /
er_k_dit_loss, against float64 CPU restatements built on the committed oracle (arae_oracle.dit_forward, point_encoder_embed) and
diffusers' add_noise / get_velocity / compute_snr restated below; the epsilon DDIM sampler; score_dit.py end to end."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
T3 = [0, 517, 999]


def opt_for(pred="v_prediction", **kw):
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy", dit_num_layers=2,
                               noise_scheduler_predtype=pred, **kw)


@pytest.fixture(scope="module")
def weights():
    from edgerunner_amd import weights as W
    opt = opt_for()
    sd_lmm = W.make_state_dict(opt, 0, "perturbed")                 # cond_mode 'point': holds point_encoder.*
    pe = {k: v for k, v in sd_lmm.items() if k.startswith("point_encoder.")}
    sd_dit = W.make_dit_state_dict(opt, 0, "perturbed")
    return opt, sd_lmm, pe, sd_dit


_MODELS = {}


def mdit(weights, pred="v_prediction", precision="fp32", point_encoder=True):
    from edgerunner_amd.models_dit import MDiT
    key = (pred, precision, point_encoder)
    if key not in _MODELS:
        _, _, pe, sd_dit = weights
        m = MDiT(opt_for(pred), DEV, clip_layers=0, precision=precision, point_encoder=point_encoder)
        m.load_state_dict(dict(sd_dit, **pe) if point_encoder else sd_dit, strict=True)
        _MODELS[key] = m
    return _MODELS[key]


def cloud(i, n):
    from edgerunner_amd import weights as W
    return W.synthetic_point_cloud(i, n)


# ------------------------------------------------------------------ float64 restatements (diffusers is not installed)
def alphas_cumprod_f64():
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2     # DDPMScheduler, scaled_linear
    return torch.from_numpy(np.cumprod(1.0 - betas))


def add_noise(x0, eps, t):              # DDPMScheduler.add_noise
    ac = alphas_cumprod_f64()[t].view(-1, 1, 1)
    return ac.sqrt() * x0 + (1 - ac).sqrt() * eps


def get_velocity(x0, eps, t):           # DDPMScheduler.get_velocity
    ac = alphas_cumprod_f64()[t].view(-1, 1, 1)
    return ac.sqrt() * eps - (1 - ac).sqrt() * x0


def compute_snr(t):                     # diffusers.training_utils.compute_snr
    ac = alphas_cumprod_f64()[t]
    return (ac.sqrt() / (1 - ac).sqrt()) ** 2


def reference_loss(pred, x0, eps, t, pred_type, gamma):
    """core/models_dit.py:158-177 in float64 -> (mse [B], loss)."""
    target = eps if pred_type == "epsilon" else get_velocity(x0, eps, t)
    mse = ((pred - target) ** 2).mean(dim=(1, 2))
    if gamma is None:
        return mse, mse.mean()
    snr = compute_snr(t)
    w = torch.minimum(snr, torch.full_like(snr, gamma))
    w = w / snr if pred_type == "epsilon" else w / (snr + 1)
    return mse, (mse * w).mean()


@pytest.fixture(scope="module")
def case(weights):
    """B = 3 at timesteps {0, 517, 999}: latents with a few NaNs, noise, CLIP hidden states, and the float64 oracle's prediction."""
    import arae_oracle as O
    opt, _, _, sd_dit = weights
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(3, 2048, 64, generator=g)
    x0[0, 5, 7] = x0[2, 2047, 63] = float("nan")
    eps = torch.randn(3, 2048, 64, generator=g)
    ch = torch.randn(3, 257, 1280, generator=g)
    t = torch.tensor(T3)
    sd64 = {k: v.double() for k, v in sd_dit.items()}
    x0c = torch.nan_to_num(x0.double(), 0.0)
    orig = O.timestep_embedding
    O.timestep_embedding = lambda tt, *a, **k: orig(tt, *a, **k).double()   # the oracle's sinusoid is fp32: widen it for the float64 run
    try:
        pred64 = O.dit_forward(sd64, add_noise(x0c, eps.double(), t), O.dit_project_cond(sd64, ch.double()), t.double(), opt.dit_num_heads)
    finally:
        O.timestep_embedding = orig
    return x0, eps, ch, t, x0c, pred64


# ------------------------------------------------------------------ 1. the point encoder inside the DiT context
def test_point_latent_equals_lmm_encoder_and_oracle(weights):
    import arae_oracle as O
    from edgerunner_amd.models import LMM
    opt, sd_lmm, pe, _ = weights
    lmm = LMM(opt, DEV)
    lmm.load_state_dict(sd_lmm, strict=True)
    m = mdit(weights)
    worst = 0.0
    for pcs in (torch.cat([cloud(0, 1000), cloud(1, 1000)]), cloud(2, 1537)):
        got = m.point_latent(pcs.to(DEV))
        want, _ = lmm.mesh_decoder.point_latent(pcs.to(DEV))
        assert tuple(got.shape) == (pcs.shape[0], 2048, 64)
        assert torch.equal(got, want), "er_dit_point_latent must run the LMM context's launch sequence"
        worst = max(worst, float((got.cpu() - O.point_encoder_embed(sd_lmm, pcs, opt.point_num_heads)).abs().max()))
    print(f"point latent: bit-identical to LMM.mesh_decoder.point_latent; max abs err vs oracle {worst:.3e}")
    assert worst <= 1e-5                       # measured 6.7e-7


# ------------------------------------------------------------------ 2. the loss against the float64 restatement
@pytest.mark.parametrize("pred_type", ["v_prediction", "epsilon"])
def test_loss_vs_float64_oracle(weights, case, pred_type):
    from edgerunner_amd.models_dit import dit_loss_coefficients
    x0, eps, ch, t, x0c, pred64 = case
    m = mdit(weights, pred_type)
    worst = {}
    base = m.opt
    for gamma in (5.0, None):
        m.opt = dataclasses.replace(base, snr_gamma=gamma)
        try:
            out = m.forward({"cond": ch, "latents": x0}, noise=eps, timesteps=t, return_pred=True)
        finally:
            m.opt = base
        want_mse, want_loss = reference_loss(pred64, x0c, eps.double(), t, pred_type, gamma)
        r_mse = float(((out["mse"].cpu().double() - want_mse).abs() / want_mse).max())
        r_loss = abs(float(out["loss"]) - float(want_loss)) / float(want_loss)
        worst[gamma] = (r_mse, r_loss)
        assert out["loss"].dim() == 0 and tuple(out["mse"].shape) == (3,) and out["timesteps"].tolist() == T3
        assert r_mse < 2e-6 and r_loss < 2e-6, (gamma, r_mse, r_loss)      # measured <= 1.6e-7
        w = out["weights"].cpu().double()
        assert abs(float((w * out["mse"].cpu().double()).mean()) - float(out["loss"])) <= 1e-6 * float(out["loss"])
    # the prediction is the DiT's output at x_t, bit for bit (x_t rebuilt from the host coefficients)
    sa, sb, _ = dit_loss_coefficients(t, pred_type)
    xt = sa.view(-1, 1, 1) * torch.nan_to_num(x0, 0.0) + sb.view(-1, 1, 1) * eps
    ref = m.dit(xt.to(DEV), m.get_cond(ch.to(DEV)), t.float())
    assert torch.equal(out["pred"], ref)
    print(f"{pred_type}: rel err vs float64 (mse, loss): gamma 5 {worst[5.0][0]:.2e} / {worst[5.0][1]:.2e}, "
          f"None {worst[None][0]:.2e} / {worst[None][1]:.2e}; pred == MDiT.dit(x_t) bit for bit")


# ------------------------------------------------------------------ 3. determinism and inputs
def test_deterministic_nan_inf_and_points(weights, case):
    x0, eps, ch, t, _, _ = case
    m = mdit(weights)
    data = {"cond": ch, "latents": x0}
    a = m.forward(data, noise=eps, timesteps=t)
    b = m.forward(data, noise=eps, timesteps=t)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["mse"], b["mse"])
    bad = x0.clone()
    bad[1, 10, 3], bad[1, 11, 4], bad[0, 0, 0] = float("inf"), float("-inf"), float("nan")
    got = m.forward({"cond": ch, "latents": bad}, noise=eps, timesteps=t, return_pred=True)
    want = m.forward({"cond": ch, "latents": torch.nan_to_num(bad, 0.0)}, noise=eps, timesteps=t, return_pred=True)
    assert torch.equal(got["mse"], want["mse"]) and torch.equal(got["pred"], want["pred"])
    # points through the attached encoder == latents from point_latent
    pcs = torch.cat([cloud(3, 1024), cloud(4, 1024), cloud(5, 1024)])
    p = m.forward({"cond": ch, "points": pcs}, noise=eps, timesteps=t)
    q = m.forward({"cond": ch, "latents": m.point_latent(pcs.to(DEV))}, noise=eps, timesteps=t)
    assert torch.equal(p["loss"], q["loss"]) and torch.equal(p["mse"], q["mse"])
    # default draws: torch.randn then torch.randint from the generator
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    r = m.forward(data, generator=g1)
    nz = torch.randn((3, 2048, 64), generator=g2)
    tt = torch.randint(0, 1000, (3,), generator=g2)
    s = m.forward(data, noise=nz, timesteps=tt)
    assert torch.equal(r["timesteps"], tt) and torch.equal(r["loss"], s["loss"])
    print(f"loss {float(a['loss']):.6f}; reproducible; NaN/inf latents == nan_to_num latents; points == point_latent")


# ------------------------------------------------------------------ 4. the loss kernels on their own
@pytest.mark.parametrize("B,shape", [(1, (2048, 64)), (7, (1000, 4)), (64, (3, 12292))])
@pytest.mark.parametrize("pred_type", [0, 1])
def test_loss_kernels_vs_numpy(B, shape, pred_type):
    from edgerunner_amd import kernels as K
    from edgerunner_amd.models_dit import dit_loss_coefficients
    g = torch.Generator().manual_seed(B * 10 + pred_type)
    pred, x0, eps = (torch.randn((B,) + shape, generator=g) * s for s in (1.0, 0.7, 1.3))
    t = torch.randint(0, 1000, (B,), generator=g)
    t[0] = 0
    name = "epsilon" if pred_type else "v_prediction"
    for gamma in (5.0, None):
        mse, loss = K.dit_loss(pred.to(DEV), x0.to(DEV), eps.to(DEV), t, pred_type, gamma)
        sa, sb, w = (v.double().numpy() for v in dit_loss_coefficients(t, name, gamma))
        p, x, e = (v.double().numpy().reshape(B, -1) for v in (pred, x0, eps))
        # the target in fp32 as the kernel (and torch) forms it, then float64 from there on
        tgt = e if pred_type else (sa[:, None].astype(np.float32) * e.astype(np.float32)
                                   - sb[:, None].astype(np.float32) * x.astype(np.float32)).astype(np.float64)
        want_mse = ((p - tgt) ** 2).mean(axis=1)
        want_loss = (w * want_mse).mean()
        assert np.abs(mse.cpu().double().numpy() / want_mse - 1).max() < 1e-6
        assert abs(float(loss[0]) / want_loss - 1) < 1e-6
        mse2, loss2 = K.dit_loss(pred.to(DEV), x0.to(DEV), eps.to(DEV), t, pred_type, gamma)
        assert torch.equal(mse, mse2) and torch.equal(loss, loss2)


# ------------------------------------------------------------------ 5. epsilon sampling
def test_epsilon_sampler_vs_cpu_ddim(weights):
    import arae_oracle as O
    opt, _, _, sd_dit = weights
    m = mdit(weights, "epsilon")
    gen = torch.Generator().manual_seed(11)
    ch = torch.randn(1, 257, 1280, generator=gen)
    nz = torch.randn(1, 2048, 64, generator=gen)
    steps, gs = 6, 7.5
    ts, ac, final = O.ddim_schedule(steps)
    ratio = 1000 // steps
    cond = O.dit_project_cond(sd_dit, ch)
    c2 = torch.cat([torch.zeros_like(cond), cond])
    x = nz.clone()
    for t in ts:                          # DDIMScheduler.step, prediction_type 'epsilon', eta 0
        pred = O.dit_forward(sd_dit, torch.cat([x, x]), c2, torch.tensor([float(t)] * 2), opt.dit_num_heads)
        u, c = pred.chunk(2)
        e = u + gs * (c - u)
        a_t = ac[t]
        a_p = ac[t - ratio] if t - ratio >= 0 else final
        x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
        x = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * e
    got = m.run(ch.to(DEV), num_inference_steps=steps, guidance_scale=gs, noise=nz.to(DEV)).cpu()
    err = float((got - x).abs().max())
    print(f"epsilon DDIM, {steps} steps, CFG {gs}: max abs err vs CPU loop {err:.3e}")
    assert err < 5e-4                         # measured 1.0e-4 (the v-prediction test's bound: 2e-3)


# ------------------------------------------------------------------ 6. fp16
def test_fp16_loss_close_to_fp32(weights, case):
    x0, eps, ch, t, _, _ = case
    pcs = torch.cat([cloud(6, 2048), cloud(7, 2048), cloud(8, 2048)])
    l32 = float(mdit(weights).forward({"cond": ch, "points": pcs}, noise=eps, timesteps=t)["loss"])
    l16 = float(mdit(weights, precision="fp16").forward({"cond": ch, "points": pcs}, noise=eps, timesteps=t)["loss"])
    rel = abs(l16 - l32) / l32
    print(f"fp16 loss {l16:.6f} vs fp32 {l32:.6f}: rel {rel:.2e}")
    assert rel < 2e-3                         # measured 1.4e-5


# ------------------------------------------------------------------ 7. errors
def test_error_paths(weights, case):
    import ctypes as C
    from edgerunner_amd import native
    from edgerunner_amd.models_dit import MDiT
    x0, eps, ch, t, _, _ = case
    m = mdit(weights)
    data = {"cond": ch, "latents": x0}
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m(data, noise=eps, timesteps=t)
    finally:
        m.eval()
    plain = mdit(weights, point_encoder=False)
    with pytest.raises(native.NativeError, match="no point encoder"):
        plain.point_latent(cloud(0, 100).to(DEV))
    with pytest.raises(native.NativeError, match="no point encoder"):
        plain.forward({"cond": ch, "points": cloud(0, 100).repeat(3, 1, 1)}, noise=eps, timesteps=t)
    out = torch.empty((1, 2048, 64), device=DEV)
    pts = cloud(0, 100).to(DEV)
    assert plain.lib.er_dit_point_latent(plain._ctx, native.ptr(pts), 1, 100, native.ptr(out), C.c_void_p(0)) == -5   # UNSUPPORTED
    assert plain.forward(data, noise=eps, timesteps=t)["loss"].isfinite()         # latents need no encoder
    _, _, _, sd_dit = weights
    gap = MDiT(opt_for(), DEV, clip_layers=0, point_encoder=True)
    missing, _ = gap.load_state_dict(sd_dit)
    assert missing and "point_encoder." in missing[0]
    with pytest.raises(native.NativeError, match="point_encoder"):
        gap.forward(data, noise=eps, timesteps=t)
    gap.close()
    for bad in ([0, 1000, 5], [-1, 0, 0]):
        with pytest.raises(ValueError, match=r"\[0, 1000\)"):
            m.forward(data, noise=eps, timesteps=torch.tensor(bad))
    lat, nz, cond = x0.to(DEV), eps.to(DEV), m.get_cond(ch.to(DEV))
    mse, loss = torch.empty(3, device=DEV), torch.empty(1, device=DEV)
    rc = m.lib.er_dit_loss(m._ctx, native.ptr(lat), native.ptr(nz), native.ptr(cond), native.i32_array([0, 1000, 1]), 3, 257, 5.0,
                           None, native.ptr(mse), native.ptr(loss), C.c_void_p(0))
    assert rc == -1 and b"outside [0, 1000)" in m.lib.er_last_error()
    with pytest.raises(ValueError, match="noise must be"):
        m.forward(data, noise=eps[:, :100], timesteps=t)
    with pytest.raises(ValueError, match="latents must be"):
        m.forward({"cond": ch, "latents": x0[:, :, :32]}, noise=eps, timesteps=t)
    with pytest.raises(ValueError, match="timesteps must be"):
        m.forward(data, noise=eps, timesteps=t[:2])
    with pytest.raises(ValueError, match="cond has"):
        m.forward({"cond": ch[:2], "latents": x0}, noise=eps, timesteps=t)


# ------------------------------------------------------------------ 8. score_dit.py end to end
def _write_box(path):
    box = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * 0.5
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    with open(path, "w") as fh:
        for p in box:
            fh.write(f"v {p[0]} {p[1]} {p[2]}\n")
        for q in quads:
            for f in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                fh.write(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}\n")


def test_score_dit_py_end_to_end(weights, tmp_path):
    from PIL import Image
    from safetensors.torch import save_file
    from edgerunner_amd import weights as W
    from edgerunner_amd.models_dit import MDiT
    from edgerunner_amd.options import parse_cli
    from edgerunner_amd.provider import collate_dit, dit_item
    _, sd_lmm, pe, sd_dit = weights
    lmm_ck = {k: v for k, v in sd_lmm.items() if k.startswith(("point_encoder.", "proj_cond.", "norm_cond."))}  # proj/norm: LMM shapes
    dit_ck = dict(sd_dit, **W.make_clip_state_dict(2, 0, "perturbed"))
    save_file({k: v.contiguous() for k, v in lmm_ck.items()}, str(tmp_path / "lmm.safetensors"))
    save_file({k: v.contiguous() for k, v in dit_ck.items()}, str(tmp_path / "mdit.safetensors"))
    pairs = tmp_path / "pairs"
    (pairs / "images").mkdir(parents=True)
    (pairs / "shapes").mkdir()
    rng = np.random.default_rng(3)
    Image.fromarray((rng.random((96, 80, 4)) * 255).astype(np.uint8)).save(pairs / "images" / "box.png")
    np.save(pairs / "images" / "blob.npy", rng.random((64, 64, 3)).astype(np.float32))
    _write_box(str(pairs / "shapes" / "box.obj"))
    np.save(pairs / "shapes" / "blob.npy", (rng.random((1024, 3)) * 1.9 - 0.95).astype(np.float32))
    env = dict(os.environ, EDGERUNNER_PRECISION="fp32", ER_CLIP_LAYERS="2")
    res = {}
    for bs in (1, 2):
        args = ["DiT", "--num_layers", "2", "--dit_num_layers", "2", "--resume", str(tmp_path / "lmm.safetensors"), "--resume2",
                str(tmp_path / "mdit.safetensors"), "--test_path", str(pairs), "--workspace", str(tmp_path / f"out{bs}"),
                "--batch_size", str(bs), "--test_repeat", "2", "--point_num", "1024", "--seed", "7"]
        p = subprocess.run([sys.executable, os.path.join(ROOT, "score_dit.py")] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=900)
        assert p.returncode == 0, p.stdout[-3000:]
        res[bs] = json.load(open(tmp_path / f"out{bs}" / "dit_scores.json"))
    print(p.stdout[-700:])
    r2 = res[2]
    assert [q["name"] for q in r2["pairs"]] == ["blob", "box"] and r2["precision"] == "fp32" and len(r2["pairs"][0]["draws"]) == 2
    worst = 0.0
    for q1, q2 in zip(res[1]["pairs"], r2["pairs"]):
        for d1, d2 in zip(q1["draws"], q2["draws"]):
            assert d1["t"] == d2["t"] and d1["weight"] == d2["weight"]
            worst = max(worst, abs(d1["mse"] - d2["mse"]) / d2["mse"])
    print(f"batch_size 1 vs 2: max rel mse difference {worst:.2e}")
    assert worst < 1e-5
    # the same draws in this process: batches of two jobs = (pair 0, r0), (pair 0, r1), (pair 1, r0), (pair 1, r1)
    sys.path.insert(0, ROOT)
    import score_dit
    opt = parse_cli(args)
    m = MDiT(opt, DEV, clip_layers=2, point_encoder=True)
    m.load_state_dict(dict(dit_ck, **pe), strict=True)
    names = sorted(["blob", "box"])
    files = {"blob": ("images/blob.npy", "shapes/blob.npy"), "box": ("images/box.png", "shapes/box.obj")}
    items = [dit_item(str(pairs / files[n][0]), str(pairs / files[n][1]), opt, rng=np.random.default_rng([7, i]))
             for i, n in enumerate(names)]
    batch_losses = []
    for i in range(2):
        nt = [score_dit.draw(7, i, r, (2048, 64)) for r in range(2)]
        out = m.forward(collate_dit([items[i], items[i]]), noise=torch.cat([n for n, _ in nt]), timesteps=torch.cat([t for _, t in nt]))
        batch_losses.append(float(out["loss"]))
        for r in range(2):
            d = r2["pairs"][i]["draws"][r]
            assert d["t"] == int(out["timesteps"][r]) and d["mse"] == pytest.approx(float(out["mse"][r]), rel=1e-7)
            assert d["loss"] == pytest.approx(float(out["weights"][r]) * float(out["mse"][r]), rel=1e-7)
    assert r2["mean"]["batch_loss"] == pytest.approx(float(np.mean(batch_losses)), rel=1e-7)
    m.close()
