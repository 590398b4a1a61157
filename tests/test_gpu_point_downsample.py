"""The downsample point encoder on the GPU (point_encoder_mode='downsample', core/transformer/point.py:129-169): the farthest point
sampling kernel (csrc/k_fps.h) bit-exact against the restatement (tests/point_downsample_ref.py), the encoder against the committed
golden (the reference's own PointEncoder with the restated sampling) and the live restatement, generation, scoring, MDiT and
infer.py end to end."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_downsample_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAT_TOL = 2e-4          # as the embed encoder's tests (tests/test_gpu_score.py)
LOGIT_TOL = 1e-3
_CACHE = {}


def ds_opt(num_layers=2):
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], num_layers=num_layers, generate_mode="greedy", point_encoder_mode="downsample")


def make_lmm(precision="fp32"):
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    if precision not in _CACHE:
        opt = ds_opt()
        m = LMM(opt, DEV, precision=precision)
        missing, unexpected = m.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        assert not missing and not unexpected
        _CACHE[precision] = m
    return _CACHE[precision]


def cloud(i, n):
    from edgerunner_amd import weights as W
    return W.synthetic_point_cloud(i, n)


def gpu_fps(pts, S):
    from edgerunner_amd import kernels as K
    return K.fps(torch.as_tensor(pts).to(DEV), S).cpu().numpy()


# ------------------------------------------------------------------ 1. the sampling kernel, bit-exact
@pytest.mark.parametrize("N", [8192, 2048, 40000])
def test_fps_indices_bit_equal_to_restatement(N):
    pc = cloud(7, N)                           # N = 40000 takes the large-N form (distances in global scratch)
    got = gpu_fps(pc, 2048)
    want = R.fps(pc.numpy(), 2048)
    assert np.array_equal(got, want), np.nonzero(got != want)


def test_fps_register_and_global_forms_agree():
    pc = cloud(3, 20000)
    got = gpu_fps(pc, 2048)
    assert np.array_equal(got, R.fps(pc.numpy(), 2048))


def test_fps_integer_grid_ties():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pc = torch.from_numpy(g)[None]             # 4096 lattice points: every round has exact distance ties
    got = gpu_fps(pc, 2048)
    want = R.fps(pc.numpy(), 2048)
    assert np.array_equal(got, want)


def test_fps_duplicates_and_degenerate_cloud():
    base = cloud(2, 1024)[0]
    pc = torch.cat([base, base, base[:512], base[:512]])[None]       # every point at least twice
    got = gpu_fps(pc, 2048)
    assert np.array_equal(got, R.fps(pc.numpy(), 2048))
    same = torch.full((1, 2048, 3), 0.25)
    assert np.array_equal(gpu_fps(same, 2048)[0], np.zeros(2048, dtype=np.int32))


def test_fps_batch_rows_equal_single_runs():
    pcs = torch.cat([cloud(i, 4096) for i in range(64)])
    got = gpu_fps(pcs, 2048)
    for b in range(64):
        assert np.array_equal(got[b], gpu_fps(pcs[b:b + 1], 2048)[0]), b
    for b in (0, 63):
        assert np.array_equal(got[b], R.fps(pcs[b].numpy(), 2048)), b


# ------------------------------------------------------------------ 2. the encoder
def test_point_latent_vs_golden_and_restatement():
    from edgerunner_amd import weights as W
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "point_downsample.npz")))
    lmm = make_lmm()
    sd = W.make_state_dict(lmm.opt, 0, "perturbed")
    for k, fp in zip(g["fingerprint_keys"], g["fingerprints"]):
        assert np.allclose(W.fingerprint(sd[str(k)]), fp, rtol=1e-12, atol=0), k
    pc = torch.from_numpy(g["points"])
    assert np.array_equal(gpu_fps(pc, lmm.opt.point_latent_size), g["fps_idx"])
    lat, kl = lmm.mesh_decoder.point_latent(pc.to(DEV))
    lat = lat.cpu()
    err_g = float((lat[:, g["rows"]] - torch.from_numpy(g["latent_rows"])).abs().max())
    ref = R.encoder_downsample(sd, pc, lmm.opt.point_num_heads, g["fps_idx"])
    err_r = float((lat - ref).abs().max())
    kl64 = 0.5 * float((lat.double() ** 2).sum())
    print(f"downsample latent: max abs err vs golden rows {err_g:.3e}, vs live restatement {err_r:.3e}; "
          f"kl {float(kl):.8e} vs {float(g['kl']):.8e}")
    assert err_g <= LAT_TOL and err_r <= LAT_TOL
    assert abs(float(kl) - kl64) <= 1e-6 * kl64


def test_encode_cond_vs_restatement():
    from edgerunner_amd import weights as W
    lmm = make_lmm()
    sd = W.make_state_dict(lmm.opt, 0, "perturbed")
    pcs = torch.cat([cloud(0, 2048), cloud(1, 2048)])
    got = lmm.encode_cond(pcs.to(DEV), [1000, 3000])["cond_embeds"].cpu()
    want = R.encode_cond(sd, lmm.opt, pcs, torch.tensor([1000, 3000]))
    err = float((got - want).abs().max())
    print(f"downsample encode_cond max abs err {err:.3e}")
    assert err <= LAT_TOL


# ------------------------------------------------------------------ 3. generation
def test_greedy_ids_exact_and_batched_rows():
    import arae_oracle as O
    from edgerunner_amd import weights as W
    lmm = make_lmm()
    sd = W.make_state_dict(lmm.opt, 0, "perturbed")
    pc = cloud(0, 4096)
    enc = lambda c, n: R.encode_cond(sd, lmm.opt, c, n)
    want = O.lmm_generate_ids(sd, lmm.opt, pc, 1000, max_new_tokens=48, min_new_tokens=48, encode_fn=enc).numpy()[0]
    _, toks = lmm.generate(pc.to(DEV), 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    assert np.array_equal(toks[0], want), (toks[0][:16], want[:16])
    pcs = torch.cat([cloud(0, 4096), cloud(4, 4096), cloud(0, 4096)]).to(DEV)
    _, tb = lmm.generate(pcs, 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    _, t1 = lmm.generate(pcs[1:2], 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    assert np.array_equal(tb[0], toks[0]) and np.array_equal(tb[2], toks[0]) and np.array_equal(tb[1], t1[0])


def test_fast_mode_vs_storage_rounding_emulation():
    import arae_oracle as O
    from edgerunner_amd import weights as W
    lmm = make_lmm("fp16")
    sd = O.round_streamed_weights(W.make_state_dict(lmm.opt, 0, "perturbed"), torch.float16)
    pc = cloud(0, 4096)
    enc = lambda c, n: R.encode_cond(sd, lmm.opt, c, n)
    want = O.lmm_generate_ids(sd, lmm.opt, pc, 1000, max_new_tokens=48, min_new_tokens=48, encode_fn=enc,
                              fwd=O.make_forward(sd, lmm.opt, kv_round=torch.float16)).numpy()[0]
    _, toks = lmm.generate(pc.to(DEV), 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    assert np.array_equal(toks[0], want), (toks[0][:16], want[:16])


# ------------------------------------------------------------------ 4. scoring
def test_forward_losses_vs_restatement(gold_small):
    import arae_oracle as O
    from edgerunner_amd import weights as W
    from edgerunner_amd.provider import collate_fn
    lmm = make_lmm()
    opt = dataclasses.replace(lmm.opt, max_seq_length=150)
    sd = W.make_state_dict(lmm.opt, 0, "perturbed")
    pc = cloud(0, 2048)
    ids = np.asarray(gold_small["ids_min96"][0], dtype=np.int64)
    items = [{"cond": pc[0].numpy(), "num_faces": 1000, "coords": ids, "len": len(ids), "azimuth": 0, "path": None}]
    data = collate_fn(items, opt)
    out = lmm.forward(data)
    cond = R.encode_cond(sd, lmm.opt, pc, torch.tensor([1000]))
    emb = F.embedding(data["tokens"], sd["mesh_decoder.model.embd.weight"])
    logits, _ = O.decoder_forward(sd, lmm.opt, inputs_embeds=torch.cat((cond, emb), dim=1))
    want_ce = float(F.cross_entropy(logits[0, :-1].double(), data["labels"][0, 1:], ignore_index=-100))
    lat = R.latent(sd, lmm.opt, pc)
    want_kl = 0.5 * float((lat.double() ** 2).sum())
    got_ce, got_kl = float(out["loss_ce"]), float(out["loss_kl"])
    print(f"downsample forward: loss_ce {got_ce:.7f} vs {want_ce:.7f}; loss_kl {got_kl:.6e} vs {want_kl:.6e}")
    assert abs(got_ce - want_ce) <= 1e-4 * want_ce
    assert abs(got_kl - want_kl) <= 1e-4 * want_kl


# ------------------------------------------------------------------ 5. MDiT
def test_mdit_point_latent_equals_lmm_and_forward_runs():
    from edgerunner_amd import weights as W
    from edgerunner_amd.models_dit import MDiT
    from edgerunner_amd.options import config_defaults
    lmm = make_lmm()
    opt = dataclasses.replace(config_defaults["DiT"], dit_num_layers=2, point_encoder_mode="downsample")
    sd = W.make_dit_state_dict(opt, 0, "perturbed")
    sd.update({k: v for k, v in W.make_state_dict(lmm.opt, 0, "perturbed").items() if k.startswith("point_encoder.")})
    m = MDiT(opt, DEV, clip_layers=0, precision="fp32", point_encoder=True)
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    pcs = torch.cat([cloud(0, 2048), cloud(1, 2048)]).to(DEV)
    got = m.point_latent(pcs)
    want, _ = lmm.mesh_decoder.point_latent(pcs)
    assert torch.equal(got, want)
    gen = torch.Generator().manual_seed(0)
    cond = torch.randn((2, 257, 1280), generator=gen)
    out = m.forward({"cond": cond, "points": pcs}, generator=gen)
    assert torch.isfinite(out["loss"]) and out["mse"].shape == (2,)
    m.close()


# ------------------------------------------------------------------ 6. loud errors
def test_errors():
    from edgerunner_amd import native
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    lmm = make_lmm()
    with pytest.raises(ValueError, match="point_latent_size"):
        lmm.encode_cond(cloud(0, 1024).to(DEV), [1000])
    with pytest.raises(ValueError, match="point_latent_size"):
        lmm.mesh_decoder.point_latent(cloud(0, 2047).to(DEV))
    bad = cloud(0, 2048)
    bad[0, 5, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        lmm.mesh_decoder.point_latent(bad.to(DEV))
    opt = ds_opt()
    sd = W.make_state_dict(opt, 0, "perturbed")
    for drop in ("point_encoder.point_embed.mlp.weight", "point_encoder.cross_att.att.q_proj.bias"):
        m = LMM(opt, DEV, precision="fp32")
        with pytest.raises(native.NativeError, match="never loaded"):
            m.mesh_decoder.load_state_dict({k: v for k, v in sd.items() if k != drop}, strict=True)
        m.mesh_decoder.close()
    # query_embed is a stray key in downsample mode (reported as unexpected, not loaded)
    m = LMM(opt, DEV, precision="fp32")
    extra = dict(sd)
    extra["point_encoder.query_embed"] = torch.zeros(1, opt.point_latent_size, opt.point_hidden_dim)
    missing, unexpected = m.mesh_decoder.load_state_dict(extra, strict=False)
    assert unexpected == ["point_encoder.query_embed"] and not missing
    lib = native.load_library()
    assert lib.er_set_point_encoder_mode(m.mesh_decoder._ctx, native.ER_PE_EMBED) == -1   # ER_ERR_INVALID: after loading
    m.mesh_decoder.close()


# ------------------------------------------------------------------ 7. infer.py end to end
def test_infer_py_downsample(tmp_path):
    from safetensors.torch import save_file
    from edgerunner_amd import weights as W
    opt = ds_opt()
    ckpt = str(tmp_path / "arae_ds.safetensors")
    save_file({k: v.contiguous() for k, v in W.make_state_dict(opt, 0, "perturbed").items()}, ckpt)
    box = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * 0.5
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    with open(tmp_path / "box.obj", "w") as fh:
        for p in box:
            fh.write(f"v {p[0]} {p[1]} {p[2]}\n")
        for q in quads:
            for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                fh.write(f"f {t[0] + 1} {t[1] + 1} {t[2] + 1}\n")
    out = tmp_path / "out"
    args = ["ArAE", "--num_layers", "2", "--resume", ckpt, "--test_path", str(tmp_path / "box.obj"), "--workspace", str(out),
            "--point_encoder_mode", "downsample", "--point_num", "2048", "--test_max_seq_length", "64", "--generate_mode", "greedy"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py")] + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    files = os.listdir(out)
    assert any(f.endswith(".ply") for f in files) and any(f.endswith("_tokens.npy") for f in files), files
    p = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py")] + args[:-6] + ["--point_num", "1024"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode != 0 and "point_latent_size" in p.stdout, p.stdout[-2000:]
