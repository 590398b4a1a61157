"""Host side of the DiT eval loss (no GPU): the per-sample weights against a float64 restatement of diffusers' compute_snr, the
pairing and error handling of score_dit.py, and the DiT dataset items / collate."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alphas_cumprod_f64():
    """DDPMScheduler's table (scaled_linear betas 0.00085..0.012, 1000 steps) in float64."""
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas)


def compute_snr_f64(t):
    """diffusers.training_utils.compute_snr, float64: (sqrt(ac) / sqrt(1 - ac))^2."""
    ac = alphas_cumprod_f64()[t]
    return (np.sqrt(ac) / np.sqrt(1.0 - ac)) ** 2


@pytest.mark.parametrize("pred_type", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("gamma", [5.0, 1.0, None])
def test_snr_weight_table_vs_float64(pred_type, gamma):
    from edgerunner_amd.models_dit import dit_loss_coefficients, dit_loss_weights
    t = np.arange(1000)
    sa, sb, w = dit_loss_coefficients(t, pred_type, gamma)
    ac = alphas_cumprod_f64()
    snr = compute_snr_f64(t)
    if gamma is None:
        want = np.ones(1000)
    else:
        m = np.minimum(snr, gamma)                                  # models_dit.py:169
        want = m / snr if pred_type == "epsilon" else m / (snr + 1)   # :170-173
    rel = np.abs(w.double().numpy() - want) / want
    print(f"{pred_type}, gamma {gamma}: max rel err of the fp32 weights vs float64 {rel.max():.2e}")
    # fp32 as diffusers: at t = 0, 1 - ac (~8.5e-4) cancels ~2.5e-5 of relative precision away; elsewhere a few 1e-6
    assert rel.max() < 4e-5 and np.median(rel) < 5e-6
    assert np.abs(sa.double().numpy() / np.sqrt(ac) - 1).max() < 1e-6 and np.abs(sb.double().numpy() / np.sqrt(1 - ac) - 1).max() < 2e-5
    assert torch.equal(dit_loss_weights(t, pred_type, gamma), w)
    assert w.dtype == torch.float32 and tuple(w.shape) == (1000,)


def test_native_table_is_the_reference_schedule():
    """The fp32 table the sampler and loss share follows diffusers' (torch linspace / cumprod) to fp32 round-off."""
    from edgerunner_amd.models_dit import ddim_alphas_cumprod, dit_alphas_cumprod_f32
    a = dit_alphas_cumprod_f32()
    assert np.abs(a.astype(np.float64) / ddim_alphas_cumprod().double().numpy() - 1).max() < 2e-6
    assert np.abs(a.astype(np.float64) / alphas_cumprod_f64() - 1).max() < 1e-5


def test_weights_reject_unknown_prediction_type():
    from edgerunner_amd.models_dit import dit_loss_weights
    with pytest.raises(ValueError):
        dit_loss_weights([0, 1], "sample")


# ------------------------------------------------------------------ score_dit.py: pairs
def _touch(path, data=b""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def _score_dit():
    sys.path.insert(0, ROOT)
    import score_dit
    return score_dit


def test_pairs_match_by_stem(tmp_path):
    sd = _score_dit()
    for p in ("images/b.png", "images/a.npy", "images/notes.txt", "shapes/a.obj", "shapes/b.npy", "shapes/readme.md"):
        _touch(str(tmp_path / p))
    pairs = sd.find_pairs(str(tmp_path))
    assert [(n, os.path.basename(i), os.path.basename(s)) for n, i, s in pairs] == [("a", "a.npy", "a.obj"), ("b", "b.png", "b.npy")]


@pytest.mark.parametrize("files,match", [
    (("images/a.png", "shapes/a.obj", "images/c.jpg"), "unmatched"),
    (("images/a.png", "shapes/a.obj", "shapes/d.ply"), "unmatched"),
    (("images/a.png", "images/a.npy", "shapes/a.obj"), "two images"),
    (("images/x.txt", "shapes/y.txt"), "no \\(image, shape\\) pairs"),
    (("images/a.png",), "must hold images/ and shapes/"),
])
def test_pairing_errors(tmp_path, files, match):
    sd = _score_dit()
    for p in files:
        _touch(str(tmp_path / p))
    with pytest.raises(SystemExit, match=match):
        sd.find_pairs(str(tmp_path))


def test_draws_depend_only_on_seed_pair_and_repeat():
    sd = _score_dit()
    n1, t1 = sd.draw(0, 3, 1, (16, 8))
    n2, t2 = sd.draw(0, 3, 1, (16, 8))
    n3, t3 = sd.draw(0, 3, 2, (16, 8))
    assert torch.equal(n1, n2) and torch.equal(t1, t2) and not torch.equal(n1, n3)
    assert tuple(n1.shape) == (1, 16, 8) and 0 <= int(t1) < 1000


def test_tolerant_load_keeps_matching_shapes_only(capsys):
    from edgerunner_amd.options import config_defaults
    sd = _score_dit()
    opt = dataclasses.replace(config_defaults["DiT"], dit_num_layers=1)
    want = sd.expected_shapes(opt, 0)
    ck = {"proj_cond.weight": torch.zeros(1536, 64), "point_encoder.ln.bias": torch.zeros(1024), "mesh_decoder.lm_head.weight": torch.zeros(2),
          "norm_cond.bias": torch.zeros(1024)}
    kept = sd.tolerant(ck, want)
    assert set(kept) == {"point_encoder.ln.bias", "norm_cond.bias"}
    assert "mismatching shape for param proj_cond.weight" in capsys.readouterr().out


def test_score_dit_main_rejects_a_folder_without_pairs(tmp_path):
    """main() checks the pairs before it looks for a device or loads a checkpoint."""
    sd = _score_dit()
    with pytest.raises(SystemExit, match="must hold images/ and shapes/"):
        sd.main(["DiT", "--test_path", str(tmp_path), "--workspace", str(tmp_path / "out")])


# ------------------------------------------------------------------ dataset items
def _write_box(path):
    box = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * 0.5 + 0.3
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    with open(path, "w") as fh:
        for p in box:
            fh.write(f"v {p[0]} {p[1]} {p[2]}\n")
        for q in quads:
            for f in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                fh.write(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}\n")


def test_dit_item_and_collate_shapes(tmp_path):
    from edgerunner_amd.options import config_defaults
    from edgerunner_amd.provider import collate_dit, dit_item
    opt = dataclasses.replace(config_defaults["DiT"], point_num=300)
    rgba = np.random.default_rng(0).random((40, 30, 4)).astype(np.float32)
    np.save(tmp_path / "img.npy", rgba)
    _write_box(str(tmp_path / "box.obj"))
    cloud = np.random.default_rng(1).random((300, 3)).astype(np.float32) - 0.5
    np.save(tmp_path / "cloud.npy", cloud)
    a = dit_item(str(tmp_path / "img.npy"), str(tmp_path / "box.obj"), opt, np.random.default_rng(5))
    b = dit_item(str(tmp_path / "img.npy"), str(tmp_path / "cloud.npy"), opt)
    assert tuple(a["cond"].shape) == (3, 512, 512) and a["cond"].dtype == torch.float32
    assert 0.0 <= float(a["cond"].min()) and float(a["cond"].max()) <= 1.0
    assert tuple(a["points"].shape) == (300, 3) and float(a["points"].abs().max()) <= 0.95 + 1e-6
    assert float(a["points"].max()) == pytest.approx(0.95, abs=1e-6) or float(-a["points"].min()) == pytest.approx(0.95, abs=1e-6)
    assert torch.equal(b["points"], torch.from_numpy(cloud))              # a .npy cloud is used as it is
    again = dit_item(str(tmp_path / "img.npy"), str(tmp_path / "box.obj"), opt, np.random.default_rng(5))
    assert torch.equal(again["points"], a["points"])
    data = collate_dit([a, b])
    assert tuple(data["cond"].shape) == (2, 3, 512, 512) and tuple(data["points"].shape) == (2, 300, 3)
    assert data["paths"][1] == (str(tmp_path / "img.npy"), str(tmp_path / "cloud.npy"))
    np.save(tmp_path / "small.npy", cloud[:100])
    c = dit_item(str(tmp_path / "img.npy"), str(tmp_path / "small.npy"), opt)
    with pytest.raises(ValueError, match="same shape"):
        collate_dit([a, c])
    np.save(tmp_path / "bad.npy", cloud[:, :2])
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        dit_item(str(tmp_path / "img.npy"), str(tmp_path / "bad.npy"), opt)
