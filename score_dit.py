#!/usr/bin/env python3
"""Eval loss of a DiT checkpoint on held-out (image, shape) pairs on MI355X: the reference's eval loop over MDiT
(main_dit.py:216-230, ``model.eval(); out = model(data); total_loss += out['loss']``).

    python score_dit.py DiT --resume lmm.safetensors --resume2 mdit.safetensors --test_path pairs/ --workspace out
                        [--batch_size 4] [--test_repeat K] [--seed S]

Pairs: ``pairs/images/{name}.{png,jpg,npy}`` with ``pairs/shapes/{name}.{obj,ply,npy}`` (a mesh is normalised and surface-sampled
to ``--point_num`` points; a .npy is a ready [N, 3] cloud).  Both checkpoints are loaded tolerantly (strict=False) as main_dit.py:54-88
does; ``point_encoder.*`` may come from either (the LMM checkpoint holds it).  Every pair is scored ``--test_repeat`` times; the noise
and timestep of (pair i, repeat r) come from a CPU generator seeded by (seed, i, r), so they do not depend on ``--batch_size``.
Printed and written to ``{workspace}/dit_scores.json``: per draw t, mse, weight and weighted loss (weight * mse), their means per
pair, the mean over pairs, and ``batch_loss``: the mean over batches of ``out['loss']`` (what main_dit.py logs).
EDGERUNNER_PRECISION=fp32 selects the exact mode (default fp16, like infer_dit.py); ER_CLIP_LAYERS sets the image encoder depth.
"""
from __future__ import annotations

import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from edgerunner_amd.models_dit import MDiT, point_encoder_keys  # noqa: E402
from edgerunner_amd.options import parse_cli  # noqa: E402
from edgerunner_amd.provider import collate_dit, dit_item  # noqa: E402
from edgerunner_amd.utils import seed_everything  # noqa: E402

IMAGE_EXT = (".png", ".jpg", ".npy")
SHAPE_EXT = (".obj", ".ply", ".npy")


def find_pairs(test_path: str):
    """[(name, image path, shape path)] sorted by name; every image needs a shape of the same stem and vice versa."""
    def stems(sub, exts):
        out = {}
        for p in sorted(glob.glob(os.path.join(test_path, sub, "*"))):
            stem, ext = os.path.splitext(os.path.basename(p))
            if ext.lower() in exts:
                if stem in out:
                    raise SystemExit(f"two {sub} files for '{stem}': {out[stem]} and {p}")
                out[stem] = p
        return out
    if not os.path.isdir(os.path.join(test_path, "images")) or not os.path.isdir(os.path.join(test_path, "shapes")):
        raise SystemExit(f"{test_path} must hold images/ and shapes/")
    images, shapes = stems("images", IMAGE_EXT), stems("shapes", SHAPE_EXT)
    lone = sorted(set(images) ^ set(shapes))
    if lone:
        raise SystemExit(f"unmatched pair stems (an image without a shape or a shape without an image): {lone}")
    if not images:
        raise SystemExit(f"no (image, shape) pairs under {test_path}")
    return [(k, images[k], shapes[k]) for k in sorted(images)]


def draw(seed: int, pair: int, repeat: int, shape):
    """The noise [1, *shape] and timestep [1] of draw (pair, repeat): torch.randn then torch.randint(0, 1000), as MDiT.forward draws."""
    g = torch.Generator().manual_seed(int(np.random.SeedSequence([int(seed) & 0xFFFFFFFF, pair, repeat]).generate_state(1, np.uint64)[0] >> 1))
    noise = torch.randn((1,) + tuple(shape), generator=g)
    t = torch.randint(0, 1000, (1,), generator=g)
    return noise, t


def expected_shapes(opt, clip_layers: int):
    """key -> shape of every tensor MDiT(..., point_encoder=True) loads."""
    import dataclasses
    from edgerunner_amd import weights as W
    specs = W.dit_tensor_specs(opt) + (W.clip_tensor_specs(clip_layers) if clip_layers > 0 else [])
    specs += [s for s in W.tensor_specs(W.dims_from_options(dataclasses.replace(opt, cond_mode="point"))) if s[0].startswith("point_encoder.")]
    return {k: tuple(shape) for k, shape, _ in specs}


def tolerant(ckpt, want):
    """main_dit.py:61-70: keep the entries whose key and shape match the model, warn about the rest."""
    out = {}
    for k, v in ckpt.items():
        kk = k if not k.startswith("image_encoder.") or k.startswith("image_encoder.vision_model.") else \
            "image_encoder.vision_model." + k[len("image_encoder."):]
        if kk not in want:
            continue
        if tuple(v.shape) != want[kk]:
            print(f"[WARN] mismatching shape for param {k}: ckpt {tuple(v.shape)} != model {want[kk]}, ignored.")
            continue
        out[k] = v
    return out


def load_ckpt(path):
    if path.endswith("safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu")


def main(argv=None):
    opt = parse_cli(argv)
    seed_everything(opt.seed)
    assert opt.test_path is not None, "--test_path pairs/"
    pairs = find_pairs(opt.test_path)
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible: this path has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    clip_layers = int(os.environ.get("ER_CLIP_LAYERS", "32"))
    model = MDiT(opt, device, clip_layers=clip_layers, precision=None, point_encoder=True)
    pe_keys = point_encoder_keys(opt)
    want = expected_shapes(opt, clip_layers)
    have = set()
    for path in (opt.resume, opt.resume2):
        if path is None:
            continue
        # tolerant load (main_dit.py:54-88): what MDiT holds with matching shapes; an LMM checkpoint contributes its point_encoder.*
        ckpt = tolerant(load_ckpt(path), want)
        model.load_state_dict(ckpt, strict=False)
        have |= set(ckpt) & pe_keys
        print(f"[INFO] Loaded checkpoint from {path}")
    if pe_keys - have:
        raise SystemExit(f"point_encoder weights missing from --resume and --resume2 (e.g. {sorted(pe_keys - have)[0]}): the point "
                         "encoder is frozen and comes from the ArAE / LMM checkpoint (pass it as --resume)")
    if os.environ.get("EDGERUNNER_PRECISION", "fp16") == "fp32":
        model = model.float().eval()
    else:
        model = model.half().eval()
    model.release_checkpoint()
    os.makedirs(opt.workspace, exist_ok=True)

    items = [dit_item(img, shp, opt, rng=np.random.default_rng([int(opt.seed) & 0xFFFFFFFF, i])) for i, (_, img, shp) in enumerate(pairs)]
    jobs = [(i, r) for i in range(len(pairs)) for r in range(max(1, int(opt.test_repeat)))]
    shape = (opt.point_latent_size, opt.point_latent_dim)
    draws = {i: [] for i in range(len(pairs))}
    batch_losses = []
    bs = max(1, int(opt.batch_size))
    for j0 in range(0, len(jobs), bs):
        chunk = jobs[j0:j0 + bs]
        data = collate_dit([items[i] for i, _ in chunk])
        nt = [draw(opt.seed, i, r, shape) for i, r in chunk]
        out = model.forward(data, noise=torch.cat([n for n, _ in nt]), timesteps=torch.cat([t for _, t in nt]))
        mse, w = out["mse"].cpu().tolist(), out["weights"].cpu().tolist()
        batch_losses.append(float(out["loss"]))
        for k, (i, r) in enumerate(chunk):
            draws[i].append({"repeat": r, "t": int(out["timesteps"][k]), "mse": mse[k], "weight": w[k], "loss": w[k] * mse[k]})
    per_pair = []
    for i, (name, img, shp) in enumerate(pairs):
        d = sorted(draws[i], key=lambda x: x["repeat"])
        rec = {"name": name, "image": img, "shape": shp, "draws": d,
               "mean": {k: float(np.mean([x[k] for x in d])) for k in ("mse", "loss")}}
        per_pair.append(rec)
        print(f"[INFO] {name}: " + ", ".join(f"t={x['t']} mse={x['mse']:.6f} w={x['weight']:.5f}" for x in d) +
              f" -> loss {rec['mean']['loss']:.6f}")
    mean = {k: float(np.mean([p["mean"][k] for p in per_pair])) for k in ("mse", "loss")}
    mean["batch_loss"] = float(np.mean(batch_losses))
    print(f"[INFO] mean over {len(per_pair)} pairs: loss {mean['loss']:.6f}, mse {mean['mse']:.6f}; mean of out['loss'] over "
          f"{len(batch_losses)} batches {mean['batch_loss']:.6f}")
    res = {"precision": model.precision, "prediction_type": model.prediction_type, "snr_gamma": opt.snr_gamma, "seed": opt.seed,
           "test_repeat": max(1, int(opt.test_repeat)), "batch_size": bs, "pairs": per_pair, "mean": mean}
    with open(os.path.join(opt.workspace, "dit_scores.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
