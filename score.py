#!/usr/bin/env python3
"""Teacher-forced scoring of meshes under an ArAE checkpoint on MI355X: the reference's ``eval_mode='loss'`` loop
(main.py:244-268, ``model.eval(); out = model(data)``) over a folder of meshes, one dataset item per file.

    python score.py ArAE --resume model.safetensors --test_path meshes/ --workspace out [--batch_size 4]

Same ``Options`` flags as infer.py.  Each mesh is normalised, surface-sampled and tokenised as infer.py / the reference's
dataset do (``edgerunner_amd.provider.mesh_item``), padded into batches of ``--batch_size`` by ``provider.collate_fn`` and scored by
``LMM.forward``.  Printed per mesh: loss_ce (mean NLL of the next token over its supervised positions), perplexity
exp(loss_ce) and next-token accuracy (argmax == label) over the same positions; then the means over meshes (and
``loss_ce_tokens``, the mean over all supervised positions: LMM.forward's loss_ce when everything fits one batch).  Written:
``{workspace}/scores.json``.  EDGERUNNER_PRECISION=fp32 selects the exact mode, fp8 the e4m3 row-scaled mode, fp4 the MXFP4 block-scaled mode (default fp16, like infer.py).  No CPU fallback.
"""
from __future__ import annotations

import glob
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from edgerunner_amd.meto import get_tokenizer  # noqa: E402
from edgerunner_amd.models import LMM  # noqa: E402
from edgerunner_amd.options import parse_cli  # noqa: E402
from edgerunner_amd.provider import collate_fn, mesh_item  # noqa: E402
from edgerunner_amd.utils import seed_everything  # noqa: E402


def main(argv=None):
    opt = parse_cli(argv)
    seed_everything(opt.seed)
    if opt.cond_mode not in ("point", "none"):
        raise SystemExit("score.py serves cond_mode='point' (ArAE preset) and 'none'")
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible: this path has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    # EDGERUNNER_KV_PRECISION=fp8: the KV cache as e4m3 bytes - what that costs THIS checkpoint, against the fp16 run's loss
    model = LMM(opt, device, precision=None, kv_precision=os.environ.get("EDGERUNNER_KV_PRECISION") or None)
    if opt.resume is not None:
        if opt.resume.endswith("safetensors"):
            from safetensors.torch import load_file
            ckpt = load_file(opt.resume, device="cpu")
        else:
            ckpt = torch.load(opt.resume, map_location="cpu")
        model.load_state_dict(ckpt, strict=False)
        print(f"[INFO] Loaded checkpoint from {opt.resume}")
    else:
        from edgerunner_amd import weights as W
        print("[WARN] model randomly initialized, are you sane?")
        model.load_state_dict(W.make_state_dict(opt, opt.seed, "reference"), strict=True)
    if os.environ.get("EDGERUNNER_PRECISION", "fp16") == "fp32":
        model = model.float().eval().to(device)
    elif os.environ.get("EDGERUNNER_PRECISION") == "fp8":      # what e4m3 rows cost THIS checkpoint: compare the loss with the fp16 run's
        model = model.fp8().eval().to(device)
    elif os.environ.get("EDGERUNNER_PRECISION") in ("fp4", "mxfp4"):      # what MXFP4 blocks cost THIS checkpoint: compare the loss with the fp16 run's
        model = model.fp4().eval().to(device)
    else:
        model = model.half().eval().to(device)
    model.release_checkpoint()
    ckpt = None

    tokenizer, _ = get_tokenizer(opt)
    assert opt.test_path is not None
    paths = sorted(glob.glob(os.path.join(opt.test_path, "*"))) if os.path.isdir(opt.test_path) else [opt.test_path]
    paths = [p for p in paths if p.lower().endswith((".obj", ".ply"))]
    if not paths:
        raise SystemExit(f"no .obj / .ply mesh under {opt.test_path}")
    os.makedirs(opt.workspace, exist_ok=True)
    bs = max(1, int(opt.batch_size))
    per_mesh = []
    tok_sum, tok_n = 0.0, 0            # loss_ce of every batch (LMM.forward's value) weighted by its supervised positions
    for i in range(0, len(paths), bs):
        items = [mesh_item(p, opt, tokenizer) for p in paths[i:i + bs]]
        data = collate_fn(items, opt)
        out = model.score(data)
        labels = data["labels"]
        nll = out["nll"].cpu().double()
        pred = out["pred"].cpu().long()
        n_batch = int((labels[:, 1:] != -100).sum())
        tok_sum += float(out["loss_ce"]) * n_batch
        tok_n += n_batch
        for r, item in enumerate(items):
            # position s predicts labels[s + 1]: the supervised targets are the labels that are not -100, shifted by one
            target = labels[r, 1:]
            sup = target != -100
            n = int(sup.sum())
            loss = float(nll[r, :-1][sup].sum() / n) if n else float("nan")
            acc = float((pred[r, :-1][sup] == target[sup]).double().mean()) if n else float("nan")
            rec = {"path": item["path"], "num_faces": item["num_faces"], "tokens": item["len"], "supervised": n,
                   "loss_ce": loss, "perplexity": math.exp(loss) if n else float("nan"), "accuracy": acc}
            per_mesh.append(rec)
            print(f"[INFO] {os.path.basename(item['path'])}: {item['num_faces']} faces, {n} supervised tokens, "
                  f"loss_ce = {loss:.6f}, ppl = {rec['perplexity']:.4f}, acc = {acc:.4f}")
    mean = {k: float(np.mean([m[k] for m in per_mesh])) for k in ("loss_ce", "perplexity", "accuracy")}
    # over all supervised positions of all meshes (with one batch: exactly LMM.forward's loss_ce of that batch)
    mean["loss_ce_tokens"] = tok_sum / tok_n if tok_n else float("nan")
    print(f"[INFO] mean over {len(per_mesh)} meshes: loss_ce = {mean['loss_ce']:.6f}, ppl = {mean['perplexity']:.4f}, "
          f"acc = {mean['accuracy']:.4f}")
    with open(os.path.join(opt.workspace, "scores.json"), "w") as f:
        json.dump({"precision": model.precision, "kv_precision": model.kv_precision, "meshes": per_mesh, "mean": mean}, f, indent=1)


if __name__ == "__main__":
    main()
