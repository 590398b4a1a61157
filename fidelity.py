#!/usr/bin/env python3
"""Reconstruction fidelity of an ``infer.py`` workspace on MI355X: how close every generated mesh is to the cloud it was
conditioned on, and which candidate of an input is the closest.

    python fidelity.py --workspace out [--samples N] [--tau T] [--seed S] [--copy_best]

Needs no checkpoint and no model.  Every ``{name}_pc.obj`` of the workspace is an input; its candidates are the
``{name}_{i}[_{n}f].ply`` files infer.py wrote for it (``edgerunner_amd.fidelity.pair_workspace``).  Each candidate is surface-sampled
(``--samples`` points, default: as many as the cloud has) and compared with the cloud by nearest-neighbour distances in both
directions, up to ER_INFER_BATCH (default 32) meshes per device call.  Written: ``{workspace}/fidelity.json`` - per output file
chamfer_l1, chamfer_l2, hausdorff, precision, recall, fscore (at ``--tau``, default 0.02 = 1 % of the normalised cube's edge),
mean_a2b (cloud -> mesh) and mean_b2a (mesh -> cloud), or null for a file without faces or area and for a file that cannot be
measured (unreadable, non-finite or out-of-range coordinates, a face index outside the mesh: the reason is kept under "errors" and
the other files are still ranked); per input the candidate with the lowest chamfer_l1.  ``--copy_best`` also writes that
candidate as ``{name}_best.ply``.  The samples of a file come from the Philox stream (--seed, index of the file in the sorted
listing), so a result does not depend on ER_INFER_BATCH.  No CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from edgerunner_amd import meshio  # noqa: E402
from edgerunner_amd.fidelity import fidelity, mesh_arrays, pair_workspace  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workspace", required=True)
    ap.add_argument("--samples", type=int, default=None, help="surface samples per mesh (default: the cloud's point count)")
    ap.add_argument("--tau", type=float, default=0.02, help="F-score distance threshold")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--copy_best", action="store_true", help="write the best candidate of every input as {name}_best.ply")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible: this path has no CPU fallback")
    torch.cuda.set_device(0)
    ws = args.workspace
    pairs = pair_workspace(sorted(os.listdir(ws)))
    if not pairs:
        raise SystemExit(f"no *_pc.obj under {ws}: run infer.py with --workspace {ws} first")
    jobs = [(name, f) for name, files in pairs.items() for f in files]          # global order: the Philox stream of a file
    clouds = {name: meshio.load_obj(os.path.join(ws, name + "_pc.obj"))[0].astype(np.float32) for name in pairs}
    cap = max(1, int(os.environ.get("ER_INFER_BATCH", "32")))
    results, errors = {}, {}
    by_size = {}
    for j, (name, _) in enumerate(jobs):
        by_size.setdefault(clouds[name].shape[0], []).append(j)                  # one call holds clouds of one size
    for n_points, js in sorted(by_size.items()):
        for k in range(0, len(js), cap):
            chunk = js[k:k + cap]
            meshes = []
            for j in chunk:                       # one bad candidate is recorded, it does not stop the ranking of the others
                try:
                    meshes.append(mesh_arrays(meshio.load_mesh(os.path.join(ws, jobs[j][1])), jobs[j][1]))
                except Exception as e:  # noqa: BLE001  (a truncated or foreign .ply fails in the reader in many ways)
                    meshes.append(None)
                    errors[jobs[j][1]] = f"{type(e).__name__}: {e}"
                    print(f"[WARN] {jobs[j][1]} left out: {errors[jobs[j][1]]}")
            cond = np.stack([clouds[jobs[j][0]] for j in chunk])
            res = fidelity(cond, meshes, n_samples=args.samples, tau=args.tau, seed=args.seed, streams=chunk)
            for j, r in zip(chunk, res):
                results[jobs[j][1]] = r
                print(f"[INFO] {jobs[j][1]}: " + ("no surface" if r is None else
                                                   f"chamfer_l1 = {r['chamfer_l1']:.6f}, hausdorff = {r['hausdorff']:.6f}, "
                                                   f"fscore = {r['fscore']:.4f}"))
    inputs = {}
    for name, files in pairs.items():
        scored = [f for f in files if results[f] is not None]
        best = min(scored, key=lambda f: (results[f]["chamfer_l1"], f)) if scored else None
        inputs[name] = {"points": int(clouds[name].shape[0]), "candidates": files, "best": best}
        if best is not None:
            print(f"[INFO] {name}: best of {len(files)} = {best}")
            if args.copy_best:
                shutil.copyfile(os.path.join(ws, best), os.path.join(ws, f"{name}_best.ply"))
    with open(os.path.join(ws, "fidelity.json"), "w") as fh:
        json.dump({"tau": args.tau, "seed": args.seed, "samples": args.samples, "files": results, "errors": errors, "inputs": inputs},
                  fh, indent=1)


if __name__ == "__main__":
    main()
