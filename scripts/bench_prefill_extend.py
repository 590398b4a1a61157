#!/usr/bin/env python3
"""The prefill with a past against the full prefill on one GPU, same process.  24-layer synthetic checkpoint, exact (fp32) and fast
(fp16) mode, B = 1 and B = 32 rows of different clouds.  Prints one JSON object (and writes it to --out) with

* ``new_face_count``: everything ``LMM.generate_ids`` does in front of the decode loop, between two HIP events on the caller's stream -
  the full path (``encode_cond``, the BOS embedding, ``prefill`` over num_cond_tokens + 1 positions) against the extend path
  (``embed_num_face``, the BOS embedding, ``prefill_extend`` over n_new = 2 positions behind num_cond_tokens - 1 kept ones), alternated,
  a warm-up of each first;
* ``route_table``: ``prefill_extend`` alone at past_len = num_cond_tokens - 1 and n_new = 2 .. 128 with ER_EXTEND_ATTN=rows and =flash
  alternated - what csrc/er_extend_plan.h's EXTEND_ROWS_MAX_NEW is read from: the largest n_new up to which the rows route is not slower
  in any of the four (mode, batch) columns (tests/test_prefill_extend_cpu.py holds the constant to this table);
* ``parent_full_path``: the full path timed the same way by the same script on another tree's build (``--root DIR --full-only``, run on
  the parent commit in the same session; merged in with ``--baseline FILE``).

    python scripts/bench_prefill_extend.py [--precision fp32 fp16] [--batches 1 32] [--layers 24] [--rounds 5] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

ROUTE_N = (2, 4, 8, 16, 32, 64, 128)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    e0, e1 = events()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1), 3)


def full_path(lmm, conds, num_faces, room):
    opt, dec = lmm.opt, lmm.mesh_decoder
    n = conds.shape[0]
    cond = lmm.encode_cond(conds, [num_faces] * n)["cond_embeds"]
    emb = torch.cat((cond, dec.model.embd(torch.full((n, 1), opt.bos_token_id, dtype=torch.long))), dim=1)
    dec.prefill(emb, room)


def extend_path(lmm, n, num_faces, past, extra_ids=()):
    from edgerunner_amd.utils import quantize_num_faces
    opt, dec = lmm.opt, lmm.mesh_decoder
    face = dec.embed_num_face([quantize_num_faces(num_faces)] * n)[:, None, :]
    toks = torch.tensor([[opt.bos_token_id] + list(extra_ids)] * n, dtype=torch.long)
    dec.prefill_extend(torch.cat((face, dec.model.embd(toks)), dim=1), past)


def summary(ms):
    return {"ms": ms, "ms_min": min(ms), "ms_median": round(statistics.median(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["fp32", "fp16"], choices=["fp16", "fp32"])
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 32])
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--room", type=int, default=192, help="max_new_tokens the cache is reserved for behind the prefill (>= 128 + 2)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package and build are measured")
    ap.add_argument("--full-only", action="store_true", help="time the full path alone (a tree without prefill_extend: the parent commit)")
    ap.add_argument("--baseline", default=None, help="JSON of a --full-only run on the parent commit in the same session")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults

    mode_of = {"fp32": "exact", "fp16": "fast"}
    res = {"layers": a.layers, "points": a.points, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "tree": "parent" if a.full_only else "this",
           "new_face_count": [], "route_table": []}
    for precision in a.precision:
        opt = dataclasses.replace(config_defaults["ArAE"], num_layers=a.layers, generate_mode="greedy")
        lmm = LMM(opt, "cuda:0", precision=precision)
        lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        past = opt.num_cond_tokens - 1
        res["past_len"] = past
        for B in a.batches:
            conds = torch.cat([W.synthetic_point_cloud(c, a.points) for c in range(B)]).to("cuda:0")
            full_path(lmm, conds, 1000, a.room)                     # warm-up: code objects, scratch, the reservation
            if not a.full_only:
                extend_path(lmm, B, 4000, past)
            torch.cuda.synchronize()
            full, ext = [], []
            for _ in range(a.rounds):
                full.append(timed(lambda: full_path(lmm, conds, 4000, a.room)))
                if not a.full_only:
                    ext.append(timed(lambda: extend_path(lmm, B, 1000, past)))
            row = {"mode": mode_of[precision], "batch": B, "n_new": 2, "full": summary(full)}
            if not a.full_only:
                row["extend"] = summary(ext)
                row["full_over_extend"] = round(min(full) / min(ext), 2)
            res["new_face_count"].append(row)
            print(f"[bench_prefill_extend] {row}", file=sys.stderr, flush=True)
            if a.full_only:
                continue
            for n_new in ROUTE_N:
                ids = [7 + (i % 500) for i in range(n_new - 2)]
                t = {"rows": [], "flash": []}
                for r in ("rows", "flash"):                         # warm-up of both routes at this shape
                    os.environ["ER_EXTEND_ATTN"] = r
                    extend_path(lmm, B, 4000, past, ids)
                torch.cuda.synchronize()
                for _ in range(a.rounds):
                    for r in ("rows", "flash"):
                        os.environ["ER_EXTEND_ATTN"] = r
                        t[r].append(timed(lambda: extend_path(lmm, B, 4000, past, ids)))
                os.environ.pop("ER_EXTEND_ATTN", None)
                entry = {"mode": mode_of[precision], "batch": B, "n_new": n_new, "past_len": past, "rows_ms": min(t["rows"]), "flash_ms": min(t["flash"]),
                         "rows_ms_all": t["rows"], "flash_ms_all": t["flash"]}
                res["route_table"].append(entry)
                print(f"[bench_prefill_extend] {entry}", file=sys.stderr, flush=True)
        lmm.mesh_decoder.close()
        del lmm
        torch.cuda.empty_cache()
    if a.baseline:
        base = json.load(open(a.baseline))
        res["parent_full_path"] = [{k: r[k] for k in ("mode", "batch", "full")} for r in base["new_face_count"]]
    if not a.full_only:
        ns = sorted({r["n_new"] for r in res["route_table"]})
        best = 0
        for n in ns:
            if not all(r["rows_ms"] <= r["flash_ms"] for r in res["route_table"] if r["n_new"] == n):
                break
            best = n
        res["rows_route_wins_up_to_n_new"] = best
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
