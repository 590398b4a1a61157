#!/usr/bin/env python3
"""kv8 mode (e4m3 byte KV cache) against fast mode, same build, same process, same session (GPU box only).

One 24-layer fast-mode (fp16 weights, fp16 cache) context and one kv8 context (fp16 weights, byte cache) on the synthetic checkpoint,
alternated:
  * decode tok/s of a --tokens (2000) token greedy generation at B = 1, 4, 8, 16, 32: median of --runs (3) after one warm-up run each;
  * the in-situ launch time of the attention launch and the merge launch (where the plan has one) from the context's profiler (24
    graph-replayed launches of a kind at context 4050, as scripts/ab_decode.py takes them), --runs sweeps per mode, alternated; the
    spread of the repeated fp16 runs is the session's run-to-run noise;
  * which attention kernel each context's plan runs at that batch (kv8 gives up version 3 at B = 1 and the round-1 split kernel at
    5 <= B < 16: the table says where that makes it slower);
  * printed, not judged: max |dlogit| of the kv8 context against the committed 24-layer golden path (the reference's fp32 logits,
    teacher-forced) and the first index at which its greedy ids leave that path, next to fast mode's.  Synthetic weights: they say
    nothing about a trained checkpoint (run score.py under EDGERUNNER_KV_PRECISION=fp8 for that).

    python scripts/bench_kv8.py --out profiles/kv8_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_w8 import decode, golden_drift  # noqa: E402

KINDS = ("attn_decode", "attn_combine")
ATTN_NAMES = {1: "split1", 2: "split2", 3: "balanced (version 3)", 4: "stream", 5: "shared"}


def make(kv, layers):
    import dataclasses
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=layers, generate_mode="greedy")
    lmm = LMM(opt, "cuda:0", precision="fp16", kv_precision=kv)
    lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
    return lmm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tokens", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8, 16, 32])
    ap.add_argument("--no-golden", action="store_true")
    a = ap.parse_args()
    from edgerunner_amd import weights as W
    ctx = {"fp16": make(None, a.layers), "kv8": make("fp8", a.layers)}
    res = {"tokens": a.tokens, "runs": a.runs, "layers": a.layers, "profile_context": 4050, "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in a.batches:
        pc = torch.cat([W.synthetic_point_cloud(i, 4096) for i in range(B)]).to("cuda:0")
        tok = {m: [] for m in ctx}
        us = {m: {k: [] for k in KINDS} for m in ctx}
        plans = {}
        for run in range(a.runs + 1):                      # run 0 warms both contexts up
            for m, lmm in ctx.items():                     # alternated: fp16, kv8, fp16, kv8, ...
                rate, _ = decode(lmm, pc, a.tokens)
                prof = lmm.mesh_decoder.profile_decode_kernels(repeats=5, context_len=4050, use_graph=True)
                plans[m] = lmm.mesh_decoder.plan()
                if run:
                    tok[m].append(rate)
                    for k in KINDS:
                        us[m][k].append(prof[k]["avg_us"])
        h, q = tok["fp16"], tok["kv8"]
        row = {"attn_kernel": {m: ATTN_NAMES[p["attn_kernel"]] for m, p in plans.items()},
               "decode_tok_s": {m: {"median": round(statistics.median(v), 1), "runs": [round(x, 1) for x in v]} for m, v in tok.items()},
               "speedup": round(statistics.median(q) / statistics.median(h), 4),
               "fp16_spread_tok_s": round(max(h) - min(h), 1),
               "kv8_slower_beyond_spread": bool(statistics.median(h) - statistics.median(q) > max(h) - min(h)),
               "kinds_us": {}}
        for k in KINDS:
            hh, qq = us["fp16"][k], us["kv8"][k]
            row["kinds_us"][k] = {"fp16": round(statistics.median(hh), 3), "kv8": round(statistics.median(qq), 3),
                                  "fp16_spread": round(max(hh) - min(hh), 3),
                                  "fp16_runs": [round(x, 3) for x in hh], "kv8_runs": [round(x, 3) for x in qq]}
        res["batches"][str(B)] = row
        print(f"B={B}: {json.dumps(row)}", flush=True)
    if not a.no_golden:
        res["golden_path_synthetic_checkpoint"] = {m: golden_drift(lmm) for m, lmm in ctx.items()}
        print("against the fp32 golden path (synthetic checkpoint, printed only):", json.dumps(res["golden_path_synthetic_checkpoint"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "speedup": {b: r["speedup"] for b, r in res["batches"].items()}}), flush=True)


if __name__ == "__main__":
    main()
