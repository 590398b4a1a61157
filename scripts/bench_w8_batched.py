#!/usr/bin/env python3
"""fp8 mode against fast mode in the BATCHED decode step, same build, same process, same session (GPU box only).

scripts/bench_w8.py is the single-row counterpart.  For each cache type (fp16, then the e4m3 byte cache of
EDGERUNNER_KV_PRECISION=fp8) one 24-layer fast-mode context and one fp8 context created under ER_W8_BATCHED=1 - bytes in every
matrix-core form, whatever the default rule of the build says - alternated at B = 8, 16, 32:
  * decode tok/s of a --tokens (2000) token greedy generation: median of --runs (3) after one warm-up run each;
  * the in-situ launch time of qkv / out_proj / fc1 / fc2 from the context's profiler (24 graph-replayed launches of a kind at
    context 4050), --runs sweeps per mode, alternated; the spread of the repeated fp16 sweeps is the session's run-to-run noise;
  * which projections the fp8 context streamed as bytes (NativeShapeOPT.w8_streams: at B = 8 out_proj has no matrix-core form).
A (projection, batch) belongs in the default rule (csrc/er_decode_proj.h w8_streams_batched) only where "bytes_faster_beyond_spread"
holds: the fp8 median is below the fp16 median by more than the fp16 spread.  A case that is slower is recorded the same way.

    python scripts/bench_w8_batched.py --out profiles/w8_batched_bench.json
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ("qkv_gemv", "out_proj_gemv", "fc1_gemv", "fc2_gemv")


def make(prec, kv, layers):
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=layers, generate_mode="greedy")
    lmm = LMM(opt, "cuda:0", precision=prec, kv_precision=kv)
    lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
    return lmm


def decode(lmm, pc, T):
    _, toks = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    torch.cuda.synchronize()
    return pc.shape[0] * T / lmm.mesh_decoder.last_decode_ms * 1e3, toks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tokens", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 16, 32])
    a = ap.parse_args()
    from edgerunner_amd import weights as W
    res = {"tokens": a.tokens, "runs": a.runs, "layers": a.layers, "profile_context": 4050, "device": torch.cuda.get_device_name(0),
           "fp8_context": "ER_W8_BATCHED=1", "caches": {}}
    for kv in (None, "fp8"):
        os.environ.pop("ER_W8_BATCHED", None)
        ctx = {"fp16": make("fp16", kv, a.layers)}
        os.environ["ER_W8_BATCHED"] = "1"                  # read by er_create
        ctx["fp8"] = make("fp8", kv, a.layers)
        os.environ.pop("ER_W8_BATCHED", None)
        rows = {}
        for B in a.batches:
            pc = torch.cat([W.synthetic_point_cloud(i, 4096) for i in range(B)]).to("cuda:0")
            tok = {m: [] for m in ctx}
            us = {m: {k: [] for k in KINDS} for m in ctx}
            for run in range(a.runs + 1):                  # run 0 warms both contexts up
                for m, lmm in ctx.items():                 # alternated: fp16, fp8, fp16, fp8, ...
                    rate, _ = decode(lmm, pc, a.tokens)
                    prof = lmm.mesh_decoder.profile_decode_kernels(repeats=5, context_len=4050, use_graph=True)
                    if run:
                        tok[m].append(rate)
                        for k in KINDS:
                            us[m][k].append(prof[k]["avg_us"])
            row = {"decode_tok_s": {m: {"median": round(statistics.median(v), 1), "runs": [round(x, 1) for x in v]} for m, v in tok.items()},
                   "speedup": round(statistics.median(tok["fp8"]) / statistics.median(tok["fp16"]), 4),
                   "w8_streams": ctx["fp8"].mesh_decoder.w8_streams(), "kinds_us": {}}
            for k in KINDS:
                h, q = us["fp16"][k], us["fp8"][k]
                spread = max(h) - min(h)
                row["kinds_us"][k] = {"fp16": round(statistics.median(h), 3), "fp8": round(statistics.median(q), 3), "fp16_spread": round(spread, 3),
                                      "fp16_runs": [round(x, 3) for x in h], "fp8_runs": [round(x, 3) for x in q],
                                      "bytes_faster_beyond_spread": bool(statistics.median(h) - statistics.median(q) > spread)}
            rows[str(B)] = row
            print(f"kv={kv or 'fp16'} B={B}: {json.dumps(row)}", flush=True)
        res["caches"][kv or "fp16"] = rows
        for lmm in ctx.values():
            lmm.mesh_decoder.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "speedup": {c: {b: r["speedup"] for b, r in rows.items()} for c, rows in res["caches"].items()}}), flush=True)


if __name__ == "__main__":
    main()
