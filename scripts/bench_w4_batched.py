#!/usr/bin/env python3
"""fp4 mode's matrix-core nibble forms against its fp16 forms in the BATCHED decode step, with fast mode and fp8 mode beside them: same
build, same process, same session (GPU box only).

scripts/bench_w4.py is the single-row counterpart, scripts/bench_w8_batched.py the fp8 precedent.  For each cache type (fp16, then the
e4m3 byte cache of EDGERUNNER_KV_PRECISION=fp8) four 24-layer contexts - fast mode, fp8 mode (its default rule), fp4 mode created under
ER_W4_BATCHED=0 (the fp16 tiled copies everywhere) and under ER_W4_BATCHED=1 (nibbles in every matrix-core form, whatever the default
rule of the build says) - alternated at B = 8, 16, 32:
  * decode tok/s of a --tokens (2000) token greedy generation: median of --runs (3) after one warm-up run each;
  * the in-situ launch time of qkv / out_proj / fc1 / fc2 from the context's profiler (24 graph-replayed launches of a kind at
    context 4050), --runs sweeps per mode, alternated; the spread of the repeated ER_W4_BATCHED=0 sweeps is the session's run-to-run noise;
  * which projections the =1 context streamed as nibbles (NativeShapeOPT.w4_streams_batched: at B = 8 out_proj has no matrix-core form).
A (projection, batch) belongs in the default rule (csrc/er_w4_rule.h w4_streams_batched) only where "nibbles_faster_beyond_spread" holds:
the =1 median is below the =0 median by more than the =0 spread.  A case that is slower is recorded the same way.  The file is rewritten
after every cache type, so a run that is cut short leaves what it measured.

    python scripts/bench_w4_batched.py --out profiles/w4_batched_bench.json
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
MODES = (("fp16", "fp16", None), ("fp8", "fp8", None), ("fp4_fp16_copies", "mxfp4", "0"), ("fp4_nibbles", "mxfp4", "1"))


def make(prec, kv, layers, knob):
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=layers, generate_mode="greedy")
    os.environ.pop("ER_W4_BATCHED", None)
    if knob is not None:
        os.environ["ER_W4_BATCHED"] = knob                 # read by er_create
    try:
        lmm = LMM(opt, "cuda:0", precision=prec, kv_precision=kv)
    finally:
        os.environ.pop("ER_W4_BATCHED", None)
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
           "modes": {name: (f"precision {prec}" + (f", ER_W4_BATCHED={knob}" if knob else "")) for name, prec, knob in MODES}, "caches": {}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for kv in (None, "fp8"):
        ctx = {name: make(prec, kv, a.layers, knob) for name, prec, knob in MODES}
        rows = {}
        for B in a.batches:
            pc = torch.cat([W.synthetic_point_cloud(i, 4096) for i in range(B)]).to("cuda:0")
            tok = {m: [] for m in ctx}
            us = {m: {k: [] for k in KINDS} for m in ctx}
            for run in range(a.runs + 1):                  # run 0 warms every context up
                for m, lmm in ctx.items():                 # alternated: fp16, fp8, fp4 (=0), fp4 (=1), fp16, ...
                    rate, _ = decode(lmm, pc, a.tokens)
                    prof = lmm.mesh_decoder.profile_decode_kernels(repeats=5, context_len=4050, use_graph=True)
                    if run:
                        tok[m].append(rate)
                        for k in KINDS:
                            us[m][k].append(prof[k]["avg_us"])
            med = {m: statistics.median(v) for m, v in tok.items()}
            row = {"decode_tok_s": {m: {"median": round(med[m], 1), "runs": [round(x, 1) for x in v]} for m, v in tok.items()},
                   "nibbles_over_fp16_copies": round(med["fp4_nibbles"] / med["fp4_fp16_copies"], 4),
                   "nibbles_over_fp8": round(med["fp4_nibbles"] / med["fp8"], 4),
                   "w4_streams_batched": ctx["fp4_nibbles"].mesh_decoder.w4_streams_batched(),
                   "w8_streams": ctx["fp8"].mesh_decoder.w8_streams(), "kinds_us": {}}
            for k in KINDS:
                h, q = us["fp4_fp16_copies"][k], us["fp4_nibbles"][k]
                spread = max(h) - min(h)
                row["kinds_us"][k] = {"fp4_fp16_copies": round(statistics.median(h), 3), "fp4_nibbles": round(statistics.median(q), 3),
                                      "fp16": round(statistics.median(us["fp16"][k]), 3), "fp8": round(statistics.median(us["fp8"][k]), 3),
                                      "fp4_fp16_copies_spread": round(spread, 3),
                                      "fp4_fp16_copies_runs": [round(x, 3) for x in h], "fp4_nibbles_runs": [round(x, 3) for x in q],
                                      "fp16_runs": [round(x, 3) for x in us["fp16"][k]], "fp8_runs": [round(x, 3) for x in us["fp8"][k]],
                                      "nibbles_faster_beyond_spread": bool(statistics.median(h) - statistics.median(q) > spread)}
            rows[str(B)] = row
            print(f"kv={kv or 'fp16'} B={B}: {json.dumps(row)}", flush=True)
        res["caches"][kv or "fp16"] = rows
        for lmm in ctx.values():
            lmm.mesh_decoder.close()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({"out": a.out, "nibbles_over_fp16_copies": {c: {b: r["nibbles_over_fp16_copies"] for b, r in rows.items()} for c, rows in res["caches"].items()},
                      "nibbles_over_fp8": {c: {b: r["nibbles_over_fp8"] for b, r in rows.items()} for c, rows in res["caches"].items()}}), flush=True)


if __name__ == "__main__":
    main()
