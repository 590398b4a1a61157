#!/usr/bin/env python3
"""fp8 mode against fast mode, same build, same process, same session (GPU box only).

One 24-layer fast-mode (fp16) context and one fp8 context on the synthetic checkpoint, alternated:
  * decode tok/s of a --tokens (2000) token greedy generation at B = 1, 2, 4: median of --runs (3) after one warm-up run each;
  * the in-situ launch time of qkv / out_proj / fc1 / fc2 from the context's profiler (24 graph-replayed launches of a kind at context
    4050, as scripts/ab_decode.py takes them), --runs sweeps per mode, alternated; the spread of the repeated fp16 sweeps is the
    session's run-to-run noise, and a projection keeps its byte-stream form (csrc/er_decode_proj.h w8_streams) only if its fp8 time is
    below its fp16 time by more than that spread;
  * printed, not judged: max |dlogit| of the fp8 context against the committed 24-layer golden path (the reference's fp32 logits,
    teacher-forced) and the first index at which its greedy ids leave that path.  Synthetic weights: says nothing about a trained
    checkpoint (run score.py under EDGERUNNER_PRECISION=fp8 for that).

    python scripts/bench_w8.py --out profiles/w8_bench.json
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ("qkv_gemv", "out_proj_gemv", "fc1_gemv", "fc2_gemv")


def make(prec, layers):
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=layers, generate_mode="greedy")
    lmm = LMM(opt, "cuda:0", precision=prec)
    lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
    return lmm


def decode(lmm, pc, T):
    _, toks = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    torch.cuda.synchronize()
    return pc.shape[0] * T / lmm.mesh_decoder.last_decode_ms * 1e3, toks


def golden_drift(lmm):
    from edgerunner_amd import weights as W
    p = os.path.join(ROOT, "tests", "golden", "arae_long24.npz")
    if not os.path.exists(p):
        return None
    g = dict(np.load(p))
    T, R = int(g["T"][0]), int(g["R"][0])
    resume = torch.as_tensor(W.synthetic_resume_ids(500, R))[None]
    pc = W.synthetic_point_cloud(0, 4096).to("cuda:0")
    _, toks = lmm.generate(pc, 4000, resume_ids=resume, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    ids = np.asarray(toks[0][R:])
    diff = np.nonzero(ids != g["ids"][: len(ids)])[0]
    dec = lmm.mesh_decoder
    cond = lmm.encode_cond(pc, [4000])["cond_embeds"]
    inp = torch.cat((torch.full((1, 1), lmm.opt.bos_token_id, dtype=torch.long), resume), dim=1)
    dec.prefill(torch.cat((cond, dec.embd(inp)), dim=1), T + 2)
    err = 0.0
    for t in range(T):
        err = max(err, float(np.abs(dec.logits().cpu().numpy()[0] - g["logits"][t]).max()))
        if t < T - 1:
            dec.feed([int(g["ids"][t])])
    return {"steps": T, "context": 2050 + R, "max_abs_dlogit_vs_fp32_golden": err, "first_greedy_divergence": int(diff[0]) if len(diff) else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tokens", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--no-golden", action="store_true")
    a = ap.parse_args()
    from edgerunner_amd import weights as W
    ctx = {"fp16": make("fp16", a.layers), "fp8": make("fp8", a.layers)}
    res = {"tokens": a.tokens, "runs": a.runs, "layers": a.layers, "profile_context": 4050, "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in (1, 2, 4):
        pc = torch.cat([W.synthetic_point_cloud(i, 4096) for i in range(B)]).to("cuda:0")
        tok = {m: [] for m in ctx}
        us = {m: {k: [] for k in KINDS} for m in ctx}
        for run in range(a.runs + 1):                      # run 0 warms both contexts up
            for m, lmm in ctx.items():                     # alternated: fp16, fp8, fp16, fp8, ...
                rate, _ = decode(lmm, pc, a.tokens)
                prof = lmm.mesh_decoder.profile_decode_kernels(repeats=5, context_len=4050, use_graph=True)
                if run:
                    tok[m].append(rate)
                    for k in KINDS:
                        us[m][k].append(prof[k]["avg_us"])
        row = {"decode_tok_s": {m: {"median": round(statistics.median(v), 1), "runs": [round(x, 1) for x in v]} for m, v in tok.items()},
               "speedup": round(statistics.median(tok["fp8"]) / statistics.median(tok["fp16"]), 4), "kinds_us": {}}
        for k in KINDS:
            h, q = us["fp16"][k], us["fp8"][k]
            spread = max(h) - min(h)
            row["kinds_us"][k] = {"fp16": round(statistics.median(h), 3), "fp8": round(statistics.median(q), 3), "fp16_spread": round(spread, 3),
                                  "fp16_runs": [round(x, 3) for x in h], "fp8_runs": [round(x, 3) for x in q],
                                  "bytes_faster_beyond_spread": bool(statistics.median(h) - statistics.median(q) > spread)}
        res["batches"][str(B)] = row
        print(f"B={B}: {json.dumps(row)}", flush=True)
    if not a.no_golden:
        res["golden_path_synthetic_checkpoint"] = golden_drift(ctx["fp8"])
        print("fp8 vs the fp32 golden path (synthetic checkpoint, printed only):", json.dumps(res["golden_path_synthetic_checkpoint"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "speedup": {b: r["speedup"] for b, r in res["batches"].items()}}), flush=True)


if __name__ == "__main__":
    main()
