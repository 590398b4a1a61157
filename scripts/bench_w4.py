#!/usr/bin/env python3
"""fp4 mode against fast mode and fp8 mode, same build, same process, same session (GPU box only).

24-layer contexts on the synthetic checkpoint, alternated run by run:
    fp16            fast mode
    fp8             fp8 mode
    fp4             fp4 mode as it ships: the measured launch rule (csrc/er_w4_rule.h w4_streams)
    fp4_rows        fp4 mode under ER_W4_ROWS=1: nibbles in every row form that has one (qkv, fc1, fc2)
  * decode tok/s of a --tokens (2000) token greedy generation at B = 1, 2, 3, 4: median of --runs (3) after one warm-up run each, with
    the spread (max - min) of the runs;
  * the in-situ launch time of qkv / out_proj / fc1 / fc2 from the context's profiler (24 graph-replayed launches of a kind at context
    4050, as scripts/ab_decode.py takes them), --runs sweeps per context, alternated: the nibble form (fp4_rows), the byte
    form (fp8) and the fp16 form.  The spread of the repeated fp16 sweeps is the session's run-to-run noise; a projection streams
    nibbles at B rows (w4_streams) only if its nibble form is below the fp16 form by more than that spread.  out_proj has no nibble
    form: its fp4 columns time the fp16 copy;
  * printed, not judged: max |dlogit| of fp8 and fp4 mode against fast mode over --drift-steps teacher-forced steps of fast mode's own
    greedy path, and the first step at which their greedy ids leave it.  Synthetic weights: this says nothing about a trained checkpoint
    (run score.py under EDGERUNNER_PRECISION=fp4 for that).

    python scripts/bench_w4.py --out profiles/w4_bench.json
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
CONTEXTS = {"fp16": ("fp16", {}), "fp8": ("fp8", {}), "fp4": ("mxfp4", {}), "fp4_rows": ("mxfp4", {"ER_W4_ROWS": "1"})}
NIBBLE_FORMS = ("fp4_rows",)


def make(prec, env, layers):
    """a context of `layers` layers; env: the knobs er_create reads, set for the creation only"""
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=layers, generate_mode="greedy")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        lmm = LMM(opt, "cuda:0", precision=prec)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
    return lmm


def decode(lmm, pc, T):
    _, toks = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    torch.cuda.synchronize()
    return pc.shape[0] * T / lmm.mesh_decoder.last_decode_ms * 1e3, toks


def teacher_forced(lmm, pc, ids):
    dec = lmm.mesh_decoder
    cond = lmm.encode_cond(pc, [1000])["cond_embeds"]
    bos = torch.full((1, 1), lmm.opt.bos_token_id, dtype=torch.long)
    dec.prefill(torch.cat((cond, dec.embd(bos)), dim=1), len(ids) + 2)
    out = []
    for t in range(len(ids)):
        out.append(dec.logits().cpu().numpy()[0].copy())
        if t + 1 < len(ids):
            dec.feed([int(ids[t])])
    return np.stack(out)


def drift_vs_fast(ctx, steps):
    from edgerunner_amd import weights as W
    pc = W.synthetic_point_cloud(0, 4096).to("cuda:0")
    _, toks = ctx["fp16"].generate(pc, 1000, tokenizer=object(), max_new_tokens=steps, min_new_tokens=steps)
    ids = np.asarray(toks[0][:steps])
    ref = teacher_forced(ctx["fp16"], pc, ids)
    out = {"steps": steps, "largest_abs_logit_fp16": float(np.abs(ref).max())}
    for m in ("fp8", "fp4"):
        _, own = ctx[m].generate(pc, 1000, tokenizer=object(), max_new_tokens=steps, min_new_tokens=steps)
        diff = np.nonzero(np.asarray(own[0][:steps]) != ids)[0]
        out[m] = {"max_abs_dlogit_vs_fp16": float(np.abs(teacher_forced(ctx[m], pc, ids) - ref).max()),
                  "first_greedy_divergence": int(diff[0]) if len(diff) else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tokens", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--drift-steps", type=int, default=64)
    a = ap.parse_args()
    from edgerunner_amd import weights as W
    ctx = {name: make(prec, env, a.layers) for name, (prec, env) in CONTEXTS.items()}
    res = {"tokens": a.tokens, "runs": a.runs, "layers": a.layers, "profile_context": 4050, "device": torch.cuda.get_device_name(0),
           "contexts": {name: {"precision": prec, "env": env} for name, (prec, env) in CONTEXTS.items()}, "batches": {}}
    for B in (1, 2, 3, 4):
        pc = torch.cat([W.synthetic_point_cloud(i, 4096) for i in range(B)]).to("cuda:0")
        tok = {m: [] for m in ctx}
        us = {m: {k: [] for k in KINDS} for m in ctx}
        for run in range(a.runs + 1):                      # run 0 warms every context up
            for m, lmm in ctx.items():                     # alternated: fp16, fp8, fp4, ..., fp16, fp8, ...
                rate, _ = decode(lmm, pc, a.tokens)
                prof = lmm.mesh_decoder.profile_decode_kernels(repeats=5, context_len=4050, use_graph=True)
                if run:
                    tok[m].append(rate)
                    for k in KINDS:
                        us[m][k].append(prof[k]["avg_us"])
        med = {m: statistics.median(v) for m, v in tok.items()}
        row = {"decode_tok_s": {m: {"median": round(med[m], 1), "spread": round(max(v) - min(v), 1), "runs": [round(x, 1) for x in v]} for m, v in tok.items()},
               "speedup_vs_fp16": {m: round(med[m] / med["fp16"], 4) for m in ctx if m != "fp16"},
               "streams": {m: ctx[m].mesh_decoder.w4_streams() for m in ctx if m.startswith("fp4")}, "kinds_us": {}}
        for k in KINDS:
            h = us["fp16"][k]
            spread = max(h) - min(h)
            cell = {"fp16_spread": round(spread, 3)}
            for m in ctx:
                cell[m] = round(statistics.median(us[m][k]), 3)
                cell[m + "_runs"] = [round(x, 3) for x in us[m][k]]
            for m in NIBBLE_FORMS:
                cell[m + "_faster_beyond_spread"] = bool(statistics.median(h) - statistics.median(us[m][k]) > spread)
            row["kinds_us"][k] = cell
        res["batches"][str(B)] = row
        print(f"B={B}: {json.dumps(row)}", flush=True)
    res["drift_synthetic_checkpoint"] = drift_vs_fast(ctx, a.drift_steps)
    print("fp8 / fp4 against fast mode (synthetic checkpoint, printed only):", json.dumps(res["drift_synthetic_checkpoint"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": a.out, "speedup_vs_fp16": {b: r["speedup_vs_fp16"] for b, r in res["batches"].items()}}), flush=True)


if __name__ == "__main__":
    main()
