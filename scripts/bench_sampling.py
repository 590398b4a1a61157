#!/usr/bin/env python3
"""What the sampling controls and the per-token log-probs cost a decode, one GPU, one process, same build: four variants of
``LMM.generate_ids`` in sample mode on the same cloud(s), alternated, a warm-up run of each first.

    (a) defaults                                   sample_head_kernel, the captured step of every earlier build
    (b) log-probs only                             sample_head_ctl_kernel, serial draw over the top-10
    (c) temperature 0.8, top_k 10, top_p 0.9       ... workgroup-wide nucleus over 10 candidates
    (d) temperature 2.0, top_k 0, top_p 0.99       ... over the whole vocabulary: the widest nucleus

24-layer synthetic checkpoint, ``min_new_tokens = max_new_tokens`` (2000 by default); B = 1 in exact mode (fp32) and B = 32 in fast mode
(fp16).  Records the decode tok/s (``er_last_decode_ms``) of every round, per variant the mean and its ratio to (a)'s mean, and the
spread of (a) against itself ((max - min) / mean over its rounds): a variant whose ratio is inside that spread costs nothing that
this measurement can see.  Prints one JSON object.

    python scripts/bench_sampling.py [--tokens 2000] [--layers 24] [--rounds 3] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgerunner_amd import weights as W  # noqa: E402
from edgerunner_amd.models import LMM  # noqa: E402
from edgerunner_amd.options import config_defaults  # noqa: E402

VARIANTS = {
    "a_defaults": {},
    "b_logprobs": dict(output_logprobs=True),
    "c_t0.8_k10_p0.9": dict(temperature=0.8, top_k=10, top_p=0.9),
    "d_t2.0_k0_p0.99": dict(temperature=2.0, top_k=0, top_p=0.99),
}
WORKLOADS = (("fp32", 1), ("fp16", 32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=2000)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds: at least 3 (the spread of the default variant is the yardstick)")
    T = a.tokens
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=a.layers, generate_mode="sample")
    res = {"layers": a.layers, "tokens": T, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "workloads": {}}
    for precision, B in WORKLOADS:
        lmm = LMM(opt, "cuda:0", precision=precision)
        lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        batch = torch.cat([W.synthetic_point_cloud(i, a.points) for i in range(B)]).to("cuda:0")

        def run(kw):
            ids = lmm.generate_ids(batch, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T, seed=3, **kw)
            torch.cuda.synchronize()
            assert tuple(ids.shape) == (B, T)
            return B * T / lmm.mesh_decoder.last_decode_ms * 1e3

        tok_s = {name: [] for name in VARIANTS}
        for kw in VARIANTS.values():                         # warm-up of each: both step graphs are captured here
            run(kw)
        for _ in range(a.rounds):                            # alternated
            for name, kw in VARIANTS.items():
                tok_s[name].append(round(run(kw), 1))
        mean = {name: sum(v) / len(v) for name, v in tok_s.items()}
        base = tok_s["a_defaults"]
        out = {"batch": B, "tok_s": tok_s, "mean_tok_s": {n: round(m, 1) for n, m in mean.items()},
               "ratio_to_a": {n: round(m / mean["a_defaults"], 4) for n, m in mean.items()},
               "spread_of_a": round((max(base) - min(base)) / mean["a_defaults"], 4)}
        print(f"[{precision} B={B}] {json.dumps(out)}", file=sys.stderr, flush=True)
        res["workloads"][f"{precision}_b{B}"] = out
        lmm.mesh_decoder.close()
        del lmm
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
