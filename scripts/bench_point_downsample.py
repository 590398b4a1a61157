#!/usr/bin/env python3
"""Timings of the downsample point encoder (point_encoder_mode='downsample'): the farthest point sampling kernel (csrc/k_fps.h) at
B in {1, 8, 32, 256} clouds x N in {4096, 8192, 32768} points (2048 samples each), and LMM.encode_cond with the embed and the
downsample encoder at B = 1 / 8, N = 8192.  One JSON line per measurement (median of --reps timed calls after --warmup calls,
device time from HIP events); also written to --out when given.

    python scripts/bench_point_downsample.py [--reps 5] [--warmup 2] [--out point_downsample_bench.jsonl] [--quick]

--quick: only B = 8, N = 8192 (the profiled shape: rocprofv3 --kernel-trace --stats -- python <this> --quick --reps 1 --warmup 1).
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def time_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    from edgerunner_amd import kernels as K
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    S = 2048
    for N in ((8192,) if args.quick else (4096, 8192, 32768)):
        base = torch.cat([W.synthetic_point_cloud(i, N) for i in range(8)]).to(DEV)
        for B in ((8,) if args.quick else (1, 8, 32, 256)):
            pts = base.repeat((B + 7) // 8, 1, 1)[:B].contiguous()
            med, best = time_ms(lambda: K.fps(pts, S), args.reps, args.warmup)
            emit({"what": "fps", "B": B, "N": N, "samples": S, "form": "register" if N <= 16384 else "global",
                  "ms": round(med, 4), "ms_min": round(best, 4), "us_per_round": round(1000 * med / (S - 1), 4)})
        del base
    N = 8192
    for mode in ("embed", "downsample"):
        opt = dataclasses.replace(config_defaults["ArAE"], num_layers=1, point_encoder_mode=mode)
        lmm = LMM(opt, DEV, precision="fp32")
        lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        for B in ((8,) if args.quick else (1, 8)):
            pts = torch.cat([W.synthetic_point_cloud(i, N) for i in range(B)]).to(DEV)
            med, best = time_ms(lambda: lmm.encode_cond(pts, [1000] * B), args.reps, args.warmup)
            emit({"what": "encode_cond", "mode": mode, "B": B, "N": N, "ms": round(med, 3), "ms_min": round(best, 3)})
        lmm.mesh_decoder.close()
        del lmm
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
