#!/usr/bin/env python3
"""Times the device sequence of ``edgerunner_amd.fidelity.fidelity`` (one surface-sampling call, two nearest-neighbour calls, one
metrics call) at N = 8192 points and samples for B = 1 and B = 32 meshes with HIP events, and in the same process the same
quantities from ``torch.cdist(...).min(...)`` per sample (a baseline that shares no code with the kernels).  Prints one JSON line
(committed as profiles/fidelity_bench.json).

    python scripts/bench_fidelity.py [--warmup 5] [--repeats 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgerunner_amd import kernels  # noqa: E402

N = 8192


def sphere(n_lat=32, n_lon=64):
    th, ph = np.linspace(0, np.pi, n_lat + 1), np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    v = 0.9 * np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1)
    f = [t for i in range(n_lat) for j in range(n_lon)
         for p, q in [(i * n_lon + j, i * n_lon + (j + 1) % n_lon)] for t in ([p, p + n_lon, q + n_lon], [p, q + n_lon, q])]
    return v.reshape(-1, 3).astype(np.float32), np.asarray(f, np.int32)


def timed(fn, warmup, repeats):
    """Median / min / max of `repeats` event-timed calls (ms) after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    v, f = sphere()
    out = {"metric": "fidelity_device_sequence_ms", "n_points": N, "n_samples": N, "faces_per_mesh": int(len(f)), "tau": 0.02,
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats}
    for B in (1, 32):
        vd = torch.from_numpy(np.concatenate([v] * B)).to(dev)
        fd = torch.from_numpy(np.concatenate([f] * B)).to(dev)
        voff, foff = [len(v) * i for i in range(B + 1)], [len(f) * i for i in range(B + 1)]
        cloud = kernels.surface_sample(vd, fd, voff, foff, N, seed=1, return_faces=False)
        state = {}

        def sample():
            state["b"] = kernels.surface_sample(vd, fd, voff, foff, N, seed=0, return_faces=False)

        def nn_ab():
            state["ab"] = kernels.nn_dist2(cloud, state["b"], return_idx=False)

        def nn_ba():
            state["ba"] = kernels.nn_dist2(state["b"], cloud, return_idx=False)

        def metrics():
            state["m"] = kernels.fidelity_metrics(state["ab"], state["ba"], 0.02)

        def whole():
            sample(), nn_ab(), nn_ba(), metrics()

        def cdist_one(k):
            d = torch.cdist(cloud[k:k + 1], state["b"][k:k + 1])          # [1, N, N]: 268 MB, one sample at a time
            ab, ba = d.min(2).values.double(), d.min(1).values.double()
            p, r = (ba < 0.02).double().mean(), (ab < 0.02).double().mean()
            return torch.stack([ab.mean() + ba.mean(), (ab * ab).mean() + (ba * ba).mean(), torch.maximum(ab.max(), ba.max()), p, r,
                                2 * p * r / (p + r).clamp_min(1e-300), ab.mean(), ba.mean()])

        def baseline():
            sample()
            state["ref"] = torch.stack([cdist_one(k) for k in range(B)])

        row = {"kernels": timed(whole, args.warmup, args.repeats)}
        for name, fn in (("surface_sample", sample), ("nn_dist2_a2b", nn_ab), ("nn_dist2_b2a", nn_ba), ("metrics", metrics)):
            row[name] = timed(fn, 2, args.repeats)
        # the same call on one point per cloud: what an entry point costs before its kernels do any work (scratch hipMalloc /
        # hipFree, memset, two launches, the stream synchronisation)
        one = cloud[:, :1].contiguous()
        row["nn_dist2_call_floor"] = timed(lambda: kernels.nn_dist2(one, one, return_idx=False), 2, args.repeats)
        for q in (1, 2, 4):                      # queries per lane forced (csrc/k_fidelity.h nn_pick_q); unset = the rule
            os.environ["ER_NN_Q"] = str(q)
            row[f"nn_dist2_a2b_q{q}"] = timed(nn_ab, 2, args.repeats)
        del os.environ["ER_NN_Q"]
        row["cdist_baseline"] = timed(baseline, args.warmup, args.repeats)
        whole()
        baseline()
        # the baseline's distances are sqrt of a matrix-product expansion in fp32: agreement to about 1e-3 absolute, not to the bit
        row["max_abs_diff_vs_baseline"] = float((state["m"] - state["ref"]).abs().max())
        row["speedup"] = row["cdist_baseline"]["median_ms"] / row["kernels"]["median_ms"]
        out[f"B{B}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
