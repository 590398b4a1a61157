#!/usr/bin/env python3
"""Queue mode against the batch path on one GPU: the same jobs of very different lengths served (a) through
``LMM.generate_queue`` from a fixed set of cache rows and (b) through ``LMM.generate`` on consecutive groups of as many rows, each
group run to its longest budget.  24-layer synthetic checkpoint, fp16, 32 slots, 96 jobs by default; ``min_new_tokens`` is the
largest budget, so every job ends exactly at its budget and the useful work is the same on both sides.  Prints one JSON object:
useful tokens / s, row-steps executed, prefill / decode milliseconds for both, and the ratio that row-step arithmetic alone predicts
(steps of the batch path / steps of a greedy list schedule of the same budgets).

    python scripts/bench_queue.py [--jobs 96] [--slots 32] [--layers 24] [--precision fp16] [--scale 1.0] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgerunner_amd import weights as W  # noqa: E402
from edgerunner_amd.models import LMM  # noqa: E402
from edgerunner_amd.options import config_defaults  # noqa: E402
from edgerunner_amd.queue import QueueScheduler  # noqa: E402

# token budgets of the jobs, spread over 500 .. 4000 (fixed, so that two runs serve the same work)
BUDGETS = [
    1477, 717, 3458, 2698, 1938, 1178, 3919, 3159, 2399, 1639, 879, 3620, 2860, 2100, 1340, 580,
    3321, 2561, 1801, 1041, 3782, 3022, 2262, 1502, 742, 3483, 2723, 1963, 1203, 3944, 3184, 2424,
    1664, 904, 3645, 2885, 2125, 1365, 605, 3346, 2586, 1826, 1066, 3807, 3047, 2287, 1527, 767,
    3508, 2748, 1988, 1228, 3969, 3209, 2449, 1689, 929, 3670, 2910, 2150, 1390, 630, 3371, 2611,
    1851, 1091, 3832, 3072, 2312, 1552, 792, 3533, 2773, 2013, 1253, 3994, 3234, 2474, 1714, 954,
    3695, 2935, 2175, 1415, 655, 3396, 2636, 1876, 1116, 3857, 3097, 2337, 1577, 817, 3558, 2798,
]


class _CountingEngine:
    """A greedy list schedule of the budgets on paper: every job runs exactly its budget (queue.QueueScheduler drives it)."""

    def __init__(self, slots, lengths):
        self.lengths, self.left, self.steps = lengths, [None] * slots, 0

    def admit(self, slot0, jobs):
        for i, j in enumerate(jobs):
            self.left[slot0 + i] = self.lengths[j]

    def run(self):
        k = min(v for v in self.left if v is not None)
        self.steps += k
        self.left = [None if v is None else v - k for v in self.left]
        return [s for s, v in enumerate(self.left) if v == 0]

    def take(self, slot):
        self.left[slot] = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=96)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--precision", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every budget (quick runs)")
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    budgets = [max(1, int(BUDGETS[j % len(BUDGETS)] * a.scale)) for j in range(a.jobs)]
    top = max(budgets)
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=a.layers, generate_mode="greedy")
    lmm = LMM(opt, "cuda:0", precision=a.precision)
    lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
    clouds = [W.synthetic_point_cloud(j % 8, a.points).to("cuda:0") for j in range(a.jobs)]
    useful = sum(budgets)

    # ---- (a) the queue
    jobs = [(clouds[j], 1000, None, j, budgets[j]) for j in range(a.jobs)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, q_toks = lmm.generate_queue(jobs, a.slots, tokenizer=object(), max_new_tokens=top, min_new_tokens=top)
    torch.cuda.synchronize()
    q_wall = time.perf_counter() - t0
    st = lmm.last_queue_stats
    assert [len(t) for t in q_toks] == budgets, "every job ends exactly at its budget"

    # ---- (b) the batch path: consecutive groups of `slots` jobs, each group run to its longest budget
    b_wall = b_decode_ms = 0.0
    b_steps = b_row_steps = 0
    same = 0
    for g0 in range(0, a.jobs, a.slots):
        g = list(range(g0, min(g0 + a.slots, a.jobs)))
        T = max(budgets[j] for j in g)
        batch = torch.cat([clouds[j] for j in g])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, toks = lmm.generate(batch, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T, row_streams=g)
        torch.cuda.synchronize()
        b_wall += time.perf_counter() - t0
        b_decode_ms += lmm.mesh_decoder.last_decode_ms
        b_steps += T
        b_row_steps += T * len(g)
        same += sum(int((toks[r][: budgets[j]] == q_toks[j]).all()) for r, j in enumerate(g))

    paper = _CountingEngine(a.slots, budgets)
    QueueScheduler(a.slots).serve(paper, a.jobs)
    res = {
        "precision": a.precision, "layers": a.layers, "slots": a.slots, "jobs": a.jobs, "useful_tokens": useful,
        "budget_min": min(budgets), "budget_max": top,
        "queue": {"wall_s": round(q_wall, 3), "useful_tok_s": round(useful / q_wall, 1), "steps": st["steps"],
                  "row_steps": st["steps"] * a.slots, "occupied_row_steps": st["occupied_row_steps"],
                  "wait_row_steps": st["wait_row_steps"], "parked_row_steps": st["parked_row_steps"], "admissions": st["admissions"],
                  "prefill_ms": round(st["prefill_ms"], 1), "decode_ms": round(st["decode_ms"], 1),
                  "other_ms": round(q_wall * 1e3 - st["prefill_ms"] - st["decode_ms"], 1),
                  "decode_ms_per_step": round(st["decode_ms"] / max(1, st["steps"]), 4)},
        "batch": {"wall_s": round(b_wall, 3), "useful_tok_s": round(useful / b_wall, 1), "steps": b_steps, "row_steps": b_row_steps,
                  "decode_ms": round(b_decode_ms, 1), "encode_prefill_other_ms": round(b_wall * 1e3 - b_decode_ms, 1),
                  "decode_ms_per_step": round(b_decode_ms / max(1, b_steps), 4)},
        "predicted_steps_queue": paper.steps,
        "predicted_ratio_row_steps": round(b_steps / paper.steps, 4),
        "measured_ratio_wall": round(b_wall / q_wall, 4),
        "measured_ratio_decode_ms": round(b_decode_ms / st["decode_ms"], 4),
        "jobs_with_equal_ids": same,
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
