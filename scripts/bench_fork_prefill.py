#!/usr/bin/env python3
"""The forked prefill against the plain one on one GPU, same build, same process.  24-layer synthetic checkpoint, 32 rows, exact
(fp32) and fast (fp16) mode, three batches: 32 rows of ONE cloud (what ``infer.py`` runs for ``--test_repeat 32``), 8 clouds x 4 rows,
and 32 different clouds - singletons, i.e. what the switch costs when nothing repeats.  Prints one JSON object with

* ``encode_prefill_ms``: everything ``LMM.generate_ids`` does in front of the decode loop (``fork_plan`` when on, ``encode_cond``,
  the BOS embedding, ``prefill`` / ``prefill_fork``) between two HIP events on the caller's stream, ``fork_prefill`` off and on
  alternated, a warm-up of each first;
* ``fork_launch``: ``er_k_kv_fork`` alone on caches of the model's shape (24 layers, 32 rows, 16 heads, head_dim 96; 4-, 2- and 1-byte
  elements) between two HIP events, with the bytes it reads (one slab set per source) and writes (one per destination) and the TB/s
  they make;
* ``queue``: a job list with three repeats per cloud served through ``LMM.generate_queue`` with ``fork_repeats`` off and on
  (``er_queue_stats.prefill_ms`` and the rows admitted by copy).  The three repeats of a cloud share a budget, so they leave their
  slots together and the next three are admitted together; budgets differ between clouds (scripts/bench_queue.py's list, scaled).

    python scripts/bench_fork_prefill.py [--precision fp32 fp16] [--rows 32] [--layers 24] [--rounds 3] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgerunner_amd import kernels  # noqa: E402
from edgerunner_amd import weights as W  # noqa: E402
from edgerunner_amd.models import LMM, fork_plan  # noqa: E402
from edgerunner_amd.options import config_defaults  # noqa: E402

QUEUE_BUDGETS = [1477, 717, 3458, 2698, 1938, 1178, 3919, 3159, 2399, 1639, 879, 3620, 2860, 2100, 1340, 580]   # one per cloud (bench_queue.py's first 16)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def encode_prefill(lmm, conds, fork, room):
    """What generate_ids runs in front of the decode loop; ``room`` = the max_new_tokens the cache is reserved for."""
    opt, dec = lmm.opt, lmm.mesh_decoder
    leader = None
    if fork:
        order, leader, n_leaders = fork_plan(conds)
        if n_leaders < conds.shape[0]:
            conds = conds[torch.as_tensor(order[:n_leaders], device=conds.device)]
        else:
            leader = None
    n = conds.shape[0]
    cond = lmm.encode_cond(conds, [1000] * n)["cond_embeds"]
    emb = torch.cat((cond, dec.model.embd(torch.full((n, 1), opt.bos_token_id, dtype=torch.long))), dim=1)
    if leader is None:
        dec.prefill(emb, room)
    else:
        dec.prefill_fork(emb, leader, room)
    return emb.shape[1]


def time_encode_prefill(lmm, conds, rounds, room):
    out = {"off": [], "on": []}
    for fork in (False, True):
        encode_prefill(lmm, conds, fork, room)          # warm-up: code objects, scratch, the reservation
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fork in (("off", False), ("on", True)):
            e0, e1 = events()
            e0.record()
            encode_prefill(lmm, conds, fork, room)
            e1.record()
            torch.cuda.synchronize()
            out[name].append(round(e0.elapsed_time(e1), 3))
    return {"off_ms": out["off"], "on_ms": out["on"], "off_ms_min": min(out["off"]), "on_ms_min": min(out["on"])}


def time_fork_launch(layers, rows, heads, l_cap, head_dim, length, classes, reps):
    res = {}
    for esz, dtype in ((4, torch.float32), (2, torch.float16), (1, torch.uint8)):
        k = torch.zeros((layers, rows, heads, l_cap, head_dim), dtype=dtype, device="cuda:0")
        v = torch.zeros_like(k)
        for name, cls in classes.items():
            order, leader, n_leaders = fork_plan(torch.as_tensor(cls, dtype=torch.float32)[:, None])
            src, dst = [leader[i] for i in range(n_leaders, rows)], list(range(n_leaders, rows))
            if not dst:
                continue
            slab_set = 2 * layers * heads * length * head_dim * esz          # K and V [0, length) of one row, every layer and head
            moved = slab_set * (len(set(src)) + len(dst))
            for _ in range(2):
                kernels.kv_fork(k, v, src, dst, length)
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                e0, e1 = events()
                e0.record()
                kernels.kv_fork(k, v, src, dst, length)
                e1.record()
                torch.cuda.synchronize()
                ms.append(round(e0.elapsed_time(e1), 4))
            best = min(ms)
            res[f"{name}_esz{esz}"] = {"sources": len(set(src)), "destinations": len(dst), "len": length, "bytes_read": slab_set * len(set(src)),
                                       "bytes_written": slab_set * len(dst), "ms": ms, "ms_min": best,
                                       "TB_per_s": round(moved / (best * 1e-3) / 1e12, 3)}
        del k, v
        torch.cuda.empty_cache()
    return res


def time_queue(lmm, points, clouds, repeats, slots, scale):
    jobs = []
    for c in range(clouds):
        cloud = W.synthetic_point_cloud(c, points).to("cuda:0")
        budget = max(8, int(QUEUE_BUDGETS[c % len(QUEUE_BUDGETS)] * scale))
        jobs += [(cloud, 1000, None, len(jobs) + r, budget) for r in range(repeats)]
    top = max(j[4] for j in jobs)
    out = {"jobs": len(jobs), "clouds": clouds, "repeats_per_cloud": repeats, "slots": slots, "budget_min": min(j[4] for j in jobs), "budget_max": top}
    ids = {}
    for name, fork in (("warm", True), ("off", False), ("on", True)):
        _, ids[name] = lmm.generate_queue(jobs, slots, tokenizer=object(), max_new_tokens=top, min_new_tokens=top, fork_repeats=fork)
        torch.cuda.synchronize()
        st = lmm.last_queue_stats
        if name != "warm":
            out[name] = {"prefill_ms": round(st["prefill_ms"], 2), "decode_ms": round(st["decode_ms"], 1), "admissions": st["admissions"],
                         "forked": st["forked"], "steps": st["steps"]}
    out["jobs_with_equal_ids"] = sum(int((a == b).all()) for a, b in zip(ids["off"], ids["on"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["fp32", "fp16"], choices=["fp16", "fp32"])
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--room", type=int, default=64, help="max_new_tokens the cache is reserved for behind the prefill")
    ap.add_argument("--queue-clouds", type=int, default=16)
    ap.add_argument("--queue-slots", type=int, default=12)
    ap.add_argument("--queue-scale", type=float, default=0.05, help="multiplies the queue jobs' budgets")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.rows
    classes = {
        "one_cloud": [0] * B,
        "clouds_of_4_rows": [i % max(1, B // 4) for i in range(B)],
        "singletons": list(range(B)),
    }
    res = {"rows": B, "layers": a.layers, "points": a.points, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "modes": {}}
    seq_len = None
    for precision in a.precision:
        opt = dataclasses.replace(config_defaults["ArAE"], num_layers=a.layers, generate_mode="greedy")
        lmm = LMM(opt, "cuda:0", precision=precision)
        lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        mode = {"encode_prefill_ms": {}}
        for name, cls in classes.items():
            conds = torch.cat([W.synthetic_point_cloud(c, a.points) for c in cls]).to("cuda:0")
            mode["encode_prefill_ms"][name] = time_encode_prefill(lmm, conds, a.rounds, a.room)
            print(f"[bench_fork_prefill] {precision} {name}: {mode['encode_prefill_ms'][name]}", file=sys.stderr, flush=True)
        seq_len = opt.num_cond_tokens + 1
        lmm.mesh_decoder.reserve(1, 64)
        mode["queue"] = time_queue(lmm, a.points, a.queue_clouds, 3, a.queue_slots, a.queue_scale)
        print(f"[bench_fork_prefill] {precision} queue: {mode['queue']}", file=sys.stderr, flush=True)
        res["modes"][precision] = mode
        lmm.mesh_decoder.close()
        del lmm
        torch.cuda.empty_cache()
    d = config_defaults["ArAE"]
    heads = d.num_heads
    res["fork_launch"] = time_fork_launch(a.layers, B, heads, seq_len + a.room + 1, d.hidden_dim // heads, seq_len,
                                          {k: v for k, v in classes.items() if k != "singletons"}, 5)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
