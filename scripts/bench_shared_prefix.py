#!/usr/bin/env python3
"""Prefix groups against the plain batch path on one GPU, same build, same process: ``LMM.generate(share_prefix=True)`` and
``share_prefix=False`` on the same batch, alternated, a warm-up run of each first.  24-layer synthetic checkpoint, 32 rows, greedy,
``min_new_tokens = max_new_tokens`` (1000 by default), fp16 and fp32.  Three batches: 32 rows of ONE cloud (what ``infer.py`` runs for
``--test_repeat 32``), 8 clouds x 4 rows, and 32 different clouds - singletons, i.e. what the two-launch form costs when nothing is
shared.  Per batch and mode it records the decode tok/s (``er_last_decode_ms``) of every round and the per-launch microseconds of
kinds 1 and 2 (``er_profile_decode_kernels_at`` at the run's mean context, replayed from a graph); per batch the byte ratio
(sum over groups of P + rows * (L - P)) / (B * L) that the attention time is to be compared with.  Prints one JSON object.

``--prefix-pass valu mfma`` gives every named prefix pass (``er_set_prefix_pass``) a shared run of its own, each alternated with the
unshared run in the same process; the object then holds ``shared_valu`` / ``shared_mfma`` per batch beside ``shared`` (the first pass
named).  The matrix-core pass reads fp16 caches only: name it with ``--precision fp16``.

    python scripts/bench_shared_prefix.py [--precision fp16 fp32] [--prefix-pass valu mfma] [--tokens 1000] [--rows 32] [--layers 24]
                                          [--rounds 2] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgerunner_amd import native  # noqa: E402
from edgerunner_amd import weights as W  # noqa: E402
from edgerunner_amd.models import LMM, prefix_leaders  # noqa: E402
from edgerunner_amd.options import config_defaults  # noqa: E402


def run(lmm, batch, T, share):
    _, toks = lmm.generate(batch, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T, share_prefix=share)
    torch.cuda.synchronize()
    return toks, lmm.mesh_decoder.last_decode_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["fp16", "fp32"], choices=["fp16", "fp32"])
    ap.add_argument("--tokens", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--prefix-pass", nargs="+", default=["valu"], choices=["valu", "mfma"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if "mfma" in a.prefix_pass and "fp32" in a.precision:
        ap.error("--prefix-pass mfma reads fp16 caches only: run it with --precision fp16")
    B, T = a.rows, a.tokens
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=a.layers, generate_mode="greedy")
    P = opt.num_cond_tokens + 1
    L = P + T // 2                       # mean context of the run
    batches = {
        "one_cloud": [0] * B,
        "clouds_of_4_rows": [i % max(1, B // 4) for i in range(B)],
        "singletons": list(range(B)),
    }
    res = {"rows": B, "layers": a.layers, "tokens": T, "prefix_len": P, "mean_context": L, "device": torch.cuda.get_device_name(0),
           "prefix_passes": list(a.prefix_pass),
           "precisions": {}}
    for precision in a.precision:
        lmm = LMM(opt, "cuda:0", precision=precision)
        lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        dec = lmm.mesh_decoder
        out = {}
        for name, which in batches.items():
            batch = torch.cat([W.synthetic_point_cloud(i, a.points) for i in which]).to("cuda:0")
            leaders = prefix_leaders(batch)
            groups = {}
            for l in leaders:
                groups[l] = groups.get(l, 0) + 1
            byte_ratio = sum(P + n * (L - P) for n in groups.values()) / (B * L)
            shares = [False] + list(a.prefix_pass)            # False = unshared, then one shared run per prefix pass
            modes = {sh: {"decode_ms": [], "tok_s": []} for sh in shares}
            ids = {}
            for share in shares:                             # warm-up of each
                run(lmm, batch, T, share)
            for _ in range(a.rounds):                        # alternated
                for share in shares:
                    toks, ms = run(lmm, batch, T, share)
                    ids[share] = toks
                    modes[share]["decode_ms"].append(round(ms, 2))
                    modes[share]["tok_s"].append(round(B * T / ms * 1e3, 1))
                    prof = dec.profile_decode_kernels(repeats=5, context_len=L, use_graph=True)
                    modes[share]["attn_kernel"] = dec.plan()["attn_kernel"]
                    modes[share].setdefault("kind1_us", []).append(round(prof["attn_decode"]["avg_us"], 2))
                    modes[share].setdefault("kind2_us", []).append(round(prof["attn_combine"]["avg_us"], 2))
            want = {"valu": native.ER_ATTN_SHARED, "mfma": native.ER_ATTN_SHARED_MFMA}
            assert modes[False]["attn_kernel"] not in want.values() and all(modes[sh]["attn_kernel"] == want[sh] for sh in a.prefix_pass)
            mean = lambda v: sum(v) / len(v)
            attn = {s: mean(modes[s]["kind1_us"]) + mean(modes[s]["kind2_us"]) for s in shares}
            first = a.prefix_pass[0]
            out[name] = {
                "groups": len(groups), "byte_ratio": round(byte_ratio, 4),
                "unshared": modes[False], "shared": modes[first],
                "tok_s_ratio": round(mean(modes[first]["tok_s"]) / mean(modes[False]["tok_s"]), 4),
                "attn_us_per_layer": {"unshared": round(attn[False], 2), "shared": round(attn[first], 2)},
                "attn_time_ratio": round(attn[first] / attn[False], 4),
                "rows_with_equal_ids": sum(int((x == y).all()) for x, y in zip(ids[False], ids[first])),
            }
            if len(a.prefix_pass) > 1 or first != "valu":
                for sh in a.prefix_pass:
                    out[name]["shared_" + sh] = dict(
                        modes[sh], tok_s_ratio=round(mean(modes[sh]["tok_s"]) / mean(modes[False]["tok_s"]), 4),
                        attn_us_per_layer=round(attn[sh], 2), attn_time_ratio=round(attn[sh] / attn[False], 4),
                        rows_with_equal_ids=sum(int((x == y).all()) for x, y in zip(ids[False], ids[sh])))
            print(f"[{precision}] {name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
        res["precisions"][precision] = out
        dec.close()
        del lmm, dec
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
