#!/usr/bin/env python3
"""One CRC32 per case of the raw output bytes of the two sampling heads on seeded inputs (GPU box only): run once per library BUILD
(ER_LIB_PATH) and compare the printouts line for line.  ``K.sample_head``: ids, counters and flags; ``K.sample_head_ctl``: those
plus the bit patterns of lp_model, lp_policy and n_kept.  The rows are those of tests/test_gpu_sampling.py - 256 rows of randn * 3
with a tie inside every top-10, a state that walks the grammar's branches with every 19th row finished - at the vocabularies
70, 518, 1030 and 1088 (ER_HEAD_MAX_VOCAB), both grammars, both modes, steps 0, 1 and 17; the ctl head at its defaults and at the six
configurations of the tests; then one row of all -inf and one of NaN."""
import math
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgerunner_amd import kernels as K  # noqa: E402

B = 256
CONFIGS = [None, (0.7, 10, 0.9), (1.3, 0, 0.8), (1.0, 50, 0.5), (0.5, 0, 0.95), (2.0, 10, 1.0), (2.0, 0, 0.99)]   # None: the defaults


def rows_with_a_tie(V, seed):
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * 3
    top = torch.topk(x, 4, dim=-1).indices
    x[torch.arange(B), top[:, 3]] = x[torch.arange(B), top[:, 2]]
    return x


def head_state():
    last = [3 if b % 2 == 0 else 6 for b in range(B)]
    counter = [0 if b % 2 == 0 else 1 + (b % 3) for b in range(B)]
    unfinished = [0 if b % 19 == 7 else 1 for b in range(B)]
    return last, counter, unfinished


def crc(out):
    """out: (ids, counters, flags[, lp_model, lp_policy, n_kept]) as lists"""
    kinds = (np.int32, np.int32, np.int32, np.float32, np.float32, np.int32)
    return zlib.crc32(b"".join(np.asarray(v, dtype=k).tobytes() for v, k in zip(out, kinds)))


def both_heads(tag, logits, md, grammar, step, state):
    print(f"{tag} plain: {crc(K.sample_head(logits, md, grammar, step, *state, top_k=10, seed=1234)):08x}")
    for cfg in CONFIGS:
        kw = {} if cfg is None else dict(temperature=cfg[0], sampling_top_k=cfg[1], top_p=cfg[2])
        out = K.sample_head_ctl(logits, md, grammar, step, *state, top_k=10, seed=1234, **kw)
        print(f"{tag} ctl {'defaults' if cfg is None else cfg}: {crc(out):08x}")


for V in (70, 518, 1030, 1088):
    logits = rows_with_a_tie(V, 52).to("cuda:0")
    for grammar in (0, 2):
        for md in (0, 1):
            for step in (0, 1, 17):
                both_heads(f"V {V} grammar {grammar} mode {md} step {step}", logits, md, grammar, step, head_state())
bad = rows_with_a_tie(518, 53)
bad[3] = -math.inf
bad[4] = math.nan
for md in (0, 1):
    both_heads(f"V 518 rows 3 / 4 all -inf / NaN, mode {md}", bad.to("cuda:0"), md, 0, 2, ([7] * B, [0] * B, [1] * B))
