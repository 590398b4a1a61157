#!/usr/bin/env python3
"""One CRC32 per case of the raw output bytes of the four fused attention kernels on seeded inputs (GPU box only): run once per
library BUILD (ER_LIB_PATH) and compare the printouts line for line.  The cases are the shapes of tests/test_gpu_kernels.py's flash
tests - the point encoder's cross-attention and the key-range-split single prefill (B = 1, causal, head_dim 96, N = 2050) among them."""
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgerunner_amd import kernels as K  # noqa: E402

F16 = [(1, 16, 2048, 2048), (2, 16, 2048, 257), (1, 2, 100, 70), (1, 1, 33, 1), (2, 3, 130, 257)]                 # B, H, N, M (D = 64)
F32 = [(2, 16, 2050, 2050, 96, True), (1, 16, 2048, 4096, 64, False), (2, 3, 130, 1000, 64, False), (1, 2, 100, 100, 96, True),
       (1, 2, 70, 200, 96, True), (1, 1, 33, 1, 64, False), (1, 1, 1, 1, 96, True),                               # B, H, N, M, D, causal
       (1, 16, 2050, 2050, 96, True), (3, 4, 300, 300, 96, True), (1, 3, 64, 64, 96, True), (1, 2, 129, 129, 96, True),   # key-range split
       (6, 128, 40, 70, 64, False), (6, 128, 70, 70, 96, True), (3, 256, 100, 200, 96, True), (2, 128, 70, 70, 96, True)]  # four waves
F16S = [(2, 16, 2050, 2050, True), (1, 3, 100, 333, False), (1, 2, 33, 33, True),                                 # B, H, N, M, causal (D = 96)
        (6, 128, 70, 70, True), (6, 128, 40, 333, False), (2, 128, 70, 70, True)]


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to("cuda:0")


def crc(t):
    return zlib.crc32(t.contiguous().cpu().numpy().tobytes())


for B, H, N, M in F16:
    q, k, v = rnd(B, N, H * 64, seed=80), rnd(B, M, H * 64, seed=81), rnd(B, M, H * 64, seed=82)
    k[:, M // 2] *= 3.0
    print(f"f16  B {B} H {H} N {N} M {M}: {crc(K.flash_attn_f16(q, k, v, H)):08x}")
    print(f"hh   B {B} H {H} N {N} M {M}: {crc(K.flash_attn_hh(q, k, v, H)):08x}")
for B, H, N, M, D, causal in F32:
    q, k, v = rnd(B, N, H * D, seed=83), rnd(B, M, H * D, seed=84), rnd(B, M, H * D, seed=85)
    k[:, M // 2] *= 3.0
    print(f"f32  B {B} H {H} N {N} M {M} D {D} causal {int(causal)}: {crc(K.flash_attn_f32(q, k, v, H, causal=causal)):08x}")
for B, H, N, M, causal in F16S:
    q = rnd(B, N, H * 96, seed=80)
    k, v = rnd(B, M, H * 96, seed=81).half().float(), rnd(B, M, H * 96, seed=82).half().float()
    print(f"f16s B {B} H {H} N {N} M {M} causal {int(causal)}: {crc(K.flash_attn_f16s(q, k, v, H, causal=causal)):08x}")
