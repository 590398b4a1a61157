#!/usr/bin/env python3
"""One CRC32 per case and form of the raw output bytes of the GEMM kernels on seeded inputs (GPU box only): run once per library BUILD
(ER_LIB_PATH) and compare the printouts line for line; once more per build with ER_F16S_BK=64 in the environment (read once per
process: the only way to the BK = 64 instantiations of the register-staged split kernel).

Forms and operands are those of tests/test_gpu_gemm_epilogue.py (its FORMS, its seeded random operands, its guarded output
allocations: the CRC covers the guard rows and columns too), on its cases 2-gr40, 8-scalar-67 and 10-order and on two more shapes, a
ragged 3001 x 4164 x 192 with gate rows and a residual and a 129 x 65 x 128 with odd leading dimensions; then the fused GEGLU forms,
the V^T forms of the q/k/v projection and the two forms of the split product."""
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_gemm_epilogue as E  # noqa: E402
from edgerunner_amd import kernels as K  # noqa: E402

E.CASES["ragged-3001x4164x192"] = E.case(3001, 4164, 192, 1000)
E.CASES["small-129x65x128"] = E.case(129, 65, 128, 43, pad4=False, odd_ld=True)


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to("cuda:0")


def crc(*tensors):
    c = 0
    for t in tensors:
        if t is not None:
            c = zlib.crc32(t.contiguous().cpu().numpy().tobytes(), c)
    return c


print(f"ER_F16S_BK={os.environ.get('ER_F16S_BK', '')}")
for cname in ("2-gr40", "8-scalar-67", "10-order", "ragged-3001x4164x192", "small-129x65x128"):
    for form in E.FORMS:
        call, h16 = E.launch(cname, "random", form)
        print(f"{cname} {form}: {crc(call.view(torch.int32), None if h16 is None else h16.view(torch.int16)):08x}")

a, w, b = rnd(300, 192, seed=90), rnd(256, 192, seed=91, scale=0.05).half(), rnd(256, seed=92)
with E.environment({"ER_GEMM_STREAM": "0"}):
    for ft in (0, 1, 2, 4):
        print(f"geglu M 300 F 128 K 192 force_tile {ft}: {crc(K.gemm_hh_geglu(a, w, b, force_tile=ft).view(torch.int16)):08x}")

a, w, b = rnd(384, 192, seed=93), rnd(768, 192, seed=94, scale=0.05).half(), rnd(768, seed=95)
for name, env, ft in [(f"tile {t}", {"ER_GEMM_STREAM": "0"}, t) for t in range(5)] + [("stream", {"ER_GEMM_STREAM": "2"}, 0)]:
    with E.environment(env):
        qk, vt = K.gemm_hh_qkv(a, w, b, 128, force_tile=ft)
    print(f"qkv V^T M 384 rows 128 heads 4 K 192 {name}: {crc(qk.view(torch.int16), vt.view(torch.int16)):08x}")

a, w, b = rnd(300, 1536, seed=96), rnd(1536, 1536, seed=97, scale=0.05).half(), rnd(1536, seed=98)
for f in ("reg", "dma"):
    os.environ["ER_K_GEMM_F16S_FORM"] = f
    print(f"f16s 300 x 1536 x 1536 {f}: {crc(K.gemm_f16s(a, w, b).view(torch.int32)):08x}")
os.environ.pop("ER_K_GEMM_F16S_FORM", None)
