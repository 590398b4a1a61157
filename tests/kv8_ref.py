"""Shared pieces of the kv8 tests.  For tests/test_kv8_cpu.py: the host program tests/host/kv8_map_check.cpp, built with ASan + UBSan and
run once per session (host_output, encode_sweep - CPU suite only).  For both files: the e4m3 cast the byte KV cache is defined by
(torch_kv8, which the CPU test proves equal to the host encoder) and the same sweep of inputs built in torch (torch_sweep)."""
import functools
import os
import shutil
import subprocess
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32_of_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=None)
def host_output():
    """stdout lines of kv8_map_check (None: no host C++ compiler).  ASan + UBSan, as tests/test_w8_cpu.py builds w8_check."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="kv8_"), "kv8_map_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "host", "kv8_map_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    subprocess.run(cmd, check=True, cwd=ROOT)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "kv8_map_check: ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    return tuple(res.stdout.splitlines())


def encode_sweep():
    """(values fp32 [n], bytes uint8 [n]) of the host encoder's sweep: every finite code, every midpoint and its fp32 neighbours, fp32
    subnormals, +-448 and beyond, +-inf, NaNs."""
    rows = [l.split() for l in host_output() if l.startswith("E ")]
    return f32_of_bits([int(r[1]) for r in rows]), torch.tensor([int(r[2]) for r in rows], dtype=torch.int32).to(torch.uint8)


def torch_sweep():
    """fp32 [n]: the inputs of the host program's sweep, built in torch - every finite code, every midpoint between neighbouring codes
    and the fp32 numbers just below and above it, fp32 subnormals, +-448 and beyond, +-inf, quiet and signalling NaNs of both signs."""
    table = torch.arange(0x7F, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float32)      # the 127 finite magnitudes
    mid = 0.5 * (table[:-1] + table[1:])
    inf = torch.tensor(float("inf"))
    special = torch.tensor([448.0, 464.0, 480.0, 1e6, 3.0e38, float("inf"), 0.0, 1e-38, 1.1754942e-38, 1e-41, 1.4e-45])
    pos = torch.cat((table, mid, torch.nextafter(mid, -inf), torch.nextafter(mid, inf), torch.nextafter(torch.tensor([448.0]), inf), special))
    nans = f32_of_bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF])
    return torch.cat((pos, -pos, nans))


def torch_kv8(v):
    """The cache byte of fp32 values by torch: clamp(+-448) then the float8_e4m3fn cast (round to nearest even); NaN -> 0x7F | sign."""
    v = v.float()
    out = v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    nan = torch.isnan(v)
    sign = ((v.view(torch.int32) >> 24) & 0x80).to(torch.uint8)
    return torch.where(nan, sign | 0x7F, out)


def kv8_decode(b):
    """e4m3 bytes (uint8) -> fp32, through the table of all 256 codes (on the bytes' device)"""
    table = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float32)
    return table.to(b.device)[b.long()]
