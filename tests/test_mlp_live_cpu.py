"""Which fc2 rows the fused single-row MLP requests, without a device: the slot map of csrc/er_mlp_map.h (mlp_live_count,
mlp_live_slots, mlp_live_lane, mlp_live_place) for all 4096 live masks of a half-chain.  tests/host/mlp_live_check.cpp checks that the
slots list exactly the live places in ascending order, that the requested count is the next multiple of 4 (0 for the empty mask),
that pad slots carry f = +0 and the zero row, and that a float chain over the compacted slots equals the 12-step chain with zeros up
to the sign of a zero result, which no add of the finish tree lets through (24 chains per mask, products that underflow to -0
among them).  Built plain and with the host sanitizers and run directly, as tests/test_mlp_finish_cpu.py builds its program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "mlp_live_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_live_slots_and_compacted_chain(tmp_path, extra):
    exe = build(tmp_path, "mlp_live_check" + ("_san" if extra else ""), extra)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "mlp_live_check: ok (4096 masks, 98304 chains" in out.stdout
