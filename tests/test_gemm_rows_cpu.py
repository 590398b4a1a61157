"""The GEMM epilogues' row -> batch arithmetic without a device: csrc/er_gemm_rows.h (RowBatch with its compare and division forms,
the gate-row pair and the pre-fetched residual rows of a wave, also of a wave wholly beyond M) enumerated against m / period and
m % period over span in {32, 64}, period 1..300, M 1..600 and every wave start up to M rounded up to 256, by the stand-alone program
tests/host/gemm_rows_check.cpp - built plain and with the host sanitizers and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "gemm_rows_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def test_kernels_compile_the_checked_header():
    """The header is what the kernels compile: k_gemm.h and k_gemm_stream.h include it and define no map of their own."""
    csrc = os.path.join(ROOT, "edgerunner_amd", "csrc")
    gemm, stream = (open(os.path.join(csrc, f)).read() for f in ("k_gemm.h", "k_gemm_stream.h"))
    assert '#include "er_gemm_rows.h"' in gemm and "struct RowBatch" not in gemm and "struct RowBatch" not in stream
    assert gemm.count("gate_row_pair(") == 1 and stream.count("gate_row_pair(") == 1      # hh_epi_rows and gs_load_pre: one helper


def test_row_maps_plain(tmp_path):
    out = subprocess.run([build(tmp_path, "gemm_rows_check", [])], check=True, capture_output=True, text=True)
    assert "gemm_rows_check: ok" in out.stdout


def test_row_maps_under_sanitizers(tmp_path):
    exe = build(tmp_path, "gemm_rows_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "gemm_rows_check: ok" in out.stdout
