"""The tiled byte copy of fp8 mode without a device: csrc/er_w8_tile_map.h (where weight (n, k) of a row-major e4m3 matrix lives in the
copy the matrix-core batched projections stream) enumerated by the stand-alone program tests/host/w8_tile_check.cpp - every (n, k) of
[N][K] in exactly one (tile, lane, byte), pad rows zero, and every lane's load holding the weights the fp16 form holds in that slot; N =
4608, 1536, 6144 and N that are no multiple of 32.  Built plain and with the host sanitizers and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edgerunner_amd", "csrc")


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "w8_tile_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def test_kernels_compile_the_checked_header():
    """Both kernels that touch the tiled bytes take their indices from the header: the one that tiles and the one that streams."""
    src = open(os.path.join(CSRC, "k_gemv_mfma.h")).read()
    code = "\n".join(l.split("//")[0] for l in src.split("\n"))
    assert '#include "er_w8_tile_map.h"' in code
    assert code.count("w8t_piece_source(") == 1 and code.count("w8t_piece(") == 1 and code.count("w8t_scales(") == 1
    api = open(os.path.join(CSRC, "er_api.hip")).read()
    assert "w8t_" not in api, "the host layer sizes the copy through tiled_weight_bytes<w8_t> and nothing else"


def test_tile_map_plain(tmp_path):
    out = subprocess.run([build(tmp_path, "w8_tile_check", [])], check=True, capture_output=True, text=True)
    assert "w8_tile_check: ok" in out.stdout


def test_tile_map_under_sanitizers(tmp_path):
    exe = build(tmp_path, "w8_tile_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "w8_tile_check: ok" in out.stdout
