"""The GEMM kernels' index maps without a device: csrc/er_gemm_map.h (XCD-aware tile order, the streamed kernel's dealing and band
order, the swizzled 128-byte row image and its conflict-free fragment reads, the 32 x 32 MFMA C/D map, the GEGLU row permutation)
enumerated by the stand-alone program tests/host/gemm_map_check.cpp - built plain and with the host sanitizers and run directly."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edgerunner_amd", "csrc")


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "gemm_map_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def test_kernels_compile_the_checked_header():
    """The header is what the kernels compile: the GEMM and LDS-DMA attention kernels reach it through their includes and spell out
    none of its maps themselves - no C/D row expression, no XCD order, no swizzle key, no dealing arithmetic, no second GEGLU map."""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("k_gemm.h", "k_gemm_stream.h", "k_gemm_lanes.h", "k_flash_attn.h", "k_flash_lanes.h")}
    assert '#include "er_gemm_map.h"' in src["k_gemm_lanes.h"] and '#include "k_gemm_lanes.h"' in src["k_gemm.h"]
    assert '#include "k_gemm.h"' in src["k_gemm_stream.h"] and '#include "er_gemm_map.h"' in src["k_flash_lanes.h"]
    code = {f: "\n".join(l.split("//")[0] for l in t.split("\n")) for f, t in src.items()}       # comments may describe the maps
    for f, t in code.items():
        assert not re.search(r"8 \* \(r >> 2\)", t), (f, "the C/D row map is mfma32_row")
        assert not re.search(r">> 1\) & 7", t), (f, "the swizzle key is swz_key / swz_slot")
        assert not re.search(r"\bxq\b|\bxcd\b", t), (f, "the XCD order / dealing is xcd_tile / gs_deal")
        assert "gemm_hh_geglu_row(int" not in t and "gs_tile_coords(int" not in t, (f, "defined in er_gemm_map.h")
    assert "mfma32_row" in code["k_gemm.h"] and "mfma32_row" in code["k_flash_lanes.h"]
    assert code["k_gemm.h"].count("xcd_tile(") == 3 and code["k_gemm_stream.h"].count("gs_deal(") == 1
    assert "global_load_lds_dwordx4" not in code["k_gemm.h"] and "global_load_lds_dwordx4" not in code["k_flash_attn.h"]      # er_common.h er_glds16


def test_index_maps_plain(tmp_path):
    out = subprocess.run([build(tmp_path, "gemm_map_check", [])], check=True, capture_output=True, text=True)
    assert "gemm_map_check: ok" in out.stdout


def test_index_maps_under_sanitizers(tmp_path):
    exe = build(tmp_path, "gemm_map_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "gemm_map_check: ok" in out.stdout
