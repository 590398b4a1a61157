"""The fused MLP's finish launch without a device: the lane mapping and the level schedule of csrc/er_mlp_map.h (mlp_fin_chain,
mlp_fin_piece, mlp_fin_level) for 8, 16 and 32 outputs per workgroup (the kernel is launched with 32).  tests/host/mlp_finish_tree_check.cpp checks that (load, lane) ->
(chain, piece) covers a slice's 64 chains x NC / 4 pieces exactly once and that the schedule - register adds for the chain bits held
in the load index, lane steps for the others - gives the bit pattern of the plain 64-lane butterfly of er_common.h's wave_sum, for
16 000 vectors per form (magnitudes over twelve decades, signed zeros, one huge element).  Built with the host sanitizers and run
directly, as tests/test_mlp_sparse_cpu.py builds its program."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "mlp_finish_tree_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def test_finish_map_and_tree_under_sanitizers(tmp_path):
    exe = build(tmp_path, "mlp_finish_tree_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "mlp_finish_tree_check: ok (48000 vectors)" in out.stdout

