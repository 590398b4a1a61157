"""The fused single-row MLP without a device: the neuron map of csrc/er_mlp_map.h (a bijection on 0..6143 that reproduces the
(slice, j, lane, e) index formula of gemv_kernel, for 4 and 8 elements per load) and the plan flag that selects the fused launches
(one exact row -> fused; two rows, knob off, forced batched, another width -> not), checked by the stand-alone program
tests/host/mlp_map_check.cpp built with the host sanitizers and run directly."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "mlp_map_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def test_map_and_plan_selection_under_sanitizers(tmp_path):
    exe = build(tmp_path, "mlp_map_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "mlp_map_check: ok" in out.stdout


def test_plan_selection_cases(tmp_path):
    """The four cases by name, through a tiny program of their own: B = 1 exact -> fused; B = 2; knob off; a model of another width."""
    src = tmp_path / "cases.cpp"
    src.write_text('''
#include <cstdio>
#include "%s/edgerunner_amd/csrc/er_decode_plan.h"
using namespace er;
int main() {
    const AttnChunking ch{16, 16 * 512, 128};
    const ReserveKnobs rk{false, false, true};
    DecodeKnobs on, off;
    on.mlp_v = 1; off.mlp_v = 0;
    printf("%%d %%d %%d %%d\\n",
           (int)make_decode_plan(on, rk, false, 1, 6080, 24, 16, 96, 1536, ch).mlp_fused,
           (int)make_decode_plan(on, rk, false, 2, 6080, 24, 16, 96, 1536, ch).mlp_fused,
           (int)make_decode_plan(off, rk, false, 1, 6080, 24, 16, 96, 1536, ch).mlp_fused,
           (int)make_decode_plan(on, rk, false, 1, 6080, 24, 16, 64, 1024, ch).mlp_fused);
    return 0;
}
''' % ROOT)
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / "cases")
    cmd = [cxx, "-std=c++17", "-o", exe, str(src)]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    subprocess.run(cmd, check=True)
    assert subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split() == ["1", "0", "0", "0"]
