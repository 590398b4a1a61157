"""The decode step's decision table without a device: csrc/er_decode_plan.h (plan of a reserved shape, form of each projection, "the
step can launch this") enumerated by the stand-alone program tests/host/decode_plan_check.cpp, once plain and once under the host
sanitizers, and the forms it reaches held against the coverage table of tests/test_gpu_decode_proj.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every (projection, form, waves x rows, weight type) proj_form returns over batch 1..40 and 64, both precisions, ER_DECODE_V 2 / 3,
# ER_ATTN_V_BATCHED 0 / 1 / 3, ER_FORCE_BATCHED / ER_BATCHED_VALU / ER_XT on and off, ER_NW_QKV 4 / 6 / 9, ER_NW_FC1 4 / 12,
# ER_RW_FC2 2 / 4 / 6, Lcap 64 / 8192 / 8224, first / middle / last layer ("0x0": the batched forms' shapes are fixed per projection)
REACHED = """
fc1 mfma 0x0 fp16    fc1 mfma 0x0 fp32    fc1 row 12x2 fp16    fc1 row 12x2 fp32    fc1 row 4x2 fp16     fc1 row 4x2 fp32
fc1 valu 0x0 fp16    fc1 valu 0x0 fp32    fc1 xt 0x0 fp16
fc2 defer 0x0 fp16   fc2 mfma 0x0 fp16    fc2 mfma 0x0 fp32    fc2 narrow 0x0 fp16  fc2 row 4x2 fp16     fc2 row 4x2 fp32
fc2 row 4x4 fp16     fc2 row 4x6 fp16     fc2 valu 0x0 fp16    fc2 valu 0x0 fp32
head row 4x1 fp16    head row 4x1 fp32    head valu 0x0 fp16   head valu 0x0 fp32
out defer 0x0 fp16   out mfma 0x0 fp16    out mfma 0x0 fp32    out row 3x1 fp16     out row 3x1 fp32     out rows8 3x1 fp16
out rows8 3x1 fp32   out valu 0x0 fp16    out valu 0x0 fp32
qkv mfma 0x0 fp16    qkv mfma 0x0 fp32    qkv row 4x1 fp16     qkv row 4x1 fp32     qkv row 6x1 fp16     qkv row 6x1 fp32
qkv row 9x2 fp16     qkv row 9x2 fp32     qkv valu 0x0 fp16    qkv valu 0x0 fp32    qkv xt 0x0 fp16
"""
REACHED = sorted(" ".join(t) for t in re.findall(r"(\w+) (\w+) (\d+x\d+) (fp16|fp32)", REACHED))


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "decode_plan_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module")
def reached(tmp_path_factory):
    """The program's output: every proj_form result is legal and the relations the step relies on hold, or it exits non-zero."""
    out = subprocess.run([build(tmp_path_factory.mktemp("plan"), "decode_plan_check", [])], check=True, capture_output=True, text=True).stdout
    assert "decode_plan_check: ok" in out
    return sorted(re.findall(r"^reached (.+)$", out, flags=re.M))


def test_forms_the_step_reaches(reached):
    assert reached == REACHED, (sorted(set(reached) - set(REACHED)), sorted(set(REACHED) - set(reached)))


def test_every_reached_form_is_in_the_coverage_table(reached):
    """tests/test_gpu_decode_proj.py's docstring lists `projection form shapes weights ...` per line (shapes: waves x rows, comma
    separated, or - for a batched form)."""
    text = open(os.path.join(ROOT, "tests", "test_gpu_decode_proj.py")).read()
    table = set()
    for proj, form, shapes, wt in re.findall(r"^  (qkv|out|fc1|fc2|head) +(row|rows8|valu|mfma|xt|narrow|defer) +(\S+) +(fp16|fp32) ", text, flags=re.M):
        for s in shapes.split(","):
            table.add(f"{proj} {form} {'0x0' if s == '-' else s} {wt}")
    missing = [t for t in reached if t not in table]
    assert not missing, f"forms the decode step reaches that the coverage table does not name: {missing}"
    assert not sorted(table - set(reached)), f"the coverage table names forms the step never reaches: {sorted(table - set(reached))}"


def test_decision_table_under_sanitizers(tmp_path):
    exe = build(tmp_path, "decode_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "decode_plan_check: ok" in out.stdout
