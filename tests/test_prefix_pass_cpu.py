"""The prefix-pass switch without a device: header, binding and library agree on ``er_set_prefix_pass`` and ``er_k_attn_shared_mfma``,
the two entries refuse what they can refuse before any HIP call, and the plan rule behind the switch (csrc/er_decode_plan.h:
``shared_mfma`` only with prefix groups on a batched shape, an fp16 cache and head_dim 96; never with a byte cache) is enumerated by the
stand-alone program tests/host/prefix_pass_plan_check.cpp, once plain and once under the host sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("er_set_prefix_pass", "er_k_attn_shared_mfma")


def test_header_and_binding_agree():
    from edgerunner_amd import native
    src = open(os.path.join(ROOT, "include", "edgerunner_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint {name}\(", src) and name in native.EXPORTS, name
    assert re.search(r"enum er_prefix_pass \{ ER_PREFIX_PASS_VALU = 0, ER_PREFIX_PASS_MFMA = 1 \}", src)
    assert re.search(r"\bER_ATTN_SHARED_MFMA = 6\b", src)
    assert (native.ER_PREFIX_PASS_VALU, native.ER_PREFIX_PASS_MFMA, native.ER_ATTN_SHARED_MFMA) == (0, 1, 6)
    assert native.PREFIX_PASSES == {"valu": 0, "mfma": 1}
    # the unit entry takes er_k_attn_shared's argument list
    args = {n: re.sub(r"\s+", " ", re.search(rf"\bint {n}\(([^)]*)\)", src).group(1)) for n in ("er_k_attn_shared", "er_k_attn_shared_mfma")}
    assert args["er_k_attn_shared"] == args["er_k_attn_shared_mfma"]


def test_library_exports_and_early_refusals():
    from edgerunner_amd import build, native
    build.build(verbose=False)
    lib = native.load_library()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    assert lib.er_k_attn_shared_mfma.argtypes == lib.er_k_attn_shared.argtypes
    assert lib.er_set_prefix_pass(None, native.ER_PREFIX_PASS_MFMA) == -1                    # ER_ERR_INVALID: null context
    buf = (C.c_float * 8)()
    one = native.i32_array([1])
    zero = native.i32_array([0])
    for kv_half in (0, 2):          # an fp32 and a byte cache: ER_ERR_UNSUPPORTED before anything is allocated or launched
        rc = lib.er_k_attn_shared_mfma(C.addressof(buf), C.addressof(buf), C.addressof(buf), one, zero, 1, C.addressof(buf), None, 1, 16, 32, kv_half, None)
        assert rc == -5 and b"fp16" in lib.er_last_error(), (kv_half, rc, lib.er_last_error())
    rc = lib.er_k_attn_shared_mfma(C.addressof(buf), C.addressof(buf), C.addressof(buf), one, zero, 0, C.addressof(buf), None, 1, 16, 32, 1, None)
    assert rc == -1 and b"er_k_attn_shared_mfma: prefix_len" in lib.er_last_error()          # the shared check names the entry that was called


def test_python_layer_refuses_unknown_passes():
    from edgerunner_amd import kernels
    with pytest.raises(ValueError):
        kernels.attn_shared(None, None, None, [], [], 1, prefix_pass="wmma")


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "prefix_pass_plan_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_plan_rule_enumerated(tmp_path, extra):
    out = subprocess.run([build(tmp_path, "prefix_pass_plan_check", extra)], check=True, capture_output=True, text=True).stdout
    assert "prefix_pass_plan_check: ok" in out, out
