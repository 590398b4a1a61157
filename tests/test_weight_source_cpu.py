"""Which weight copy each decode projection streams, without a device: csrc/er_weight_source.h (weight_source: the one rule the decode
step, the builder of the derived copies, the reporters and the profile's byte accounting read) enumerated by the stand-alone program
tests/host/weight_source_check.cpp, once plain and once under the host sanitizers, and the rows of the default knobs pinned to the table
written out below - the rows tests/test_gpu_w8*.py and tests/test_gpu_w4*.py compare with live contexts."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Default knobs (ER_DECODE_V=3, ER_MLP_V=0, ER_XT on, no forced or VALU batches, fp16 / fp32 cache, no row class, measured rules), layer 0:
# the source of qkv, out_proj, fc1, fc2 per mode and batch.  One row: out_proj is the fused merge launch (fp8: the byte block).  Eight rows:
# out_proj is the eight-row VALU pass on the plain copy.  fp8: out_proj streams bytes at B <= 2 and keeps fp16 in the matrix-core forms;
# fp4: qkv streams nibbles in its row form at B = 1 only, out_proj has no nibble row form, all four stream tiled nibbles at B > 4.
PINNED = {
    ("exact", 1): "plain plain plain plain", ("exact", 2): "plain plain plain plain", ("exact", 4): "plain plain plain plain",
    ("exact", 8): "tiled plain tiled tiled", ("exact", 16): "tiled tiled tiled tiled", ("exact", 32): "tiled tiled tiled tiled",
    ("fast", 1): "plain plain plain plain", ("fast", 2): "plain plain plain plain", ("fast", 4): "plain plain plain plain",
    ("fast", 8): "tiled plain tiled tiled", ("fast", 16): "tiled tiled tiled tiled", ("fast", 32): "tiled tiled tiled tiled",
    ("fp8", 1): "bytes bytes bytes bytes", ("fp8", 2): "bytes bytes bytes bytes", ("fp8", 4): "bytes plain bytes bytes",
    ("fp8", 8): "tiled_bytes plain tiled_bytes tiled_bytes", ("fp8", 16): "tiled_bytes tiled tiled_bytes tiled_bytes",
    ("fp8", 32): "tiled_bytes tiled tiled_bytes tiled_bytes",
    ("fp4", 1): "quads plain quads quads", ("fp4", 2): "plain plain quads quads", ("fp4", 4): "plain plain quads quads",
    ("fp4", 8): "tiled_nibbles plain tiled_nibbles tiled_nibbles", ("fp4", 16): "tiled_nibbles tiled_nibbles tiled_nibbles tiled_nibbles",
    ("fp4", 32): "tiled_nibbles tiled_nibbles tiled_nibbles tiled_nibbles",
}
DEFAULTS = "force=0 valu=0 xt=1 v=3 mlp=0 rc=0 kv8=0 w8b=-1 w4r=-1 w4b=-1 L=0"


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "weight_source_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def test_decision_table_plain_and_pinned_rows(tmp_path):
    exe = build(tmp_path, "weight_source_check", [])
    assert "weight_source_check: ok" in subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    dump = subprocess.run([exe, "--dump"], check=True, capture_output=True, text=True).stdout
    rows = {}
    for mode, B, proj, src in re.findall(r"^(\w+) B=(\d+) %s (qkv|out|fc1|fc2) (\w+)$" % re.escape(DEFAULTS), dump, flags=re.M):
        rows.setdefault((mode, int(B)), []).append(src)
    got = {key: " ".join(v) for key, v in rows.items() if key in PINNED}
    assert got == PINNED, {key: (got.get(key), PINNED[key]) for key in PINNED if got.get(key) != PINNED[key]}


def test_decision_table_under_sanitizers(tmp_path):
    exe = build(tmp_path, "weight_source_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "weight_source_check: ok" in out.stdout


def test_the_rules_are_asked_in_one_place():
    """The primitive measured rules are defined once and composed by weight_source alone: nothing else under csrc calls them."""
    csrc = os.path.join(ROOT, "edgerunner_amd", "csrc")
    calls = {}
    for name in sorted(os.listdir(csrc)):
        code = "\n".join(l.split("//")[0] for l in open(os.path.join(csrc, name)).read().split("\n"))
        for fn in re.findall(r"(?<![A-Za-z0-9_])(w8_streams|w8_streams_batched|w4_streams|w4_streams_batched)\(", code):
            calls.setdefault(name, []).append(fn)
    assert sorted(calls) == ["er_w4_rule.h", "er_weight_source.h"], calls
    assert sorted(calls["er_w4_rule.h"]) == ["w4_streams", "w4_streams_batched"]                      # the definitions
    assert sorted(calls["er_weight_source.h"]) == ["w4_streams", "w4_streams_batched", "w8_streams", "w8_streams", "w8_streams", "w8_streams_batched",
                                                    "w8_streams_batched"]      # two definitions, five calls in weight_source
