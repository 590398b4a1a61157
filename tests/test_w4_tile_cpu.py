"""The tiled nibble copy of fp4 mode without a device: csrc/er_w4_tile_map.h (where weight (n, k) and the scale of block (n, k / 32) of an
MXFP4 matrix live in the copy the matrix-core batched projections stream) enumerated by the stand-alone program
tests/host/w4_tile_check.cpp - offsets injective, the inverse agreeing, every byte a weight, a scale or named padding, and every lane's
loads holding the (row, k) set the fp16 tiled copy gives that lane.  Built plain and with the host sanitizers and run directly.  The
program also prints the launch rules of csrc/er_w4_rule.h, which are compared here with a table written out below, and header, binding
and library are compared on the new entry er_ctx_w4_streams_batched."""
import functools
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edgerunner_amd", "csrc")
SHAPES = [(4608, 1536), (6144, 1536), (1536, 6144), (1536, 1536), (501, 6144), (48, 1536)]
QKV, OUT, FC1, FC2, HEAD = range(5)

# (projection, B) pairs whose matrix-core nibble form measured faster than the fp16 form of the same build, in the same session, by more
# than the spread of the fp16 runs (profiles/w4_batched_bench.json: B = 8, 16, 32, fp16 and byte caches; batches in between go with the
# measured ones, csrc/er_w4_rule.h).  All four passed in every case in which they have a matrix-core form: qkv, fc1 and fc2 in six of
# six, out_proj at B = 16 and 32 with either cache (at B <= 8 it runs the eight-row VALU pass, which the plan - not this rule - excludes).
MEASURED_BATCHED = (QKV, OUT, FC1, FC2)


def measured_batched_rule(proj, B):
    """w4_streams_batched(proj, B, -1) as this file states it (tests/test_gpu_w4_batched.py compares a live context with it)."""
    return 5 <= B and proj in MEASURED_BATCHED


def build(tmp_path, name, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library's own build needs one)"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "w4_tile_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


@functools.lru_cache(maxsize=None)
def sanitized_lines():
    import tempfile
    import pathlib
    exe = build(pathlib.Path(tempfile.mkdtemp(prefix="w4t_")), "w4_tile_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "w4_tile_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    return [l.split() for l in out.stdout.splitlines()]


def test_kernels_compile_the_checked_header():
    """The kernel that tiles and the kernel that streams take their indices from the header, and nobody else computes them."""
    strip = lambda src: "\n".join(l.split("//")[0] for l in src.split("\n"))
    mfma = strip(open(os.path.join(CSRC, "k_gemv_mfma.h")).read())
    assert '#include "er_w4_tile_map.h"' in mfma
    for fn in ("w4t::lane_a_offset(", "w4t::lane_b_offset(", "w4t::lane_scale_offset("):
        assert mfma.count(fn) == 1, fn
    weights = strip(open(os.path.join(CSRC, "er_weights.h")).read())
    assert weights.count("w4t::what(") == 1 and "w4_tile_kernel" in weights
    assert "1664" not in mfma and "1664" not in weights and "1664" not in strip(open(os.path.join(CSRC, "er_api.hip")).read())


def test_tile_map_plain(tmp_path):
    out = subprocess.run([build(tmp_path, "w4_tile_check", [])], check=True, capture_output=True, text=True)
    assert "w4_tile_check: ok" in out.stdout


def test_tile_map_under_sanitizers():
    m = [[int(t) for t in l[1:]] for l in sanitized_lines() if l[0] == "M"]
    assert [tuple(r[:2]) for r in m] == SHAPES
    for n, k, units, total in m:                                  # 1664 bytes per (32 rows, 96 k): 0.5417 bytes per weight, padding rows included
        assert units == (n + 31) // 32 * (k // 96) and total == units * 1664


def test_batched_rule_over_projection_batch_and_knob():
    rule = {(int(p), int(b), int(k)): (int(v), int(rows)) for _, p, b, k, v, rows in (l for l in sanitized_lines() if l[0] == "R")}
    assert len(rule) == 5 * 34 * 3
    for (proj, B, knob), (batched, rows) in rule.items():
        if proj == HEAD or B <= 4 or knob == 0:
            assert batched == 0, (proj, B, knob)                 # never the lm_head, never B <= 4, never under ER_W4_BATCHED=0
        elif knob == 1:
            assert batched == 1, (proj, B, knob)                 # every matrix-core form of qkv, out_proj, fc1, fc2
        else:
            assert batched == int(measured_batched_rule(proj, B)), (proj, B)
        # w4_streams (the row forms) is what tests/test_w4_cpu.py pins, whatever is added beside it
        want_rows = 0 if proj in (OUT, HEAD) or not 1 <= B <= 4 or knob == 0 else 1 if knob == 1 else int(proj in (FC1, FC2) or (proj == QKV and B == 1))
        assert rows == want_rows, (proj, B, knob)
        assert not (batched and rows), "a row form and a batched form never both stream at one B"


def test_header_binding_and_library_agree_on_the_new_entry():
    from edgerunner_amd import native
    from edgerunner_amd.shape_opt import NativeShapeOPT
    name = "er_ctx_w4_streams_batched"
    header = open(os.path.join(ROOT, "include", "edgerunner_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*er_ctx\s*\*\s*ctx\s*,\s*int32_t\s+out\[4\]\s*\)\s*;" % name, header)
    assert name in native.EXPORTS and callable(getattr(NativeShapeOPT, "w4_streams_batched"))
    api = open(os.path.join(CSRC, "er_api.hip")).read()
    assert re.search(r'extern "C" int %s\(er_ctx\* c, int32_t out\[4\]\)' % name, api)
    from edgerunner_amd import build as B
    B.build(verbose=False)              # cross-compiles for gfx950 when stale; no GPU needed
    assert hasattr(native.load_library(), name), "the built library does not export the entry"
