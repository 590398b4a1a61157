"""The prefill with a past without a device: header, binding and library agree on the three new entries and refuse what they can refuse
before any HIP call; the ``keep_cond`` record's match / forget rules on host tensors (``edgerunner_amd.models.CondRecord``); the job
order ``infer.py`` uses under ER_INFER_KEEP_COND=1 (``edgerunner_amd.dist.group_jobs_keep_cond``); and the host rules of
csrc/er_extend_plan.h - the attention route's threshold and the past a call may keep - enumerated by the stand-alone program
tests/host/extend_plan_check.cpp, once plain and once under the host sanitizers."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("er_prefill_extend", "er_embed_num_face", "er_k_attn_extend")


def test_header_and_binding_agree():
    from edgerunner_amd import native
    src = open(os.path.join(ROOT, "include", "edgerunner_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(rf"\bint {name}\(", src) and name in native.EXPORTS, name
    flat = re.sub(r"\s+", " ", src)
    assert "int er_prefill_extend(er_ctx* ctx, const float* embeds_new_dev, int batch, int past_len, int n_new, void* stream);" in flat
    assert "int er_embed_num_face(er_ctx* ctx, const int32_t* face_bucket_host, int batch, float* out_dev, void* stream);" in flat


def test_library_exports_and_early_refusals():
    from edgerunner_amd import build, native
    build.build(verbose=False)
    lib = native.load_library()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
    buf = (C.c_float * 8)()
    a = C.addressof(buf)
    assert lib.er_prefill_extend(None, a, 1, 1, 1, None) == -1              # ER_ERR_INVALID: null context
    assert lib.er_embed_num_face(None, native.i32_array([0]), 1, a, None) == -1
    assert lib.er_k_attn_extend(a, a, a, 0, 1, a, 1, 16, 32, 96, 0, None) == -1 and b"er_k_attn_extend" in lib.er_last_error()
    assert lib.er_k_attn_extend(a, a, a, 31, 2, a, 1, 16, 32, 96, 0, None) == -4          # ER_ERR_CAPACITY: 33 positions in a cache of 32
    assert lib.er_k_attn_extend(a, a, a, 8, 2, a, 1, 16, 32, 64, 2, None) == -5           # ER_ERR_UNSUPPORTED: byte cache at head_dim 64


# ------------------------------------------------------------------ the keep_cond record
def clouds(seed=0, B=2, N=16):
    return torch.randn(B, N, 3, generator=torch.Generator().manual_seed(seed))


def test_kept_prefix_len_follows_the_face_token():
    from edgerunner_amd.models import kept_prefix_len
    assert kept_prefix_len(2049, True) == 2048 and kept_prefix_len(2048, False) == 2048


def test_cond_record_matches_on_bits_batch_context_and_reservation():
    from edgerunner_amd.models import CondRecord, cond_key
    r = CondRecord()
    c = clouds()
    args = dict(batch=2, need_len=2100, dec_id=11, reserved=(2, 2200), epoch=5)
    assert not r.usable(c, **args)                                          # nothing recorded
    r.remember(c, 2, 2048, 11, (2, 2200), 5)
    assert r.usable(c, **args) and r.usable(c.clone(), **args) and r.usable(c.numpy().copy(), **args)
    assert r.past == 2048
    z = c.clone()
    z[0, 0, 0] = 0.0
    r0 = CondRecord()
    r0.remember(z, 2, 2048, 11, (2, 2200), 5)
    nz = z.clone()
    nz[0, 0, 0] = -0.0                                                      # -0.0 != 0.0: the comparison is on the stored bits
    assert r0.usable(z, **args) and not r0.usable(nz, **args) and cond_key(z) != cond_key(nz)
    moved = c.clone()
    moved[1, 3, 2] = torch.nextafter(moved[1, 3, 2], torch.tensor(10.0))       # one ulp in one coordinate
    assert not r.usable(moved, **args)
    assert not r.usable(c[:1], **dict(args, batch=1))                       # another batch
    assert not r.usable(c.reshape(1, 32, 3), **dict(args, batch=1))         # the same bytes in another shape
    assert not r.usable(c.double(), **args)                                 # ... or another dtype
    assert not r.usable(c, **dict(args, need_len=2201))                     # the reservation must already fit
    assert r.usable(c, **dict(args, need_len=2200))
    assert not r.usable(c, **dict(args, reserved=(2, 4000)))                # any re-reserve
    assert not r.usable(c, **dict(args, dec_id=12))                         # another native context (.half() / .float())
    assert not r.usable(c, **dict(args, epoch=6))                           # the cache was rewritten in between
    assert not r.usable(c, queue_open=True, **args)
    assert not r.usable(None, **args)
    r.forget()
    assert not r.usable(c, **args)


def test_cond_record_is_forgotten_by_casts_and_loads():
    """``.half()`` / ``.float()`` / ``load_state_dict`` on the LMM shell (no native context is created: module style, nothing materialised)."""
    import dataclasses
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=1)
    if not torch.cuda.is_available():
        m = LMM.__new__(LMM)                   # the constructor insists on a HIP device; the rules under test are plain attributes
        from edgerunner_amd.models import CondRecord
        m._cond_record, m._sources, m._dec, m._kv8 = CondRecord(), [], None, False
        m._dtype, m._w8, m._w4 = torch.float32, False, False
        from edgerunner_amd.weights import dims_from_options
        m.dims = dims_from_options(opt)
    else:
        m = LMM(opt, "cuda:0", precision=None)
    c = clouds()
    for act in (lambda: m.half(), lambda: m.float(), lambda: m.load_state_dict({}, strict=False)):
        m._cond_record.remember(c, 2, 2048, 1, (2, 2200), 0)
        act()
        assert m._cond_record.key is None


# ------------------------------------------------------------------ infer.py's job order
def test_group_jobs_keep_cond_order():
    from edgerunner_amd import dist as D
    paths = ["a", "b", "c", "d", "e"]
    n_points = {"a": 512, "b": 512, "c": 300, "d": 512, "e": 512}
    for world, rows_max, repeat in ((1, 4, 1), (1, 3, 2), (2, 4, 2), (3, 2, 1), (1, 32, 3)):
        for rank in range(world):
            jobs, mine, _ = D.plan_jobs(paths, repeat, (1000, 4000, 2500), rank, world)
            plain = D.group_jobs(jobs, mine, lambda p: n_points[p], rows_max)
            keep = D.group_jobs_keep_cond(jobs, mine, lambda p: n_points[p], rows_max)
            assert sorted(j for _, g in keep for j in g) == sorted(mine) == sorted(j for _, g in plain for j in g)      # every job once
            for nf, g in keep:
                assert 1 <= len(g) <= rows_max
                assert all(jobs[j][2] == nf for j in g) and len({n_points[jobs[j][0]] for j in g}) == 1
            # consecutive calls of one set carry the same (path, repeat) items in the same rows; a set is left only once all of its
            # face counts ran
            items = [tuple((jobs[j][0], jobs[j][1]) for j in g) for _, g in keep]
            seen, i = set(), 0
            while i < len(items):
                k = i
                while k + 1 < len(items) and items[k + 1] == items[i]:
                    k += 1
                assert items[i] not in seen, "a set of clouds came back after another set ran"
                seen.add(items[i])
                assert len({nf for nf, _ in keep[i:k + 1]}) == k + 1 - i      # its face counts, each once
                i = k + 1
    jobs, mine, _ = D.plan_jobs(["a", "b"], 1, (1000, 4000), 0, 1)
    assert D.group_jobs_keep_cond(jobs, mine, lambda p: 512, 4) == [(1000, [0, 2]), (4000, [1, 3])]
    jobs, mine, _ = D.plan_jobs(["a"], 1, (1000, 1000), 0, 1)                # a face count named twice stays two jobs
    assert D.group_jobs_keep_cond(jobs, mine, lambda p: 512, 4) == [(1000, [0]), (1000, [1])]


# ------------------------------------------------------------------ the threshold rule and the bench table behind it
def threshold():
    src = open(os.path.join(ROOT, "edgerunner_amd", "csrc", "er_extend_plan.h")).read()
    return int(re.search(r"constexpr int EXTEND_ROWS_MAX_NEW = (\d+);", src).group(1))


def test_threshold_is_where_the_measured_table_puts_it():
    """profiles/prefill_extend_bench.json holds the route table (rows vs flash, B = 1 and 32, exact and fast mode, past_len 2048): the
    constant is the largest measured n_new up to which the rows route is not slower than the flash route in ANY of the four columns."""
    table = json.load(open(os.path.join(ROOT, "profiles", "prefill_extend_bench.json")))["route_table"]
    ns = sorted({r["n_new"] for r in table})
    assert set(ns) >= {2, 8, 32, 64, 128}
    assert {(r["mode"], r["batch"]) for r in table} == {("exact", 1), ("exact", 32), ("fast", 1), ("fast", 32)}
    wins = lambda n: all(r["rows_ms"] <= r["flash_ms"] for r in table if r["n_new"] == n)
    best = 0
    for n in ns:
        if not wins(n):
            break
        best = n
    assert threshold() == best, (threshold(), best)


def build_check(tmp_path, extra):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "extend_plan_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "host", "extend_plan_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif extra and "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_extend_rules_enumerated(tmp_path, extra):
    out = subprocess.run([build_check(tmp_path, extra)], check=True, capture_output=True, text=True).stdout
    assert "extend_plan_check: ok" in out and f"rows up to n_new = {threshold()}" in out, out
