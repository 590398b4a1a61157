"""The host side of the forked prefill without a device: ``fork_plan`` / ``fork_streams`` / ``queue_fork_split``
(edgerunner_amd/models.py) on hand-written and random batches, and ``check_admit_copy`` / ``admit_copy`` behind er_queue_admit_copy
(csrc/er_queue_host.h) as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgerunner_amd.models import fork_plan, fork_streams, queue_fork_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_plan(conds, resume, order, leader, n_leaders):
    """Every property er_prefill_fork and generate_ids rest on, against the batch itself."""
    B = conds.shape[0]
    assert sorted(order) == list(range(B)), "order is a permutation"
    key = lambda b: (conds[b].tobytes(), b"" if resume is None else resume[b].tobytes())
    # leaders first, in first-occurrence order: exactly the rows whose key was not seen before, ascending
    firsts = [b for b in range(B) if key(b) not in {key(a) for a in range(b)}]
    assert n_leaders == len(firsts) and order[:n_leaders] == firsts
    assert order[n_leaders:] == sorted(order[n_leaders:]), "the repeats keep the caller's order (stable)"
    # er_prefill_fork's table rule; it is also a legal er_set_prefix_groups table
    assert len(leader) == B
    for i in range(B):
        assert leader[i] == i if i < n_leaders else 0 <= leader[i] < n_leaders
        assert leader[i] <= i and leader[leader[i]] == leader[i]
        assert key(order[i]) == key(order[leader[i]]), "a row and its leader hold the same input"
    for i in range(n_leaders):
        for k in range(i):
            assert key(order[i]) != key(order[k]), "two leaders never hold the same input"
    # un-permuting restores the caller's order
    permuted = np.asarray(order)
    back = np.empty(B, dtype=np.int64)
    back[permuted] = np.arange(B)
    assert np.array_equal(permuted[back], np.arange(B))
    assert np.array_equal(conds[permuted][back], conds)


def test_fork_plan_by_hand():
    c = np.zeros((6, 4, 3), dtype=np.float32)
    for b, v in enumerate([0, 0, 3, 0, 3, 4]):
        c[b] += v
    assert fork_plan(c) == ([0, 2, 5, 1, 3, 4], [0, 1, 2, 0, 0, 1], 3)
    assert fork_plan(torch.from_numpy(c)) == fork_plan(c)
    check_plan(c, None, *fork_plan(c))
    # no repeats: the identity, every row its own leader
    assert fork_plan(c[[0, 2, 5]]) == ([0, 1, 2], [0, 1, 2], 3)
    # one class
    assert fork_plan(c[[0, 1, 3]]) == ([0, 1, 2], [0, 0, 0], 1)
    # a repeat in front of a new class: the new class's first row moves in front of it
    assert fork_plan(c[[0, 1, 2]]) == ([0, 2, 1], [0, 1, 0], 2)


def test_fork_plan_tells_resume_ids_and_zero_signs_apart():
    c = np.zeros((4, 2, 3), dtype=np.float32)
    r = np.array([[5, 6], [5, 6], [5, 7], [5, 6]], dtype=np.int64)
    assert fork_plan(c, r) == ([0, 2, 1, 3], [0, 1, 0, 0], 2), "rows 0, 1, 3 are equal; row 2 differs in resume_ids only"
    assert fork_plan(c, torch.from_numpy(r)) == fork_plan(c, r)
    assert fork_plan(c) == ([0, 1, 2, 3], [0, 0, 0, 0], 1)
    z = c.copy()
    z[1, 0, 0] = -0.0
    assert z[1, 0, 0] == c[1, 0, 0], "the values compare equal; the bits do not"
    assert fork_plan(z) == ([0, 1, 2, 3], [0, 1, 0, 0], 2), "-0.0 and 0.0 are different inputs"
    # without conditioning the resume rows alone tell the rows apart
    assert fork_plan(None, r) == ([0, 2, 1, 3], [0, 1, 0, 0], 2)
    with pytest.raises(ValueError):
        fork_plan(None, None)
    with pytest.raises(ValueError):
        fork_plan(c, r[:3])


def test_fork_plan_random_batches():
    rng = np.random.default_rng(20240611)
    for trial in range(300):
        B = int(rng.integers(1, 40))
        classes = int(rng.integers(1, B + 1))
        pool = rng.standard_normal((classes, 5, 3)).astype(np.float32)
        conds = pool[rng.integers(0, classes, size=B)]
        resume = None
        if trial % 3 == 1:
            resume = rng.integers(0, 3, size=(B, 2)).astype(np.int64)
        elif trial % 3 == 2:
            conds = conds.copy()
            conds[rng.integers(0, B), 0, 0] = -0.0
            conds[rng.integers(0, B), 0, 0] = 0.0
        check_plan(conds, resume, *fork_plan(conds, resume))


def test_fork_streams():
    order = [0, 2, 5, 1, 3, 4]
    assert fork_streams(order) == order, "row_streams=None: permuted place i draws from the stream of the caller's row order[i]"
    given = [100, 101, 102, 103, 104, 105]
    assert fork_streams(order, given) == [100, 102, 105, 101, 103, 104]
    assert fork_streams(order, np.asarray(given)) == [100, 102, 105, 101, 103, 104]
    with pytest.raises(ValueError):
        fork_streams(order, given[:5])


def test_queue_fork_split():
    assert queue_fork_split([]) == []
    assert queue_fork_split(["a", "a", "b", "a", "b", "c"]) == [0, 0, 2, 0, 2, 5]
    assert queue_fork_split(["a", "b", "c"]) == [0, 1, 2]


def test_queue_jobs_are_keyed_by_cloud_face_count_and_resume():
    from edgerunner_amd.models import _QueueJob
    c = torch.zeros(8, 3)
    jobs = [_QueueJob(j, spec, 16) for j, spec in enumerate([
        (c, 1000), (c.clone(), 1000, None, 7, 9), (c, 800), (c, 1000, torch.tensor([1, 2])), (c[None], 1000), (c + 1, 1000),
        (c, 1000, torch.tensor([1, 2]))])]
    assert queue_fork_split([j.input_key() for j in jobs]) == [0, 0, 2, 3, 0, 5, 3], "stream and budget are not part of the key"


def test_admit_copy_bookkeeping_under_sanitizers(tmp_path):
    """check_admit_copy / admit_copy, compiled with their own main and run under ASan + UBSan (as tests/test_queue_cpu.py builds
    queue_host_check.cpp)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "queue_fork_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "host", "queue_fork_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "queue_fork_check: ok" in out.stdout
