"""The queue mode's host side without a device: the scheduler (edgerunner_amd/queue.py) against a scripted engine, and the C++
bookkeeping behind er_queue_* (csrc/er_queue_host.h) as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import pytest

from edgerunner_amd.queue import QueueScheduler, free_runs, list_scheduling_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeEngine:
    """Every job runs `lengths[j]` steps; the engine looks at its slots every `check_every` steps, as er_queue_run does."""

    def __init__(self, slots, lengths, check_every=1):
        self.slots, self.lengths, self.check_every = slots, lengths, check_every
        self.job = [None] * slots          # job in each slot
        self.ran = [0] * slots             # steps since its admission
        self.steps = 0
        self.admitted = []                 # job indices in admission order
        self.calls = []                    # (slot0, jobs) per admit call

    def admit(self, slot0, jobs):
        assert jobs, "an admit call carries at least one job"
        for i, j in enumerate(jobs):
            assert 0 <= slot0 + i < self.slots
            assert self.job[slot0 + i] is None, f"slot {slot0 + i} is occupied"
            self.job[slot0 + i], self.ran[slot0 + i] = j, 0
            self.admitted.append(j)
        self.calls.append((slot0, list(jobs)))

    def _done(self):
        return [s for s in range(self.slots) if self.job[s] is not None and self.ran[s] >= self.lengths[self.job[s]]]

    def run(self):
        if all(j is None for j in self.job):
            return []
        while not self._done():
            self.steps += self.check_every
            for s in range(self.slots):
                if self.job[s] is not None:
                    self.ran[s] += self.check_every
        return self._done()

    def take(self, slot):
        j = self.job[slot]
        assert j is not None and self.ran[slot] >= self.lengths[j]
        self.job[slot] = None
        return ("result", j)


def serve(slots, lengths, check_every=1):
    eng, sched = FakeEngine(slots, lengths, check_every), QueueScheduler(slots)
    return eng, sched, sched.serve(eng, len(lengths))


def test_free_runs():
    assert free_runs([]) == []
    assert free_runs({3, 0, 1, 5, 6, 7}) == [(0, 2), (3, 1), (5, 3)]


@pytest.mark.parametrize("slots,check_every", [(1, 1), (2, 4), (3, 1), (6, 8), (32, 32)])
def test_results_in_job_order_every_job_once_within_the_bound(slots, check_every):
    lengths = [95, 39, 11, 39, 95, 11, 11, 160, 1, 57, 32, 33, 8, 120, 64] * 3
    eng, sched, results = serve(slots, lengths, check_every)
    assert results == [("result", j) for j in range(len(lengths))]
    assert sorted(eng.admitted) == list(range(len(lengths))), "every job is admitted exactly once"
    assert eng.admitted == list(range(len(lengths))), "jobs are admitted in index order"
    assert all(0 <= s < slots for s in sched.slot_of)
    assert sched.admissions == eng.calls
    assert eng.steps <= list_scheduling_bound(lengths, slots, check_every)


def test_first_fill_is_one_contiguous_run_and_refills_use_runs():
    eng, sched, _ = serve(4, [10, 10, 30, 30, 5, 5, 5])
    assert eng.calls[0] == (0, [0, 1, 2, 3]), "an empty queue is filled by one call over all slots"
    assert eng.calls[1] == (0, [4, 5]), "slots 0 and 1 finish together: one call over the run"
    assert eng.calls[2] == (0, [6])
    assert sched.slot_of == [0, 1, 2, 3, 0, 1, 0]


def test_empty_job_list_and_more_slots_than_jobs():
    eng, _, results = serve(3, [])
    assert results == [] and eng.calls == [] and eng.steps == 0
    eng, sched, results = serve(8, [7, 3])
    assert results == [("result", 0), ("result", 1)]
    assert eng.calls == [(0, [0, 1])] and sched.slot_of == [0, 1] and eng.steps == 7
    with pytest.raises(ValueError):
        QueueScheduler(0)


def test_engine_that_reports_nothing_is_an_error():
    class Stuck(FakeEngine):
        def run(self):
            return []
    with pytest.raises(RuntimeError, match="no finished job"):
        QueueScheduler(2).serve(Stuck(2, [5]), 1)


def test_list_scheduling_bound_arithmetic():
    assert list_scheduling_bound([], 4) == 0.0
    assert list_scheduling_bound([95, 39, 11], 2, 4) == (96 + 40 + 12) / 2 + 0.5 * 96


def test_host_bookkeeping_under_sanitizers(tmp_path):
    """Argument validation and the er_queue_stats arithmetic, compiled with their own main and run under ASan + UBSan."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "queue_host_check")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "host", "queue_host_check.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    elif "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # gcc links the runtimes dynamically by default: keep the program self-contained
    subprocess.run(cmd, check=True, cwd=ROOT)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert "queue_host_check: ok" in out.stdout
