"""Scheduler of the queue mode (continuous batching): serves a list of independent jobs from a fixed number of cache rows ("slots").

``LMM.generate`` runs a batch until its longest row ends; a row that finished early keeps riding through every step.  Here a job
leaves its slot as soon as it is done and the next waiting job is admitted into that slot while the other rows keep their state
(C ABI: ``er_queue_*`` in include/edgerunner_hip.h).  This module is the host policy only and has no device dependency: it talks
to an *engine* with three methods

    admit(slot0, jobs)   start ``jobs`` (job indices) in the free slots slot0, slot0 + 1, ...
    run() -> [slot, ...] advance every slot until at least one job is done; the slots of ALL done jobs ([] when none is occupied)
    take(slot) -> result hand back the finished job of ``slot`` and free the slot

``edgerunner_amd.models`` holds the engine that drives the HIP library; tests drive the scheduler with a scripted one.
"""
from __future__ import annotations

from collections import deque
from typing import Any, List, Sequence, Tuple


def free_runs(free: Sequence[int]) -> List[Tuple[int, int]]:
    """Maximal runs of consecutive slot numbers in ``free`` as (first slot, length), lowest first."""
    runs: List[Tuple[int, int]] = []
    for s in sorted(free):
        if runs and runs[-1][0] + runs[-1][1] == s:
            runs[-1] = (runs[-1][0], runs[-1][1] + 1)
        else:
            runs.append((s, 1))
    return runs


def list_scheduling_bound(lengths: Sequence[int], slots: int, check_every: int = 1) -> float:
    """Graham's bound on the steps a greedy scheduler needs for jobs of ``lengths`` steps on ``slots`` slots, a job holding its slot
    until the next look (every ``check_every`` steps): sum / slots + (1 - 1 / slots) * max over the rounded-up lengths."""
    if not lengths:
        return 0.0
    up = [-(-int(n) // check_every) * check_every for n in lengths]
    return sum(up) / slots + (1.0 - 1.0 / slots) * max(up)


class QueueScheduler:
    """Jobs are admitted in index order, each into the lowest free slots; jobs that become admissible together go into one
    ``admit`` call per contiguous run of free slots (the first fill of an empty queue is one call over all slots).  After
    ``serve``: ``slot_of[j]`` is the slot job j ran in and ``admissions`` the ``(slot0, [jobs])`` calls in order."""

    def __init__(self, slots: int):
        if slots < 1:
            raise ValueError(f"slots={slots}: at least one slot")
        self.slots = int(slots)
        self.slot_of: List[int] = []
        self.admissions: List[Tuple[int, List[int]]] = []

    def serve(self, engine, n_jobs: int) -> List[Any]:
        """Runs jobs 0 .. n_jobs - 1 through ``engine`` and returns their results in job order."""
        results: List[Any] = [None] * n_jobs
        self.slot_of = [-1] * n_jobs
        self.admissions = []
        waiting = deque(range(n_jobs))
        free = set(range(self.slots))
        job_in = {}
        while waiting or job_in:
            while waiting and free:
                slot0, length = free_runs(free)[0]
                batch = [waiting.popleft() for _ in range(min(length, len(waiting)))]
                engine.admit(slot0, batch)
                self.admissions.append((slot0, batch))
                for i, j in enumerate(batch):
                    free.remove(slot0 + i)
                    job_in[slot0 + i] = j
                    self.slot_of[j] = slot0 + i
            done = list(engine.run())
            if not done:
                raise RuntimeError(f"queue engine reported no finished job while {len(job_in)} are running")
            for s in done:
                if s not in job_in:
                    raise RuntimeError(f"queue engine reported slot {s}, which holds no job")
                results[job_in.pop(s)] = engine.take(s)
                free.add(s)
        return results
