"""Queue mode with repeats admitted by copy (er_queue_admit_copy -> NativeShapeOPT.queue_admit_copy ->
LMM.generate_queue(fork_repeats=True)) on the 2-layer synthetic model of tests/test_gpu_shared_prefix.py.

Nine jobs, three clouds x three repeats, budgets 24 .. 64 with one repeat of each cloud on a budget of its own; EOS is held back
(min_new_tokens = the largest budget), so every job ends at its budget and the schedule is the same with the option on and off.
Six slots (the batched kernel class) and three (the single-row class), exact and fast mode.  The queue's contract is unchanged, so
every comparison of the option on against off is bit for bit: ids (greedy and sample mode) and log-probs."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_shared_prefix import cloud, make_lmm  # noqa: E402

pytestmark = pytest.mark.gpu

CLOUDS = [0, 0, 0, 3, 3, 3, 4, 4, 4]
BUDGETS = [40, 40, 24, 48, 64, 48, 32, 32, 56]
CASES = [("fp32", 6), ("fp32", 3), ("fp16", 6), ("fp16", 3)]


def jobs9(streams=None):
    return [(cloud(c), 1000, None, None if streams is None else streams[j], BUDGETS[j]) for j, c in enumerate(CLOUDS)]


def serve(lmm, slots, fork, **kw):
    _, toks = lmm.generate_queue(jobs9(kw.pop("streams", None)), slots=slots, tokenizer=object(), max_new_tokens=64, min_new_tokens=64,
                                 check_every=8, fork_repeats=fork, **kw)
    return toks, dict(lmm.last_queue_stats), list(lmm.last_queue_admissions), lmm.last_queue_logprobs


def copies_the_schedule_implies(admissions):
    """Inside one admit call every job after the first of its cloud is a copy (face count and resume are the same for all nine)."""
    return sum(len(jobs) - len({CLOUDS[j] for j in jobs}) for _, jobs in admissions)


def sampling(lmm):
    class Swap:
        def __enter__(self):
            self.greedy = lmm.opt
            lmm.opt = dataclasses.replace(lmm.opt, generate_mode="sample")

        def __exit__(self, *exc):
            lmm.opt = self.greedy
    return Swap()


@pytest.mark.parametrize("precision,slots", CASES)
def test_greedy_ids_and_counters(precision, slots):
    lmm = make_lmm(precision)
    off, st_off, adm_off, _ = serve(lmm, slots, False)
    on, st_on, adm_on, _ = serve(lmm, slots, True)
    assert lmm.mesh_decoder.plan()["batched"] == (1 if slots > 4 else 0)
    assert [len(t) for t in off] == BUDGETS
    for j in range(9):
        assert np.array_equal(on[j], off[j]), f"{precision}, {slots} slots: job {j} (cloud {CLOUDS[j]}) with fork_repeats vs without"
    assert np.array_equal(on[0][:24], on[2]) and np.array_equal(on[3][:48], on[4][:48]), "greedy repeats of one cloud agree up to their budgets"
    assert adm_on == adm_off, "the schedule does not depend on the option"
    want = copies_the_schedule_implies(adm_on)
    assert adm_on[0] == (0, list(range(min(slots, 9)))) and want >= (4 if slots == 6 else 2)
    print(f"{precision}, {slots} slots: admissions {adm_on}, forked {st_on['forked']} (schedule: {want}), prefill_ms off {st_off['prefill_ms']:.2f} on {st_on['prefill_ms']:.2f}")
    assert st_on["forked"] == want and st_off["forked"] == 0
    assert st_on["admissions"] == 9 and st_off["admissions"] == 9
    for k in ("steps", "occupied_row_steps", "wait_row_steps", "parked_row_steps"):
        assert st_on[k] == st_off[k], k
    lmm.mesh_decoder.reserve(1, 4096)


@pytest.mark.parametrize("precision,slots", CASES)
def test_sample_mode_ids(precision, slots):
    lmm = make_lmm(precision)
    with sampling(lmm):
        off, _, _, _ = serve(lmm, slots, False, seed=77)
        on, st, _, _ = serve(lmm, slots, True, seed=77)
        moved, _, _, _ = serve(lmm, slots, True, seed=77, streams=[100 + j for j in range(9)])
    assert st["forked"] > 0
    for j in range(9):
        assert np.array_equal(on[j], off[j]), f"{precision}, {slots} slots, sample mode: job {j} with fork_repeats vs without"
    assert not (np.array_equal(on[0][:24], on[1][:24]) and np.array_equal(on[0][:24], on[2])), "the repeats of cloud 0 draw from their own streams"
    assert sum(int(np.array_equal(moved[j], on[j])) for j in range(9)) < 9, "other stream ids, other draws: the copies carry their own ids"
    lmm.mesh_decoder.reserve(1, 4096)


@pytest.mark.parametrize("precision,slots", CASES)
def test_logprobs_are_the_same_bits(precision, slots):
    lmm = make_lmm(precision)
    off, _, _, lp_off = serve(lmm, slots, False, output_logprobs=True)
    on, st, _, lp_on = serve(lmm, slots, True, output_logprobs=True)
    assert st["forked"] > 0 and len(lp_on) == 9
    for j in range(9):
        assert np.array_equal(on[j], off[j]), j
        for k, name in enumerate(("model", "policy")):
            a, b = lp_on[j][k], lp_off[j][k]
            assert a.shape == (BUDGETS[j],) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"job {j}: {name} log-probs"
    lmm.mesh_decoder.reserve(1, 4096)


def test_admit_copy_refusals_on_the_device():
    from edgerunner_amd import native
    lmm = make_lmm()
    dec, opt = lmm.mesh_decoder, lmm.opt
    cond = lmm.encode_cond(cloud(0), [1000])["cond_embeds"]
    emb = torch.cat((cond, dec.embd(torch.full((1, 1), opt.bos_token_id, dtype=torch.long))), dim=1)
    S = emb.shape[1]
    dec.queue_begin(3, S + 40, 16, 16)          # EOS held back: every job ends at its budget
    try:
        with pytest.raises(native.NativeError) as e:          # nothing admitted yet
            dec.queue_admit_copy(0, [1])
        assert "(-1)" in str(e.value) and "fresh" in str(e.value)
        dec.queue_admit(0, emb, [0], [16])
        dec.queue_admit(1, emb, [1], [4])
        with pytest.raises(native.NativeError) as e:
            dec.queue_admit_copy(0, [1])
        assert "(-1)" in str(e.value) and "occupied" in str(e.value)
        with pytest.raises(native.NativeError) as e:
            dec.queue_admit_copy(0, [2, 2])
        assert "(-1)" in str(e.value) and "twice" in str(e.value)
        with pytest.raises(native.NativeError) as e:
            dec.queue_admit_copy(0, [2], budgets=[17])
        assert "(-1)" in str(e.value) and "budget" in str(e.value)
        dec.queue_admit_copy(0, [2], stream_ids=[9], budgets=[12])          # a good copy, behind the refusals
        assert dec.queue_stats()["admissions"] == 3
        assert dec.queue_run() == [1]                                        # four steps: row 1 spent its budget
        short = dec.queue_take(1, 16)
        with pytest.raises(native.NativeError) as e:                         # row 0 has run four steps: no longer a source
            dec.queue_admit_copy(0, [1])
        assert "(-1)" in str(e.value) and "has run a step" in str(e.value)
        assert dec.queue_run() == [2]
        copy = dec.queue_take(2, 16)
        assert dec.queue_run() == [0]
        full = dec.queue_take(0, 16)
        assert len(short) == 4 and len(copy) == 12 and len(full) == 16
        assert np.array_equal(full[:4], short) and np.array_equal(full[:12], copy), "greedy: the copy and its source give one sequence"
    finally:
        dec.queue_end()
        dec.reserve(1, 4096)
