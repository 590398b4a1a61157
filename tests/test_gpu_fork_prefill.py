"""The forked prefill end to end (er_prefill_fork -> NativeShapeOPT.prefill_fork -> LMM.generate(fork_prefill=True) -> infer.py
ER_INFER_FORK_PREFILL=1) on the 2-layer synthetic model, set up as tests/test_gpu_shared_prefix.py sets it up: every distinct input of
a batch is encoded and prefilled once, its repeats start from a copy of that row's cache rows and last hidden state.

Batch [c0, c0, c3, c0, c3, c4]: the plan is order [0, 2, 5, 1, 3, 4], leaders [0, 1, 2, 0, 0, 1], three leaders.

What is asserted bit for bit: a follower against its leader (logits right after the prefill, ids), and in exact mode the forked run
against the unforked one row for row.  Both exact-mode passes run under prefix groups (no GEMV tail), 3 and 6 samples take no key
split in the causal attention, and the fp32 GEMMs accumulate k in one order whatever the tile, so a row's bits do not depend on the rows
beside it: measured on the MI355X, the assertion holds (greedy and sample mode, 6 rows equal of 6).  In fast mode the Linears of the
prefill pick their kernel by the row count of the pass (3 rows against 6), so ids against the unforked run are printed as
"rows equal of 6", not asserted - the convention of tests/test_gpu_shared_prefix_mfma.py - and the first logits are held to LOGIT_TOL."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_shared_prefix import LOGIT_TOL, _run_infer, assert_ids, batch6, cloud, gen, make_lmm  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ORDER6, FORK6, N_LEADERS6 = [0, 2, 5, 1, 3, 4], [0, 1, 2, 0, 0, 1], 3
T = 96


def rows_equal(a, b):
    return sum(int(np.array_equal(np.asarray(x), np.asarray(y))) for x, y in zip(a, b))


def embeds_of(lmm, batch):
    dec, opt = lmm.mesh_decoder, lmm.opt
    n = batch.shape[0]
    cond = lmm.encode_cond(batch, [1000] * n)["cond_embeds"]
    return torch.cat((cond, dec.embd(torch.full((n, 1), opt.bos_token_id, dtype=torch.long))), dim=1)


def raw_fork(dec, emb, leaders, n=None):
    """er_prefill_fork itself, without the wrapper's reserve / group calls in front: the status code."""
    from edgerunner_amd import native
    emb = emb.contiguous()
    torch.cuda.synchronize()
    rc = dec.lib.er_prefill_fork(dec._ctx, native.ptr(emb), emb.shape[0], emb.shape[1], native.i32_array(leaders),
                                 len(leaders) if n is None else n, native.stream_ptr(None))
    torch.cuda.synchronize()
    return rc


def test_plan_of_the_batch():
    from edgerunner_amd.models import fork_plan
    assert fork_plan(batch6()) == (ORDER6, FORK6, N_LEADERS6)


# ------------------------------------------------------------------ fast mode
@pytest.fixture(scope="module")
def fast6():
    lmm = make_lmm("fp16")
    plain = gen(lmm, batch6(), T)
    forked = gen(lmm, batch6(), T, fork_prefill=True)
    print(f"fast mode, 6 rows, {T} greedy tokens: forked vs unforked prefill {rows_equal(forked, plain)} rows equal of 6")
    return lmm, plain, forked


def test_fast_mode_rows_of_one_cloud(fast6):
    _, plain, forked = fast6
    assert len(forked) == 6 and all(len(t) == T for t in forked)
    assert_ids(forked[1], forked[0], "rows 0 and 1 hold cloud 0")
    assert_ids(forked[3], forked[0], "rows 0 and 3 hold cloud 0")
    assert_ids(forked[4], forked[2], "rows 2 and 4 hold cloud 3")
    assert not np.array_equal(forked[0], forked[2]) and not np.array_equal(forked[0], forked[5]), "the clouds give different meshes"


def test_fast_mode_first_logits(fast6):
    lmm = fast6[0]
    dec = lmm.mesh_decoder
    batch = batch6()
    dec.prefill(embeds_of(lmm, batch), T)
    plain = dec.logits().clone()                                   # caller's row order
    dec.prefill_fork(embeds_of(lmm, batch[ORDER6[:N_LEADERS6]]), FORK6, T)
    forked = dec.logits().clone()                                  # permuted place i = caller's row ORDER6[i]
    assert forked.shape == plain.shape and not torch.isnan(forked).any()
    for i in range(N_LEADERS6, 6):
        assert torch.equal(forked[i], forked[FORK6[i]]), f"place {i}: a follower's first logits are its leader's, bit for bit"
    err = float((forked - plain[ORDER6]).abs().max())
    print(f"fast mode: first logits, forked vs unforked prefill: max|dlogit| {err:.3e}")
    assert err < LOGIT_TOL
    # the state is complete: the forked rows decode on from it
    dec.feed([7] * 6)
    nxt = dec.logits()
    for i in range(N_LEADERS6, 6):
        assert torch.equal(nxt[i], nxt[FORK6[i]]), f"place {i} after one fed token"
    dec.reserve(1, 4096)


# ------------------------------------------------------------------ exact mode
@pytest.fixture(scope="module")
def exact6():
    lmm = make_lmm()
    shared = gen(lmm, batch6(), T, share_prefix=True)
    both = gen(lmm, batch6(), T, share_prefix=True, fork_prefill=True)
    print(f"exact mode, 6 rows, {T} greedy tokens, share_prefix: forked vs unforked prefill {rows_equal(both, shared)} rows equal of 6")
    return lmm, shared, both


def test_exact_mode_ids_equal_the_unforked_run(exact6, gold_small):
    from edgerunner_amd import native
    lmm, shared, both = exact6
    assert lmm.mesh_decoder.plan()["attn_kernel"] == native.ER_ATTN_SHARED
    for r in range(6):
        assert_ids(both[r], shared[r], f"row {r}: share_prefix + fork_prefill vs share_prefix")
    assert_ids(both[0], gold_small["ids_min96"][0], "row 0 (cloud 0) vs the golden ids")


def test_exact_mode_without_share_prefix(exact6):
    lmm, shared, _ = exact6
    forked = gen(lmm, batch6(), T, fork_prefill=True)
    for a, b in ((1, 0), (3, 0), (4, 2)):
        assert_ids(forked[a], forked[b], f"rows {a} and {b} hold one cloud")
    print(f"exact mode, fork_prefill alone vs share_prefix alone: {rows_equal(forked, shared)} rows equal of 6")


def test_no_repeats_takes_the_plain_path(exact6):
    lmm = exact6[0]
    batch = torch.cat([cloud(0), cloud(3), cloud(4)])
    a, b = gen(lmm, batch, 24), gen(lmm, batch, 24, fork_prefill=True)
    for r in range(3):
        assert_ids(b[r], a[r], f"row {r} of a batch without repeats")


def test_sample_mode_streams_follow_the_rows(exact6):
    lmm = exact6[0]
    greedy = lmm.opt
    lmm.opt = dataclasses.replace(greedy, generate_mode="sample")
    try:
        kw = dict(seed=1234, share_prefix=True)
        shared = gen(lmm, batch6(), T, **kw)
        both = gen(lmm, batch6(), T, fork_prefill=True, **kw)
        print(f"exact mode, sample, seed 1234: forked vs unforked prefill {rows_equal(both, shared)} rows equal of 6")
        for r in range(6):
            assert_ids(both[r], shared[r], f"sample mode row {r}: share_prefix + fork_prefill vs share_prefix")
        assert not (np.array_equal(both[0], both[1]) and np.array_equal(both[0], both[3])), "every follower draws from its own stream"
        # a shuffled copy of the batch, every row keeping the stream of its original index: each job gives the ids it gave unshuffled
        perm = [4, 0, 5, 1, 2, 3]
        shuffled = gen(lmm, batch6()[perm], T, fork_prefill=True, row_streams=perm, **kw)
        for i, r in enumerate(perm):
            assert_ids(shuffled[i], both[r], f"shuffled place {i} = original row {r}")
    finally:
        lmm.opt = greedy


def test_logprobs_come_back_in_the_callers_order(exact6):
    lmm = exact6[0]
    gen(lmm, batch6(), 24, share_prefix=True, output_logprobs=True)
    want = {k: v.clone() for k, v in lmm.last_logprobs.items()}
    gen(lmm, batch6(), 24, share_prefix=True, fork_prefill=True, output_logprobs=True)
    got = lmm.last_logprobs
    assert got["model"].shape == (6, 24)
    for k in ("model", "policy"):
        assert torch.equal(got[k][1], got[k][0]) and torch.equal(got[k][4], got[k][2])
        assert torch.equal(got[k], want[k]), k
    gen(lmm, batch6(), 8)          # the controls are back at their defaults
    assert lmm.last_logprobs is None


# ------------------------------------------------------------------ the byte cache, a small batch
def test_byte_cache():
    from edgerunner_amd import native
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
    lmm = LMM(opt, DEV, precision="fp16", kv_precision="fp8")
    missing, unexpected = lmm.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
    assert not missing and not unexpected
    plain = gen(lmm, batch6(), T)
    forked = gen(lmm, batch6(), T, fork_prefill=True)
    assert lmm.mesh_decoder.plan()["attn_kernel"] == native.ER_ATTN_STREAM
    print(f"fp16 weights, e4m3 cache, 6 rows: forked vs unforked prefill {rows_equal(forked, plain)} rows equal of 6")
    for a, b in ((1, 0), (3, 0), (4, 2)):
        assert_ids(forked[a], forked[b], f"byte cache: rows {a} and {b} hold one cloud")
    assert not np.array_equal(forked[0], forked[2])
    lmm.mesh_decoder.close()


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_two_rows_of_one_cloud(precision, monkeypatch):
    """B = 2, the single-row kernel class.  The forked pass is a one-row pass, whose causal attention is key-split in exact mode, the
    unforked one a two-row pass without the split: only the two rows against each other are asserted."""
    monkeypatch.delenv("ER_FORCE_BATCHED", raising=False)
    lmm = make_lmm(precision)
    batch = torch.cat([cloud(0), cloud(0)])
    plain = gen(lmm, batch, 48)
    forked = gen(lmm, batch, 48, fork_prefill=True)
    assert lmm.mesh_decoder.plan()["batched"] == 0
    assert_ids(forked[1], forked[0], f"{precision}: two rows of one cloud")
    print(f"{precision}, 2 rows, 48 tokens: forked vs unforked prefill {rows_equal(forked, plain)} rows equal of 2")
    lmm.mesh_decoder.reserve(1, 4096)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(exact6):
    from edgerunner_amd import native
    lmm, shared, _ = exact6
    dec = lmm.mesh_decoder
    before = gen(lmm, batch6(), T)
    assert dec._reserved[0] == 6
    emb3 = embeds_of(lmm, batch6()[ORDER6[:N_LEADERS6]])
    S, P = emb3.shape[1], lmm.opt.num_cond_tokens + 1
    INVALID = -1

    def refused(rc, *words):
        msg = dec.lib.er_last_error().decode()
        assert rc == INVALID, (rc, msg)
        assert all(w in msg for w in words), msg

    refused(raw_fork(dec, emb3, [0, 0, 2, 0, 2, 5]), "er_prefill_fork", "leaders first")          # a group table that is not leaders-first
    refused(raw_fork(dec, emb3, [0, 1, 2, 3, 0, 1]), "leaders first")                               # a follower led by a follower's place
    refused(raw_fork(dec, emb3, [0, 1, 2, 0, 0, -1]), "leaders first")
    refused(raw_fork(dec, emb3, [0, 1, 2, 0, 0]), "reserved for 6")                                 # five entries for six rows
    refused(raw_fork(dec, emb3, FORK6 + [1]), "reserved for 6")
    with pytest.raises(native.NativeError) as e:     # the wrapper raises what the entry refuses
        dec.prefill_fork(emb3, [0, 0, 2, 0, 2, 5], T)
    assert "(-1)" in str(e.value) and "er_prefill_fork" in str(e.value)
    # prefix groups set to another table
    dec.set_prefix_groups(([0, 1, 2, 0, 0, 2], P))
    refused(raw_fork(dec, emb3, FORK6), "another leader table")
    dec.set_prefix_groups((FORK6, S + 1))            # the same table, a prefix longer than the prefill
    refused(raw_fork(dec, emb3, FORK6), "prefix groups share")
    dec.set_prefix_groups((FORK6, P))                # the same table: allowed
    assert raw_fork(dec, emb3, FORK6) == 0, dec.lib.er_last_error().decode()
    lg = dec.logits()
    assert torch.equal(lg[3], lg[0]) and torch.equal(lg[5], lg[1])
    dec.set_prefix_groups(None)
    # a queue is open
    dec.queue_begin(6, S + 50, 8)
    try:
        refused(raw_fork(dec, emb3, FORK6), "queue")
    finally:
        dec.queue_end()
    after = gen(lmm, batch6(), T)
    for r in range(6):
        assert_ids(after[r], before[r], f"row {r}: a plain generate after the refusals")
    again = gen(lmm, batch6(), T, share_prefix=True, fork_prefill=True)
    for r in range(6):
        assert_ids(again[r], shared[r], f"row {r}: a forked generate after the refusals")
    dec.reserve(1, 4096)


# ------------------------------------------------------------------ infer.py
def test_infer_py_fork_prefill(tmp_path):
    from safetensors.torch import save_file
    from edgerunner_amd import weights as W
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
    ckpt = str(tmp_path / "arae_2layers.safetensors")
    save_file({k: v.contiguous() for k, v in W.make_state_dict(opt, 0, "perturbed").items()}, ckpt)
    inp = tmp_path / "a.npy"
    np.save(inp, W.synthetic_point_cloud(0, 512)[0].numpy())
    base = ["ArAE", "--num_layers", 2, "--resume", ckpt, "--test_path", inp, "--generate_mode", "greedy", "--test_num_face", 1000,
            "--test_repeat", 6, "--test_max_seq_length", 48]
    for name, extra in (("plain", {}), ("forked", {"ER_INFER_FORK_PREFILL": "1"})):
        p = _run_infer(base + ["--workspace", tmp_path / name], {"EDGERUNNER_PRECISION": "fp32", **extra})
        assert p.returncode == 0, p.stdout[-3000:]
        assert "(6 jobs in this call)" in p.stdout, p.stdout[-2000:]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "forked"))
    toks = [np.load(tmp_path / "forked" / f"a_{i}_1000f_tokens.npy") for i in range(6)]
    assert len(toks[0]) > 0
    for i in range(1, 6):
        assert np.array_equal(toks[i], toks[0]), (i, toks[i], toks[0])
