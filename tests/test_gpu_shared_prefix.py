"""Prefix groups end to end (er_set_prefix_groups -> NativeShapeOPT.prefill(prefix_groups=) -> LMM.generate(share_prefix=True) ->
infer.py ER_INFER_SHARE_PREFIX=1) on the 2-layer synthetic model and tests/golden/arae_small.npz, set up as tests/test_gpu_parity.py
sets them up: rows that hold the same cloud read their cond + BOS prefix from the first such row's cache."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LOGIT_TOL = 1e-3          # as tests/test_gpu_parity.py
_CACHE = {}
_ENV = ("ER_NO_GRAPH", "ER_XT", "ER_FORCE_BATCHED")


def make_lmm(precision="fp32"):
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    key = (precision, tuple(os.environ.get(k, "") for k in _ENV))
    if key not in _CACHE:
        opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
        m = LMM(opt, DEV, precision=precision)
        missing, unexpected = m.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        assert not missing and not unexpected
        _CACHE[key] = m
    return _CACHE[key]


def cloud(i, n=4096):
    from edgerunner_amd import weights as W
    return W.synthetic_point_cloud(i, n).to(DEV)


def assert_ids(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert len(got) == len(want), f"{what}: lengths {len(got)}/{len(want)}"
    d = np.nonzero(got != want)[0]
    assert len(d) == 0, f"{what}: token ids diverge at index {d[0]} (got {got[max(0, d[0] - 2):d[0] + 3]}, want {want[max(0, d[0] - 2):d[0] + 3]})"


def gen(lmm, batch, T, **kw):
    _, toks = lmm.generate(batch, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T, **kw)
    return toks


def batch6():
    return torch.cat([cloud(0), cloud(0), cloud(3), cloud(0), cloud(3), cloud(4)])


LEADERS6 = [0, 0, 2, 0, 2, 5]


@pytest.fixture(scope="module")
def runs6():
    """Batch [c0, c0, c3, c0, c3, c4] in exact mode, 96 tokens: unshared, then shared on the same reservation (computed once)."""
    from edgerunner_amd import native
    lmm = make_lmm()
    unshared = gen(lmm, batch6(), 96)
    plan_unshared = lmm.mesh_decoder.plan()
    shared = gen(lmm, batch6(), 96, share_prefix=True)
    plan_shared = lmm.mesh_decoder.plan()
    assert plan_unshared["attn_kernel"] != native.ER_ATTN_SHARED
    return lmm, unshared, shared, plan_shared


def test_prefix_leaders_of_the_batch():
    from edgerunner_amd.models import prefix_leaders
    assert prefix_leaders(batch6()) == LEADERS6


def test_golden_ids_fp32(runs6, gold_small):
    from edgerunner_amd import native
    _, unshared, shared, plan = runs6
    assert plan["attn_kernel"] == native.ER_ATTN_SHARED and plan["merge_launch"] == 1 and plan["batched"] == 1
    for r in (0, 1, 3):
        assert_ids(shared[r], gold_small["ids_min96"][0], f"row {r} (cloud 0) of the shared batch vs the golden ids")
    assert_ids(shared[2], shared[4], "the two cloud-3 rows")
    assert_ids(shared[2], unshared[2], "cloud-3 row, shared vs unshared")
    assert_ids(shared[5], unshared[5], "the singleton, shared vs unshared")


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_shared_equals_unshared_b18(precision):
    """18 rows of three clouds (groups of 6; streaming attention and, in fast mode, the tiled out_proj forms behind it)."""
    from edgerunner_amd import native
    lmm = make_lmm(precision)
    batch = torch.cat([cloud(i % 3) for i in range(18)])
    ref = gen(lmm, batch, 64)
    assert lmm.mesh_decoder.plan()["attn_kernel"] == native.ER_ATTN_STREAM
    toks = gen(lmm, batch, 64, share_prefix=True)
    assert lmm.mesh_decoder.plan()["attn_kernel"] == native.ER_ATTN_SHARED
    for r in range(18):
        assert_ids(toks[r], ref[r], f"{precision} row {r}: shared vs unshared")
    assert_ids(toks[1], toks[16], "rows 1 and 16 hold the same cloud")
    lmm.mesh_decoder.reserve(1, 4096)


def test_shared_equals_unshared_b6_fast_row_major(monkeypatch):
    monkeypatch.setenv("ER_XT", "0")
    lmm = make_lmm("fp16")
    ref = gen(lmm, batch6(), 64)
    toks = gen(lmm, batch6(), 64, share_prefix=True)
    for r in range(6):
        assert_ids(toks[r], ref[r], f"fp16, ER_XT=0, row {r}: shared vs unshared")
    lmm.mesh_decoder.reserve(1, 4096)


def _teacher_forced(lmm, batch, ids, T, prefix_groups):
    dec, opt = lmm.mesh_decoder, lmm.opt
    B = batch.shape[0]
    cond = lmm.encode_cond(batch, [1000] * B)["cond_embeds"]
    emb = torch.cat((cond, dec.embd(torch.full((B, 1), opt.bos_token_id, dtype=torch.long))), dim=1)
    dec.prefill(emb, T, prefix_groups=prefix_groups)          # T - 1 tokens are fed: the reservation of a T-token generate holds them
    out = []
    for t in range(T):
        out.append(dec.logits().cpu().numpy())
        if t + 1 < T:
            dec.feed([int(ids[t])] * B)
    return np.stack(out)          # [T, B, V]


def test_teacher_forced_logits(runs6, gold_small):
    lmm = runs6[0]
    ids, want = gold_small["ids_min96"][0], gold_small["logits_min96"][:, 0]
    P = lmm.opt.num_cond_tokens + 1
    shared = _teacher_forced(lmm, batch6(), ids, 96, (LEADERS6, P))
    plain = _teacher_forced(lmm, batch6(), ids, 96, None)
    err_gold = max(float(np.abs(shared[:, r] - want).max()) for r in (0, 1, 3))
    err_plain = float(np.abs(shared - plain).max())
    print(f"shared batch of 6, 96 teacher-forced steps: max|dlogit| vs golden {err_gold:.3e}, vs the unshared run {err_plain:.3e}")
    assert err_gold < LOGIT_TOL
    assert err_plain < LOGIT_TOL


def test_eager_launches_give_the_same_ids(runs6, monkeypatch):
    monkeypatch.setenv("ER_NO_GRAPH", "1")
    lmm = make_lmm()          # separate context created with graphs disabled
    toks = gen(lmm, batch6(), 96, share_prefix=True)
    for r in range(6):
        assert_ids(toks[r], runs6[2][r], f"row {r}: eager launches vs the replayed graph")
    lmm.mesh_decoder.reserve(1, 4096)


def test_regrouping_recaptures_the_step(runs6):
    """One reservation: shared, cleared, shared again.  The step graph is captured per grouping: a stale one would replay the other
    attention launches."""
    from edgerunner_amd import native
    lmm, unshared, shared, _ = runs6
    dec = lmm.mesh_decoder
    a = gen(lmm, batch6(), 96, share_prefix=True)
    reserved = dec._reserved
    assert dec.plan()["attn_kernel"] == native.ER_ATTN_SHARED
    b = gen(lmm, batch6(), 96)
    assert dec.plan()["attn_kernel"] != native.ER_ATTN_SHARED
    c = gen(lmm, batch6(), 96, share_prefix=True)
    assert dec.plan()["attn_kernel"] == native.ER_ATTN_SHARED and dec._reserved == reserved
    for r in range(6):
        assert_ids(b[r], unshared[r], f"row {r}: groups cleared vs never set")
        assert_ids(a[r], shared[r], f"row {r}: shared again vs the first shared run")
        assert_ids(c[r], a[r], f"row {r}: shared, cleared, shared")


def test_share_prefix_has_no_effect_below_five_rows(monkeypatch):
    from edgerunner_amd import native
    monkeypatch.delenv("ER_FORCE_BATCHED", raising=False)
    lmm = make_lmm()
    batch = torch.cat([cloud(0), cloud(0)])
    a = gen(lmm, batch, 24, share_prefix=True)
    assert lmm.mesh_decoder.plan()["attn_kernel"] != native.ER_ATTN_SHARED
    b = gen(lmm, batch, 24)
    assert_ids(a[0], b[0], "two rows: share_prefix is ignored")
    lmm.mesh_decoder.reserve(1, 4096)


def test_wrong_groups_are_loud(runs6, gold_small):
    from edgerunner_amd import native
    lmm = runs6[0]
    dec, opt = lmm.mesh_decoder, lmm.opt
    batch = batch6()
    P = opt.num_cond_tokens + 1
    cond = lmm.encode_cond(batch, [1000] * 6)["cond_embeds"]
    emb = torch.cat((cond, dec.embd(torch.full((6, 1), opt.bos_token_id, dtype=torch.long))), dim=1)
    # rows 2, 4 (cloud 3) and 5 (cloud 4) joined to cloud 0's group: the first offender in (row, layer) order is row 2, layer 0
    with pytest.raises(native.NativeError) as e:
        dec.prefill(emb, 96, prefix_groups=([0] * 6, P))
    msg = str(e.value)
    assert "(-1)" in msg and f"first {P} cache positions" in msg and "row 2" in msg and "layer 0" in msg, msg
    with pytest.raises(native.NativeError):          # the failed prefill left no state to decode from
        dec.logits()
    toks = gen(lmm, batch, 96)
    assert_ids(toks[0], gold_small["ids_min96"][0], "ungrouped generate on the same context after the refusal")
    # bad tables and states: ER_ERR_INVALID (-1)
    S = emb.shape[1]
    for groups, why in ((([0, 2, 2, 0, 2, 5], P), "leader[1] > 1"), (([0, 0, 1, 0, 2, 5], P), "a chain: row 1 is led by row 0"),
                        (([0, 0, 2, 0, 2], P), "five leaders for six rows"), ((LEADERS6, S + 1), "P > S")):
        with pytest.raises(native.NativeError) as e:
            dec.prefill(emb, 96, prefix_groups=groups)
        assert "(-1)" in str(e.value), (why, str(e.value))
    dec.set_prefix_groups(None)          # (the last case left its groups set: the prefill refused, not the table)
    dec.queue_begin(6, S + 50, 8)
    try:
        with pytest.raises(native.NativeError) as e:
            dec.set_prefix_groups((LEADERS6, P))
        assert "(-1)" in str(e.value) and "queue" in str(e.value)
    finally:
        dec.queue_end()
    # with groups set the queue and the scorer refuse
    dec.set_prefix_groups((LEADERS6, P))
    with pytest.raises(native.NativeError) as e:
        dec.queue_begin(6, S + 50, 8)
    assert "prefix groups" in str(e.value)
    dec.set_prefix_groups(None)


def test_unsupported_below_the_batched_class(monkeypatch):
    from edgerunner_amd import native
    monkeypatch.delenv("ER_FORCE_BATCHED", raising=False)
    dec = make_lmm().mesh_decoder
    dec.reserve(4, 4096)
    with pytest.raises(native.NativeError) as e:
        dec.set_prefix_groups(([0, 0, 0, 0], 10))
    assert "(-5)" in str(e.value), str(e.value)
    dec.reserve(1, 4096)


# ------------------------------------------------------------------ infer.py
def _run_infer(args, env_extra):
    env = dict(os.environ)
    env.pop("ER_NO_GRAPH", None)
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py")] + [str(a) for a in args], env=env, cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)


def test_infer_py_share_prefix(tmp_path):
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
    p = _run_infer(base + ["--workspace", tmp_path / "both"], {"EDGERUNNER_PRECISION": "fp32", "ER_INFER_SHARE_PREFIX": "1", "ER_INFER_QUEUE": "1"})
    assert p.returncode != 0 and "ER_INFER_SHARE_PREFIX" in p.stdout, p.stdout[-2000:]
    for name, extra in (("plain", {}), ("shared", {"ER_INFER_SHARE_PREFIX": "1"})):
        p = _run_infer(base + ["--workspace", tmp_path / name], {"EDGERUNNER_PRECISION": "fp32", **extra})
        assert p.returncode == 0, p.stdout[-3000:]
        assert "(6 jobs in this call)" in p.stdout, p.stdout[-2000:]
    for i in range(6):
        a, b = (np.load(tmp_path / name / f"a_{i}_1000f_tokens.npy") for name in ("plain", "shared"))
        assert len(a) > 0 and np.array_equal(a, b), (i, a, b)
