"""Prefix groups with the matrix-core prefix pass end to end (er_set_prefix_pass -> NativeShapeOPT.set_prefix_pass ->
LMM.generate(share_prefix="mfma") -> infer.py ER_INFER_PREFIX_PASS=mfma) on the 2-layer synthetic model in fast mode (fp16 weights and
cache), set up as tests/test_gpu_shared_prefix.py sets it up.

Greedy ids of the MFMA-shared run against the unshared run are printed as "rows equal of N", not asserted: the partial sums associate
differently and a near-tie may resolve the other way, as DESIGN.md records for the VALU form.  What is asserted is the plan, the
teacher-forced logits at the file's LOGIT_TOL, and every identity that holds bit for bit (rows of one group, eager against graph,
valu -> mfma -> valu on one reservation)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_shared_prefix import LEADERS6, LOGIT_TOL, _run_infer, _teacher_forced, assert_ids, batch6, cloud, gen, make_lmm  # noqa: E402

pytestmark = pytest.mark.gpu


def rows_equal(a, b):
    return sum(int(np.array_equal(np.asarray(x), np.asarray(y))) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def runs6():
    """Batch [c0, c0, c3, c0, c3, c4] in fast mode, 96 tokens, on one reservation: unshared, shared (VALU pass), shared (MFMA pass),
    with the plan each call left (computed once)."""
    lmm = make_lmm("fp16")
    dec = lmm.mesh_decoder
    out = {}
    for name, kw in (("plain", {}), ("valu", {"share_prefix": True}), ("mfma", {"share_prefix": "mfma"})):
        out[name] = (gen(lmm, batch6(), 96, **kw), dec.plan(), dec._reserved)
    print(f"fast mode, 6 rows, 96 greedy tokens: mfma-shared vs unshared {rows_equal(out['mfma'][0], out['plain'][0])} rows equal of 6, "
          f"vs valu-shared {rows_equal(out['mfma'][0], out['valu'][0])} of 6")
    return lmm, out


def test_plan_reports_the_prefix_pass(runs6):
    from edgerunner_amd import native
    lmm, out = runs6
    plan = out["mfma"][1]
    assert plan["attn_kernel"] == native.ER_ATTN_SHARED_MFMA and plan["merge_launch"] == 1 and plan["batched"] == 1, plan
    assert out["valu"][1]["attn_kernel"] == native.ER_ATTN_SHARED and out["valu"][1]["merge_launch"] == 1
    assert out["plain"][1]["attn_kernel"] not in (native.ER_ATTN_SHARED, native.ER_ATTN_SHARED_MFMA)
    assert lmm.mesh_decoder.prefix_pass == "valu"          # share_prefix="mfma" is scoped to its call
    gen(lmm, batch6(), 8, share_prefix=True)               # True after "mfma": today's meaning, the context's own (VALU) pass
    assert lmm.mesh_decoder.plan()["attn_kernel"] == native.ER_ATTN_SHARED
    # the shape-only rule never reports a shared kernel
    shape_only = native.ErDecodePlan()
    native.check(native.load_library().er_plan_decode(6, 16, 96, 1536, 4096, C.byref(shape_only)), "er_plan_decode")
    assert shape_only.attn_kernel not in (native.ER_ATTN_SHARED, native.ER_ATTN_SHARED_MFMA)


def test_rows_of_one_cloud_within_the_batch(runs6):
    toks = runs6[1]["mfma"][0]
    assert_ids(toks[0], toks[1], "rows 0 and 1 hold cloud 0")
    assert_ids(toks[0], toks[3], "rows 0 and 3 hold cloud 0")
    assert_ids(toks[2], toks[4], "rows 2 and 4 hold cloud 3")


def test_teacher_forced_logits(runs6, gold_small):
    lmm = runs6[0]
    dec = lmm.mesh_decoder
    ids = gold_small["ids_min96"][0]
    P = lmm.opt.num_cond_tokens + 1
    plain = _teacher_forced(lmm, batch6(), ids, 96, None)
    valu = _teacher_forced(lmm, batch6(), ids, 96, (LEADERS6, P))
    dec.set_prefix_pass("mfma")
    try:
        mfma = _teacher_forced(lmm, batch6(), ids, 96, (LEADERS6, P))
        from edgerunner_amd import native
        assert dec.plan()["attn_kernel"] == native.ER_ATTN_SHARED_MFMA
    finally:
        dec.set_prefix_pass("valu")
    err_plain, err_valu = float(np.abs(mfma - plain).max()), float(np.abs(mfma - valu).max())
    print(f"mfma-shared batch of 6, 96 teacher-forced steps: max|dlogit| vs the unshared run {err_plain:.3e}, vs the valu-shared run {err_valu:.3e}")
    assert not np.isnan(mfma).any()
    assert err_plain < LOGIT_TOL
    assert err_valu < LOGIT_TOL


def test_rows_of_one_group_b18():
    """18 rows of three clouds, 64 tokens: rows of one cloud give identical ids (groups of 6; the tiled out_proj forms behind it)."""
    from edgerunner_amd import native
    lmm = make_lmm("fp16")
    batch = torch.cat([cloud(i % 3) for i in range(18)])
    ref = gen(lmm, batch, 64)
    toks = gen(lmm, batch, 64, share_prefix="mfma")
    assert lmm.mesh_decoder.plan()["attn_kernel"] == native.ER_ATTN_SHARED_MFMA
    print(f"fast mode, 18 rows of three clouds, 64 greedy tokens: mfma-shared vs unshared {rows_equal(toks, ref)} rows equal of 18")
    for r in range(3, 18):
        assert_ids(toks[r], toks[r % 3], f"rows {r} and {r % 3} hold the same cloud")
    lmm.mesh_decoder.reserve(1, 4096)


def test_eager_launches_give_the_same_ids(runs6, monkeypatch):
    monkeypatch.setenv("ER_NO_GRAPH", "1")
    lmm = make_lmm("fp16")          # separate context created with graphs disabled
    toks = gen(lmm, batch6(), 96, share_prefix="mfma")
    for r in range(6):
        assert_ids(toks[r], runs6[1]["mfma"][0][r], f"row {r}: eager launches vs the replayed graph")
    lmm.mesh_decoder.reserve(1, 4096)


def test_switching_the_pass_recaptures_the_step(runs6):
    """One reservation: valu, mfma, valu.  The step graph is captured per grouping: a stale one would replay the other prefix pass."""
    from edgerunner_amd import native
    lmm, out = runs6
    dec = lmm.mesh_decoder
    a = gen(lmm, batch6(), 96, share_prefix=True)
    reserved = dec._reserved
    assert dec.plan()["attn_kernel"] == native.ER_ATTN_SHARED
    b = gen(lmm, batch6(), 96, share_prefix="mfma")
    assert dec.plan()["attn_kernel"] == native.ER_ATTN_SHARED_MFMA and dec._reserved == reserved
    c = gen(lmm, batch6(), 96, share_prefix=True)
    assert dec.plan()["attn_kernel"] == native.ER_ATTN_SHARED and dec._reserved == reserved
    for r in range(6):
        assert_ids(c[r], a[r], f"row {r}: valu, mfma, valu")
        assert_ids(a[r], out["valu"][0][r], f"row {r}: valu again vs the first valu run")
        assert_ids(b[r], out["mfma"][0][r], f"row {r}: mfma again vs the first mfma run")


def test_env_sets_the_initial_pass(monkeypatch):
    from edgerunner_amd import native
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    from edgerunner_amd import weights as W
    monkeypatch.setenv("ER_PREFIX_PASS", "mfma")
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
    m = LMM(opt, "cuda:0", precision="fp16")
    m.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
    assert m.mesh_decoder.prefix_pass == "mfma"
    gen(m, batch6(), 8, share_prefix=True)
    assert m.mesh_decoder.plan()["attn_kernel"] == native.ER_ATTN_SHARED_MFMA
    m.mesh_decoder.close()


def test_ignored_below_five_rows(monkeypatch):
    from edgerunner_amd import native
    monkeypatch.delenv("ER_FORCE_BATCHED", raising=False)
    lmm = make_lmm("fp16")
    batch = torch.cat([cloud(0), cloud(0)])
    a = gen(lmm, batch, 24, share_prefix="mfma")
    assert lmm.mesh_decoder.plan()["attn_kernel"] not in (native.ER_ATTN_SHARED, native.ER_ATTN_SHARED_MFMA)
    b = gen(lmm, batch, 24)
    assert_ids(a[0], b[0], "two rows: share_prefix='mfma' is ignored")
    with pytest.raises(ValueError):
        gen(lmm, batch, 8, share_prefix="wmma")
    lmm.mesh_decoder.reserve(1, 4096)


def test_exact_mode_refuses_and_stays_usable():
    from edgerunner_amd import native
    lmm = make_lmm()          # exact mode: fp32 cache
    dec = lmm.mesh_decoder
    before = gen(lmm, batch6(), 48, share_prefix=True)
    with pytest.raises(native.NativeError) as e:
        dec.set_prefix_pass("mfma")
    assert "(-5)" in str(e.value) and "fp32 cache" in str(e.value), str(e.value)
    assert dec.prefix_pass == "valu"
    with pytest.raises(native.NativeError) as e:
        gen(lmm, batch6(), 48, share_prefix="mfma")
    assert "(-5)" in str(e.value), str(e.value)
    after = gen(lmm, batch6(), 48, share_prefix=True)
    assert dec.plan()["attn_kernel"] == native.ER_ATTN_SHARED
    for r in range(6):
        assert_ids(after[r], before[r], f"row {r}: the ids before and after the refusal")
    with pytest.raises(ValueError):
        dec.set_prefix_pass("wmma")
    dec.set_prefix_groups(None)
    dec.queue_begin(6, 2200, 8)          # while a queue is open the call is refused, as er_set_prefix_groups is
    try:
        with pytest.raises(native.NativeError) as e:
            dec.set_prefix_pass("valu")
        assert "(-1)" in str(e.value) and "queue" in str(e.value)
    finally:
        dec.queue_end()
    lmm.mesh_decoder.reserve(1, 4096)


def test_infer_py_prefix_pass(tmp_path):
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
    files = {}
    for name, extra in (("plain", {}), ("mfma", {"ER_INFER_SHARE_PREFIX": "1", "ER_INFER_PREFIX_PASS": "mfma"})):
        p = _run_infer(base + ["--workspace", tmp_path / name], {"EDGERUNNER_PRECISION": "fp16", **extra})
        assert p.returncode == 0, p.stdout[-3000:]
        assert "(6 jobs in this call)" in p.stdout, p.stdout[-2000:]
        files[name] = sorted(f for _, _, fs in os.walk(tmp_path / name) for f in fs)
    assert files["plain"] == files["mfma"] and any(f.endswith("_tokens.npy") for f in files["plain"]), files
    same = sum(int(np.array_equal(*(np.load(tmp_path / name / f"a_{i}_1000f_tokens.npy") for name in ("plain", "mfma")))) for i in range(6))
    print(f"infer.py, 6 samples of one cloud, fast mode: mfma-shared vs plain {same} token files equal of 6")
    for i in range(1, 6):          # one group: every sample of the shared run is the same greedy sequence
        a, b = (np.load(tmp_path / "mfma" / f"a_{j}_1000f_tokens.npy") for j in (0, i))
        assert len(a) > 0 and np.array_equal(a, b), (i, a, b)
