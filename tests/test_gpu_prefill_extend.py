"""Prefill with a past on the GPU: ``er_prefill_extend`` / ``er_embed_num_face`` through ``NativeShapeOPT.prefill_extend``,
``LMM.generate_ids(keep_cond=True)`` and ``infer.py`` with ER_INFER_KEEP_COND=1, on the model of the ``gold_small`` golden (ArAE widths,
2 decoder layers, "perturbed" weights of seed 0), in exact, fast and - where marked - kv8 mode.

References: the CPU oracle's one-pass ``decoder_forward`` over [cond, face, BOS, ids[:k]] (float64 in exact mode; fast / kv8 mode on
``round_streamed_weights`` with ``kv_round``, as tests/test_gpu_score.py does), the incremental path (``er_feed``), a fresh context's full
prefill, and the committed golden.  Bounds: the project's LOGIT_TOL = 1e-3 on logits; the extend path may not be further from the oracle
than MARGIN = 4 times the ordinary full prefill's own distance to the same reference."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LOGIT_TOL = 1e-3
MARGIN = 4.0
MODES = ("exact", "fast")
_LMM, _ORACLE = {}, {}


def make_lmm(mode, fresh=False):
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    if fresh or mode not in _LMM:
        opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
        m = LMM(opt, DEV, precision="fp32" if mode == "exact" else "fp16", kv_precision="fp8" if mode == "kv8" else None)
        missing, unexpected = m.mesh_decoder.load_state_iter(W.iter_state_dict(opt, 0, "perturbed"), strict=True)
        assert not missing and not unexpected
        if fresh:
            return m
        _LMM[mode] = m
    return _LMM[mode]


def cloud(i, n=4096):
    from edgerunner_amd import weights as W
    return W.synthetic_point_cloud(i, n)


def past_of(lmm):
    return lmm.opt.num_cond_tokens - 1            # the face-count token is the LAST cond token: everything before it is the cloud's


def new_embeds(lmm, num_faces, ids, B=1):
    """[face(num_faces), BOS, ids ...] as the extend path's inputs [B, 2 + len(ids), hidden]."""
    from edgerunner_amd.utils import quantize_num_faces
    dec = lmm.mesh_decoder
    face = dec.embed_num_face([quantize_num_faces(num_faces)] * B)[:, None, :]
    toks = torch.tensor([[lmm.opt.bos_token_id] + [int(v) for v in ids]] * B)
    return torch.cat((face, dec.embd(toks)), dim=1)


def full_embeds(lmm, pcs, num_faces, ids):
    dec = lmm.mesh_decoder
    B = pcs.shape[0]
    cond = lmm.encode_cond(pcs.to(DEV), [num_faces] * B)["cond_embeds"]
    toks = torch.tensor([[lmm.opt.bos_token_id] + [int(v) for v in ids]] * B)
    return torch.cat((cond, dec.embd(toks)), dim=1)


def oracle_last_logits(mode, num_faces, ids):
    """The reference's logits at the last position of ONE pass over [cond(cloud 0), face, BOS, ids] (computed once per case)."""
    import arae_oracle as O
    from edgerunner_amd import weights as W
    key = (mode, num_faces, tuple(int(v) for v in ids))
    if key not in _ORACLE:
        opt = make_lmm(mode).opt
        sd = W.make_state_dict(opt, 0, "perturbed")
        if mode == "exact":
            sd, kv_round, pc = {k: v.double() for k, v in sd.items()}, None, cloud(0).double()
        else:
            sd, pc = O.round_streamed_weights(sd, torch.float16), cloud(0)
            kv_round = torch.float8_e4m3fn if mode == "kv8" else torch.float16
        cond = O.encode_cond(sd, opt, pc, torch.tensor([num_faces]))
        toks = torch.tensor([[opt.bos_token_id] + [int(v) for v in ids]])
        emb = F.embedding(toks, sd["mesh_decoder.model.embd.weight"])
        logits, _ = O.decoder_forward(sd, opt, inputs_embeds=torch.cat((cond, emb), dim=1), kv_round=kv_round)
        _ORACLE[key] = logits[0, -1].double()
    return _ORACLE[key]


class route:
    """ER_EXTEND_ATTN for the calls inside (the library reads it per call)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("ER_EXTEND_ATTN")
        if self.value is None:
            os.environ.pop("ER_EXTEND_ATTN", None)
        else:
            os.environ["ER_EXTEND_ATTN"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("ER_EXTEND_ATTN", None)
        else:
            os.environ["ER_EXTEND_ATTN"] = self.old


def dist(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def greedy(dec, B, T):
    from edgerunner_amd import native
    return dec._decode_device(B, T, T, False, 10, native.ER_GRAMMAR_LR_ABSCO, 0).cpu().numpy()


# ------------------------------------------------------------------ 1. against the oracle, both attention routes
@pytest.mark.parametrize("mode", ["exact", "fast", "kv8"])
@pytest.mark.parametrize("attn", ["rows", "flash"])
def test_extend_vs_oracle(gold_small, mode, attn):
    """A full prefill at 1000 faces leaves the past; the extend at 4000 faces with 9 teacher-forced ids behind it must land where the
    oracle's single pass over the whole sequence lands - through either attention route (kv8 + flash goes through the K/V gather)."""
    lmm = make_lmm(mode)
    dec = lmm.mesh_decoder
    ids = gold_small["ids_pc1_f4000"][0][:9]
    ref = oracle_last_logits(mode, 4000, ids)
    pc = cloud(0)
    dec.prefill(full_embeds(lmm, pc, 4000, ids), 8)
    d_full = dist(dec.logits()[0], ref)
    dec.prefill(full_embeds(lmm, pc, 1000, []), 32)
    with route(attn):
        dec.prefill_extend(new_embeds(lmm, 4000, ids), past_of(lmm))
    d_ext = dist(dec.logits()[0], ref)
    print(f"{mode} / {attn}: max|dlogit| vs the oracle: extend {d_ext:.3e}, full prefill {d_full:.3e}")
    assert d_ext < LOGIT_TOL and d_full < LOGIT_TOL
    assert d_ext <= MARGIN * d_full, "the extend path is further from the oracle than 4 x the full prefill: find out why"


# ------------------------------------------------------------------ 2. against the incremental path and the golden
@pytest.mark.parametrize("mode", MODES)
def test_extend_vs_feed_and_golden(gold_small, mode):
    lmm = make_lmm(mode)
    dec = lmm.mesh_decoder
    ids = gold_small["ids_min96"][0]
    pc = cloud(0)
    S = lmm.opt.num_cond_tokens + 1
    dec.prefill(full_embeds(lmm, pc, 1000, []), 130)
    for n in (1, 2, 9, 33):
        dec.prefill_extend(new_embeds(lmm, 1000, []), past_of(lmm))          # back to [cond, BOS]: the state er_prefill left
        for t in range(n):
            dec.feed([int(ids[t])])
        fed = dec.logits()[0].clone()
        dec.prefill_extend(dec.embd(torch.tensor([[int(v) for v in ids[:n]]])), S)      # the same ids as ONE pass behind the same past
        ext = dec.logits()[0]
        d = dist(ext, fed)
        print(f"{mode}: n_new {n}: max|dlogit| extend vs er_feed {d:.3e}")
        assert d < LOGIT_TOL, n
    # the golden's case (1000 faces, no resume) from a past another face count left
    dec.prefill(full_embeds(lmm, pc, 4000, []), 130)
    dec.prefill_extend(new_embeds(lmm, 1000, []), past_of(lmm))
    got = greedy(dec, 1, 96)
    if mode == "exact":
        assert np.array_equal(got[0], ids)
    else:       # fp16 storage: the ids of this mode's own full prefill
        dec.prefill(full_embeds(lmm, pc, 1000, []), 130)
        assert np.array_equal(got, greedy(dec, 1, 96))


# ------------------------------------------------------------------ 3. another face count after a look at the result
@pytest.mark.parametrize("mode", MODES)
def test_new_face_count_after_decode(mode):
    lmm, fresh = make_lmm(mode), make_lmm(mode, fresh=True)
    dec, fdec = lmm.mesh_decoder, fresh.mesh_decoder
    pc = cloud(1)
    fdec.prefill(full_embeds(fresh, pc, 4000, []), 130)
    want_logits = fdec.logits()[0].clone()
    want = greedy(fdec, 1, 96)
    dec.prefill(full_embeds(lmm, pc, 1000, []), 130)
    greedy(dec, 1, 32)
    dec.prefill_extend(new_embeds(lmm, 4000, []), past_of(lmm))
    d = dist(dec.logits()[0], want_logits)
    print(f"{mode}: first-step max|dlogit| extend vs a fresh context's full prefill {d:.3e}")
    assert d < LOGIT_TOL
    assert np.array_equal(greedy(dec, 1, 96), want)
    fresh.mesh_decoder.close()


# ------------------------------------------------------------------ 4. rewinding leaves no trace
@pytest.mark.parametrize("mode", ["exact", "fast", "kv8"])
def test_rewind_is_bit_exact(gold_small, mode):
    lmm = make_lmm(mode)
    dec = lmm.mesh_decoder
    ids = gold_small["ids_min96"][0][:5]
    dec.prefill(full_embeds(lmm, cloud(0), 1000, []), 130)
    x = new_embeds(lmm, 2500, ids)
    plan = dec.plan()
    dec.prefill_extend(x, past_of(lmm))
    l1 = dec.logits().clone()
    g1 = greedy(dec, 1, 64)
    dec.prefill_extend(x, past_of(lmm))
    l2 = dec.logits()
    assert torch.equal(l1, l2)
    assert np.array_equal(greedy(dec, 1, 64), g1)
    assert dec.plan() == plan


# ------------------------------------------------------------------ 5. a batch of the batched class, and prefix groups
@pytest.mark.parametrize("mode", MODES)
def test_batch_rows_match_their_own_run(mode):
    from edgerunner_amd import native
    lmm = make_lmm(mode)
    dec = lmm.mesh_decoder
    pcs = torch.cat([cloud(i, 1024) for i in (0, 0, 2, 3, 4, 5)])           # rows 0 and 1 share a cloud
    ids = [7, 9, 11]
    B = pcs.shape[0]
    dec.prefill(full_embeds(lmm, pcs, 1000, []), 64)
    dec.prefill_extend(new_embeds(lmm, 4000, ids, B), past_of(lmm))
    batch = dec.logits().clone()
    # prefix groups: the shared positions may not be rewritten; at or behind them the call needs no re-check
    S = lmm.opt.num_cond_tokens + 1
    dec.prefill(full_embeds(lmm, pcs, 1000, []), 64, prefix_groups=([0, 0, 2, 3, 4, 5], S))
    with pytest.raises(native.NativeError, match="prefix groups"):
        dec.prefill_extend(new_embeds(lmm, 4000, ids, B), past_of(lmm))
    dec.prefill_extend(dec.embd(torch.tensor([ids] * B)), S)
    assert bool(torch.isfinite(dec.logits()).all())
    dec.set_prefix_groups(None)
    worst = 0.0
    for b in range(B):
        dec.prefill(full_embeds(lmm, pcs[b:b + 1], 1000, []), 64)
        dec.prefill_extend(new_embeds(lmm, 4000, ids), past_of(lmm))
        worst = max(worst, dist(dec.logits()[0], batch[b]))
    print(f"{mode}: B = 6 rows vs each alone: max|dlogit| {worst:.3e}")
    assert worst < LOGIT_TOL


# ------------------------------------------------------------------ 6. refusals, all before any launch
def test_refusals_leave_the_context_usable(gold_small):
    from edgerunner_amd import native
    lmm = make_lmm("exact", fresh=True)
    dec = lmm.mesh_decoder
    pc = cloud(0, 512)
    P = past_of(lmm)
    x = None

    def refused(past, emb=None, code=-1):
        e = x if emb is None else emb
        rc = dec.lib.er_prefill_extend(dec._ctx, native.ptr(e), e.shape[0], past, e.shape[1], None)
        assert rc == code, (rc, dec.lib.er_last_error())

    dec.reserve(1, P + 2 + 40)
    x = new_embeds(lmm, 4000, [])
    refused(P)                                                              # before any prefill
    full = full_embeds(lmm, pc, 1000, [])
    dec.prefill(full, 38)
    S = full.shape[1]
    want = dec.logits().clone()
    refused(0)
    refused(S + 1)                                                          # one past the recorded prefix
    refused(-5)
    refused(P, emb=torch.zeros(2, 2, x.shape[2], device=DEV))               # not the reserved batch
    l_cap = (dec._reserved[1] + 31) // 32 * 32                              # what er_kv_reserve rounds the length to
    refused(P, emb=torch.zeros(1, l_cap - P, x.shape[2], device=DEV), code=-4)      # past_len + n_new == Lcap: ER_ERR_CAPACITY
    assert torch.equal(dec.logits(), want)                                  # nothing ran
    dec.prefill_extend(torch.zeros(1, l_cap - P - 1, x.shape[2], device=DEV), P)    # one less fits; [0, P) stays what it was
    dec.prefill_extend(full[:, P:], P)
    assert dist(dec.logits(), want) < LOGIT_TOL
    dec.prefill_extend(x, P)                                                # and the context is usable
    greedy(dec, 1, 8)
    dec.prefill_extend(x, S)                                                # decoding kept the record: [0, P + 2) is still there
    # a reserve starts over, the same shape included
    dec.reserve(1, dec._reserved[1])
    refused(P)
    dec.prefill(full, 38)
    # a queue takes the rows
    dec.queue_begin(1, dec._reserved[1], 8)
    refused(P)
    dec.queue_end()
    refused(P)                                                              # and leaves nothing behind to extend
    dec.prefill(full, 38)
    dec.prefill_extend(x, P)
    assert bool(torch.isfinite(dec.logits()).all())
    dec.close()


def test_embed_num_face_rows():
    from edgerunner_amd import native
    lmm = make_lmm("exact")
    dec = lmm.mesh_decoder
    cond = lmm.encode_cond(cloud(0, 512).to(DEV), [4000])["cond_embeds"]
    from edgerunner_amd.utils import quantize_num_faces
    assert torch.equal(dec.embed_num_face([quantize_num_faces(4000)])[0], cond[0, -1])
    out = torch.zeros(1, lmm.dims.hidden_dim, device=DEV)
    assert dec.lib.er_embed_num_face(dec._ctx, native.i32_array([99]), 1, native.ptr(out), None) == -1


# ------------------------------------------------------------------ 7. LMM.generate_ids(keep_cond=True)
@pytest.mark.parametrize("mode", MODES)
def test_generate_ids_keep_cond(mode):
    lmm, plain = make_lmm(mode, fresh=True), make_lmm(mode)
    calls = []
    dec = lmm.mesh_decoder
    inner = dec.encode_cond
    dec.encode_cond = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    pcs = torch.cat([cloud(0, 1024), cloud(3, 1024)]).to(DEV)
    kw = dict(tokenizer=object(), max_new_tokens=40, min_new_tokens=40)
    a = lmm.generate_ids(pcs, 1000, keep_cond=True, **kw)
    assert lmm.last_prefill == "full" and len(calls) == 1
    b = lmm.generate_ids(pcs, 4000, keep_cond=True, **kw)
    assert lmm.last_prefill == "extend" and len(calls) == 1, "the second face count must not run the point encoder"
    c = lmm.generate_ids(pcs.clone(), 1000, keep_cond=True, **kw)          # equal bits in another tensor: still the kept prefix
    assert lmm.last_prefill == "extend" and len(calls) == 1
    assert torch.equal(a, plain.generate_ids(pcs, 1000, **kw)) and torch.equal(c, a)
    assert torch.equal(b, plain.generate_ids(pcs, 4000, **kw))
    moved = pcs.clone()
    moved[1, 7, 2] += 0.25
    d = lmm.generate_ids(moved, 4000, keep_cond=True, **kw)                # changed conds: the full path, recorded again
    assert lmm.last_prefill == "full" and len(calls) == 2
    assert torch.equal(d, plain.generate_ids(moved, 4000, **kw))
    lmm.generate_ids(moved, 1000, **kw)                                     # a call without the flag forgets
    lmm.generate_ids(moved, 4000, keep_cond=True, **kw)
    assert lmm.last_prefill == "full"
    with pytest.raises(NotImplementedError, match="fork_prefill"):
        lmm.generate_ids(moved, 1000, keep_cond=True, fork_prefill=True, **kw)
    dec.close()


# ------------------------------------------------------------------ 8. infer.py
def test_infer_py_keep_cond_writes_the_same_files(tmp_path):
    from edgerunner_amd import weights as W
    inp = tmp_path / "inputs"
    inp.mkdir()
    for n, i in (("a", 0), ("b", 3)):
        np.save(inp / f"{n}.npy", W.synthetic_point_cloud(i, 512)[0].numpy())
    outs = {}
    for tag, env in (("plain", {}), ("keep", {"ER_INFER_KEEP_COND": "1"})):
        e = dict(os.environ)
        e.pop("ER_NO_GRAPH", None)
        e.update(env)
        out = tmp_path / tag
        p = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "ArAE", "--num_layers", "2", "--test_path", str(inp),
                            "--generate_mode", "greedy", "--test_num_face", "1000", "4000", "--test_max_seq_length", "64", "--workspace", str(out)],
                           env=e, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-3000:]
        outs[tag] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out)) if f.endswith("_tokens.npy")}
    assert sorted(outs["plain"]) == ["a_0_1000f_tokens.npy", "a_0_4000f_tokens.npy", "b_0_1000f_tokens.npy", "b_0_4000f_tokens.npy"]
    assert outs["keep"] == outs["plain"]
    e = dict(os.environ, ER_INFER_KEEP_COND="1", ER_INFER_QUEUE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "ArAE", "--num_layers", "2", "--test_path", str(inp), "--workspace", str(tmp_path / "no")],
                       env=e, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode != 0 and "ER_INFER_KEEP_COND" in p.stdout
