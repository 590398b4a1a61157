"""Teacher-forced scoring on the GPU: ``er_score`` / ``er_point_latent`` / ``er_k_score_rows`` through ``LMM.forward`` (the
reference's eval-mode forward, core/models.py:147-202) against the CPU oracle (oracle/arae_oracle.py, float64 where stated), the
incremental decode path, the committed goldens and ``score.py`` end to end."""
import dataclasses
import json
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
_CACHE = {}


def make_lmm(num_layers=2, seed=0, style="perturbed", precision="fp32"):
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    key = (num_layers, seed, style, precision)
    if key not in _CACHE:
        opt = dataclasses.replace(config_defaults["ArAE"], num_layers=num_layers, generate_mode="greedy")
        m = LMM(opt, DEV, precision=precision)
        missing, unexpected = m.mesh_decoder.load_state_iter(W.iter_state_dict(opt, seed, style), strict=True)
        assert not missing and not unexpected
        _CACHE[key] = m
    return _CACHE[key]


def cloud(i, n=4096):
    from edgerunner_amd import weights as W
    return W.synthetic_point_cloud(i, n)


def item(pc, num_faces, ids):
    ids = np.asarray(ids, dtype=np.int64)
    return {"cond": pc[0].numpy(), "num_faces": num_faces, "coords": ids, "len": len(ids), "azimuth": 0, "path": None}


def oracle_row(sd, opt, pc, num_faces, tokens):
    """Unpadded row through the oracle: logits [S, V] of cat(encode_cond, embd(tokens)) in the dtype of sd."""
    import arae_oracle as O
    cond = O.encode_cond(sd, opt, pc.to(next(iter(sd.values())).dtype), torch.tensor([num_faces]))
    emb = F.embedding(torch.as_tensor(tokens)[None], sd["mesh_decoder.model.embd.weight"])
    logits, _ = O.decoder_forward(sd, opt, inputs_embeds=torch.cat((cond, emb), dim=1))
    return logits[0]


def top2_margin(x):
    t = torch.topk(torch.as_tensor(x), 2, dim=-1).values
    return (t[..., 0] - t[..., 1]).numpy()


@pytest.fixture(scope="module")
def sd64():
    from edgerunner_amd import weights as W
    opt = make_lmm().opt
    return {k: v.double() for k, v in W.make_state_dict(opt, 0, "perturbed").items()}


@pytest.fixture(scope="module")
def ragged(gold_small):
    """Three rows of gold_small id streams, collated at max_seq_length 150: row 1 (256 ids) is truncated, rows 0 / 2 padded."""
    from edgerunner_amd.provider import collate_fn
    lmm = make_lmm()
    opt = dataclasses.replace(lmm.opt, max_seq_length=150)
    pc = cloud(0, 2048)
    items = [item(pc, 1000, gold_small["ids_min96"][0]), item(pc, 2500, gold_small["ids_natural"][0]),
             item(pc, 4000, gold_small["ids_pc1_f4000"][0])]
    data = collate_fn(items, opt)
    C = opt.num_cond_tokens
    assert data["masks"].sum(1).tolist() == [C + 98, C + 151, C + 50] and data["masks"].shape[1] == C + 152
    return items, data, pc


# ------------------------------------------------------------------ 1. small config, exact mode, ragged batch
def test_ragged_batch_vs_float64_oracle(ragged, sd64):
    lmm = make_lmm()
    items, data, pc = ragged
    C = lmm.opt.num_cond_tokens
    out = lmm.score(data)
    logits = out["logits"].cpu()
    nll_sum, n_sup, worst, checked, ties = 0.0, 0, 0.0, 0, 0
    for b in range(3):
        L = int(data["masks"][b].sum())
        ref = oracle_row(sd64, lmm.opt, pc.double(), items[b]["num_faces"], data["tokens"][b, : L - C])
        lab = data["labels"][b, :L]
        nll_sum += float(F.cross_entropy(ref[:-1], lab[1:], ignore_index=-100, reduction="sum"))
        n_sup += int((lab[1:] != -100).sum())
        worst = max(worst, float((logits[b, :L].double() - ref).abs().max()))
        margin = top2_margin(ref.float())
        sure = margin > 1e-3
        got_pred = out["pred"][b, :L].cpu().numpy()
        assert np.array_equal(got_pred[sure], ref.argmax(-1).numpy()[sure]), b
        checked += int(sure.sum())
        ties += int((~sure).sum())
    want = nll_sum / n_sup
    got = float(out["loss_ce"])
    print(f"loss_ce {got:.8f} vs float64 oracle {want:.8f} (rel {abs(got - want) / want:.2e}); max|dlogit| {worst:.3e}; "
          f"argmax checked at {checked} positions, {ties} near-ties skipped")
    assert abs(got - want) <= 1e-5 * want
    assert worst < LOGIT_TOL
    assert "pred" not in lmm.forward(data) and set(lmm(data)) == {"loss_ce", "loss_kl", "loss", "logits", "nll"}


# ------------------------------------------------------------------ 2. rows are independent
def test_rows_scored_alone_match_the_batch(ragged):
    from edgerunner_amd.provider import collate_fn
    lmm = make_lmm()
    items, data, _ = ragged
    opt = dataclasses.replace(lmm.opt, max_seq_length=150)
    batch_nll = lmm.forward(data)["nll"].cpu().numpy()
    worst = 0.0
    for b in range(3):
        alone = lmm.forward(collate_fn([items[b]], opt))["nll"].cpu().numpy()[0]
        L = int(data["masks"][b].sum())
        d = np.abs(batch_nll[b, :L] - alone[:L])
        worst = max(worst, float((d / (1.0 + np.abs(alone[:L]))).max()))
    print(f"max |nll(batch) - nll(alone)| / (1 + |nll|) = {worst:.2e}")
    assert worst <= 1e-6


# ------------------------------------------------------------------ 3. agreement with the incremental path and the golden
def test_scored_logits_match_teacher_forced_decode(gold_small):
    from edgerunner_amd.provider import collate_fn
    lmm = make_lmm()
    ids = gold_small["ids_min96"][0]
    pc = cloud(0)
    data = collate_fn([item(pc, 1000, ids)], lmm.opt)
    C = lmm.opt.num_cond_tokens
    got = lmm.forward(data)["logits"][0, C: C + 96].cpu().numpy()           # position C + t predicts ids[t]
    dec = lmm.mesh_decoder
    cond = lmm.encode_cond(pc.to(DEV), [1000])["cond_embeds"]
    dec.prefill(torch.cat((cond, dec.embd(torch.full((1, 1), lmm.opt.bos_token_id))), dim=1), 98)
    inc = []
    for t in range(96):
        inc.append(dec.logits().cpu().numpy()[0])
        if t < 95:
            dec.feed([int(ids[t])])
    inc = np.stack(inc)
    gold = gold_small["logits_min96"][:, 0]
    e_inc, e_gold = float(np.abs(got - inc).max()), float(np.abs(got - gold).max())
    print(f"scored vs er_feed logits {e_inc:.3e}, vs golden {e_gold:.3e}")
    assert e_inc < LOGIT_TOL and e_gold < LOGIT_TOL


# ------------------------------------------------------------------ 4. full depth against the reference's own run
def test_full_depth_against_gold_full(gold_full):
    from edgerunner_amd import native
    from edgerunner_amd.grammar import GrammarState
    from edgerunner_amd.provider import collate_fn
    lmm = make_lmm(num_layers=24)
    ids = gold_full["ids"][0]
    T = len(ids)
    C = lmm.opt.num_cond_tokens
    data = collate_fn([item(cloud(0), 1000, ids)], lmm.opt)
    data = {k: (v[:, : C + 1 + T] if k in ("labels", "masks") else v) for k, v in data.items()}
    data["tokens"] = data["tokens"][:, : 1 + T]                           # [cond, BOS, ids[:4000]]: S = 6050
    out = lmm.forward(data)
    logits = out["logits"][0].cpu()
    assert logits.shape[0] == C + 1 + T == 6050
    steps = gold_full["logit_steps"]
    err = float((logits[C + torch.as_tensor(steps)] - torch.as_tensor(gold_full["logits"][:, 0])).abs().max())
    st, last, ties, eos = GrammarState(native.ER_GRAMMAR_LR_ABSCO, lmm.vocab_size), None, 0, lmm.opt.eos_token_id
    for t in range(T):
        s = torch.full((lmm.vocab_size,), -float("inf"))
        allowed = [a for a in st.allowed(last) if a != eos]
        s[allowed] = logits[C + t, allowed]
        top = torch.topk(s, 2).values
        if float(top[0] - top[1]) > 1e-3:
            assert int(s.argmax()) == int(ids[t]), f"step {t}"
        else:
            ties += 1
        last = int(ids[t])
    print(f"24 layers, S = 6050: max|dlogit| at {len(steps)} golden steps {err:.3e}; grammar-masked argmax = golden id at every "
          f"decided step, {ties} near-ties; loss_ce {float(out['loss_ce']):.6f}")
    assert err < LOGIT_TOL


# ------------------------------------------------------------------ 5. the context after er_score is the one er_prefill leaves
def test_decode_after_score_equals_decode_after_prefill(gold_small):
    from edgerunner_amd import native
    lmm = make_lmm()
    T = 96
    want = lmm.generate_ids(cloud(0).to(DEV), 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T).cpu().numpy()
    dec = lmm.mesh_decoder
    cond = lmm.encode_cond(cloud(0).to(DEV), [1000])["cond_embeds"]
    emb = torch.cat((cond, dec.embd(torch.full((1, 1), lmm.opt.bos_token_id))), dim=1)
    dec.reserve(1, emb.shape[1] + T + 1)
    dec.score(emb, torch.full((1, emb.shape[1]), -100, dtype=torch.int32))
    got = dec._decode_device(1, T, T, False, 10, native.ER_GRAMMAR_LR_ABSCO, 0).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], gold_small["ids_min96"][0])


# ------------------------------------------------------------------ 6. fast mode
def test_fast_mode_vs_storage_rounding_emulation(gold_small):
    import arae_oracle as O
    from edgerunner_amd import weights as W
    from edgerunner_amd.provider import collate_fn
    lmm = make_lmm(precision="fp16")
    sd16 = O.round_streamed_weights(W.make_state_dict(lmm.opt, 0, "perturbed"), torch.float16)
    ids = gold_small["ids_min96"][0]
    pc = cloud(0, 2048)
    data = collate_fn([item(pc, 1000, ids)], lmm.opt)
    out = lmm.forward(data)
    cond = O.encode_cond(sd16, lmm.opt, pc, torch.tensor([1000]))
    emb = F.embedding(data["tokens"], sd16["mesh_decoder.model.embd.weight"])
    ref, _ = O.decoder_forward(sd16, lmm.opt, inputs_embeds=torch.cat((cond, emb), dim=1), kv_round=torch.float16)
    want = float(F.cross_entropy(ref[0, :-1].double(), data["labels"][0, 1:], ignore_index=-100))
    err = float((out["logits"][0].cpu() - ref[0]).abs().max())
    got = float(out["loss_ce"])
    print(f"fast mode: max|dlogit| vs fp16-storage emulation {err:.3e}; loss_ce {got:.6f} vs {want:.6f} "
          f"(rel {abs(got - want) / want:.2e})")
    assert err < LOGIT_TOL
    assert abs(got - want) <= 1e-3 * want


# ------------------------------------------------------------------ 7. the point latent and its KL term
def test_point_latent_kl_and_total_loss(ragged):
    import arae_oracle as O
    from edgerunner_amd import weights as W
    lmm = make_lmm()
    sd = W.make_state_dict(lmm.opt, 0, "perturbed")
    pcs = torch.cat([cloud(0, 1024), cloud(3, 1024)])
    lat, kl = lmm.mesh_decoder.point_latent(pcs.to(DEV))
    ref = O.point_encoder_embed(sd, pcs, lmm.opt.point_num_heads)
    err = float((lat.cpu() - ref).abs().max())
    kl64 = 0.5 * float((lat.double() ** 2).sum())
    print(f"latent max abs err {err:.3e}; kl {float(kl):.8e} vs float64 {kl64:.8e}")
    assert tuple(lat.shape) == (2, lmm.opt.point_latent_size, lmm.opt.point_latent_dim) and err <= 2e-4
    assert abs(float(kl) - kl64) <= 1e-6 * kl64
    _, data, _ = ragged
    out = lmm.forward(data)
    assert torch.equal(out["loss"], out["loss_ce"] + lmm.opt.kl_weight * out["loss_kl"])
    _, kl3 = lmm.mesh_decoder.point_latent(data["conds"].to(DEV))
    assert torch.equal(out["loss_kl"], kl3)


# ------------------------------------------------------------------ 8. the row kernel on its own
@pytest.mark.parametrize("V", [518, 1030, 77])
def test_score_rows_kernel(V):
    from edgerunner_amd import kernels as K
    g = torch.Generator().manual_seed(V)
    B, S = 3, 67
    x = (torch.rand((B, S, V), generator=g) * 2 - 1) * torch.tensor([1.0, 1e4, 30.0]).view(B, 1, 1)
    x[0, 5, 7] = x[0, 5, 300 % V] = x[0, 5].max() + 1.0                   # exact ties: the lowest index wins
    x[1, 9, :] = 2.5                                                        # a constant row: index 0
    labels = torch.randint(0, V, (B, S), generator=g)
    labels[:, ::5] = -100
    labels[2] = -100                                                        # an all-ignored row
    nll, pred, loss = K.score_rows(x.to(DEV), labels)
    lp = torch.log_softmax(x.double(), dim=-1)
    tgt = torch.cat((labels[:, 1:], torch.full((B, 1), -100)), dim=1)
    sup = tgt != -100
    ref = torch.zeros((B, S), dtype=torch.float64)
    ref[sup] = -lp[sup, tgt[sup]]
    d = (nll.cpu().double() - ref).abs()
    assert float((d / (1e-5 + 2e-6 * ref.abs())).max()) <= 1.0, float(d.max())
    assert (nll.cpu()[~sup] == 0).all()
    assert torch.equal(pred.cpu().long(), torch.as_tensor(np.argmax(x.numpy(), axis=-1)))
    assert int(pred[0, 5]) == 7 and int(pred[1, 9]) == 0
    want = float(ref[sup].mean())
    assert int(loss[1]) == int(sup.sum()) and abs(float(loss[0]) - want) <= 1e-6 * abs(want)
    nll2, pred2, loss2 = K.score_rows(x.to(DEV), labels)
    assert torch.equal(nll, nll2) and torch.equal(pred, pred2) and torch.equal(loss, loss2)
    _, _, none = K.score_rows(x.to(DEV), torch.full((B, S), -100))
    assert torch.isnan(none[0]) and float(none[1]) == 0


# ------------------------------------------------------------------ 9. error paths
def test_error_paths(ragged):
    import ctypes as C
    from edgerunner_amd import native
    lmm = make_lmm()
    dec = lmm.mesh_decoder
    dec.reserve(1, 64)
    x = torch.zeros((1, 64, 1536), device=DEV)
    lab = torch.full((1, 64), -100, dtype=torch.int32, device=DEV)
    nll = torch.empty((1, 64), device=DEV)
    loss = torch.empty((2,), device=DEV)
    rc = dec.lib.er_score(dec._ctx, native.ptr(x), native.ptr(lab), 1, 64, native.ptr(nll), None, None, native.ptr(loss),
                          C.c_void_p(0))
    assert rc == -4 and b"does not fit" in dec.lib.er_last_error()                      # ER_ERR_CAPACITY: S >= Lcap
    _, data, _ = ragged
    short = dict(data, labels=data["labels"][:, :-1], masks=data["masks"][:, :-1])
    with pytest.raises(ValueError, match="cond tokens"):
        lmm.forward(short)
    left = dict(data, masks=data["masks"].flip(1).clone())
    with pytest.raises(ValueError, match="right padding"):
        lmm.forward(left)
    bad = dict(data, labels=data["labels"].clone())
    bad["labels"][0, -1] = 7                                                            # a label under the mask-0 padding
    with pytest.raises(ValueError, match="-100"):
        lmm.forward(bad)
    lmm.train()
    try:
        with pytest.raises(NotImplementedError):
            lmm.forward(data)
    finally:
        lmm.eval()


# ------------------------------------------------------------------ 10. score.py end to end
def _write_mesh(path, verts, faces):
    with open(path, "w") as fh:
        for p in verts:
            fh.write(f"v {p[0]} {p[1]} {p[2]}\n")
        for f in faces:
            fh.write(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}\n")


def test_score_py_end_to_end(tmp_path):
    from safetensors.torch import save_file
    from edgerunner_amd import weights as W
    from edgerunner_amd.meto import get_tokenizer
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import parse_cli
    from edgerunner_amd.provider import collate_fn, mesh_item
    opt0 = make_lmm().opt
    sd = W.make_state_dict(opt0, 0, "perturbed")
    ckpt = str(tmp_path / "arae_2layers.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, ckpt)
    meshes = tmp_path / "meshes"
    meshes.mkdir()
    box = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * 0.5
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    _write_mesh(meshes / "box.obj", box, [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    tet = np.array([[0, 0, 0.8], [0.7, 0, -0.4], [-0.35, 0.6, -0.4], [-0.35, -0.6, -0.4]])
    _write_mesh(meshes / "tet.obj", tet, [(0, 1, 2), (0, 2, 3), (0, 3, 1), (1, 3, 2)])
    args = ["ArAE", "--num_layers", "2", "--resume", ckpt, "--test_path", str(meshes), "--workspace", str(tmp_path / "out"),
            "--batch_size", "2", "--point_num", "1024"]
    env = dict(os.environ, EDGERUNNER_PRECISION="fp32")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "score.py")] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:]
    res = json.load(open(tmp_path / "out" / "scores.json"))
    assert len(res["meshes"]) == 2 and res["precision"] == "fp32"
    for m in res["meshes"]:
        assert m["supervised"] > 0 and all(np.isfinite(m[k]) for k in ("loss_ce", "perplexity", "accuracy"))
    # the same batch through LMM.forward in this process
    opt = parse_cli(args)
    lmm = LMM(opt, DEV, precision="fp32")
    lmm.load_state_dict(sd, strict=True)
    tok, _ = get_tokenizer(opt)
    data = collate_fn([mesh_item(str(meshes / n), opt, tok) for n in ("box.obj", "tet.obj")], opt)
    want = float(lmm.forward(data)["loss_ce"])
    print(p.stdout[-600:])
    assert res["mean"]["loss_ce_tokens"] == pytest.approx(want, rel=1e-7)
