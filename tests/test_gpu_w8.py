"""fp8 mode on the device: e4m3 bytes times 2^e per row for the six decoder matrices of a layer (csrc/er_w8.h).

The mode needs no numerical oracle of its own: an fp8 context computes, bit for bit, what a fast-mode (fp16) context computes on the
checkpoint that tests/w8_ref.py dequantises.  So the quantiser is compared exactly with w8_ref, the byte kernels with the fp16 kernels on
the dequantised matrix (torch.equal), the model with a fast-mode model on the dequantised state dict (torch.equal), and one check
goes straight to the CPU oracle at fast mode's single-row tolerance (ids exact, logits 5e-6)."""
import dataclasses
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w8_ref  # noqa: E402
from test_w8_cpu import crafted_rows  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID, INTER, VOCAB, NPOS = 1536, 6144, 518, 64
HEADS, HD, LCAP = 16, 96, 64
NAN32, NAN16 = 0x7FC00123, 0x7E01               # sentinels: quiet-NaN patterns no kernel produces
# rows of the test matrices: qkv and out_proj at their real sizes (n = 3 k; the fused merge kernel), fc1 / fc2 ragged against every
# rows-per-workgroup in use (8, 24; 2, 4, 6)
ROWS = {"qkv": 3 * HID, "out": HID, "fc1": 1001, "fc2": 501}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


# ---------------------------------------------------------------------------------------------- 1. the quantiser
def quant_source(n, k, dtype):
    w = rnd(n, k, seed=n + k, scale=0.02)
    c = crafted_rows(k, seed=3, dtype=dtype)
    w[: c.shape[0]] = c
    w[c.shape[0]] = -w[c.shape[0]].abs()                       # a row of negative values
    return w.to(dtype)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n,k", [(48, HID), (16, INTER)])
def test_quantiser_equals_the_reference_exactly(n, k, dtype, where):
    from edgerunner_amd import kernels as K
    w = quant_source(n, k, dtype)
    q_ref, e_ref, w16_ref = w8_ref.quantize_rows(w)
    q, e, w16, ws = K.w8_quantize(w.to(DEV) if where == "device" else w, device=DEV)
    assert e.cpu().tolist() == e_ref.tolist()
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, (bad[:4].tolist(), [(float(w[i, j]), int(q[i, j]), int(q_ref[i, j])) for i, j in bad[:4].tolist()])
    assert same_bits(w16.cpu(), w16_ref)                       # -0 stays -0
    assert torch.equal(ws.cpu(), torch.ldexp(torch.ones(n), e_ref))
    assert set(e_ref.tolist()) >= {-15, 7, -10, -9}            # the crafted rows reach both clamps and both sides of a boundary


def test_non_finite_source_is_refused_with_the_keys_name():
    from edgerunner_amd import kernels as K, native
    lmm = fp8_pair().w8
    key = "mesh_decoder.model.layers.1.fc1.weight"
    for poison in (float("nan"), float("inf"), -float("inf")):
        w = rnd(INTER, HID, seed=9, scale=0.02)
        w[4097, 13] = poison
        with pytest.raises(native.NativeError, match=key.replace(".", r"\.")):
            native.load_tensor(lmm.mesh_decoder.lib.er_load_tensor, lmm.mesh_decoder._ctx, key, w)
        with pytest.raises(native.NativeError):
            K.w8_quantize(w[4090:4100].contiguous(), device=DEV)
    # the context is whole again once the real tensor is back
    native.load_tensor(lmm.mesh_decoder.lib.er_load_tensor, lmm.mesh_decoder._ctx, key, fp8_pair().sd[key])
    assert lmm.mesh_decoder.lib.er_finalize_weights(lmm.mesh_decoder._ctx) == 0


# ---------------------------------------------------------------------------------------------- 2. OCP e4m3fn, not fnuz
def test_hardware_decodes_ocp_e4m3fn():
    from edgerunner_amd import kernels as K, native as nat
    codes = [c for c in range(256) if c & 0x7F != 0x7F]
    q = torch.zeros((HID, HID), dtype=torch.uint8)
    e = torch.full((HID,), -15, dtype=torch.int32)
    for r, c in enumerate(codes):
        q[r, (r * 7 + 3) % HID] = c                            # one code per row, at a place of its own (every byte lane of a load)
        e[r] = (r % 23) - 15
    ws = torch.ldexp(torch.ones(HID), e)
    zero = torch.zeros(1, HID, device=DEV)
    y = K.gemv_form_w8(nat.ER_FORM_ROW, nat.ER_EPI_RESID, q.to(DEV), ws.to(DEV), 1, x=torch.ones(1, HID, device=DEV),
                       bias=zero[0], resid=zero, nw=3, rw=1)["y"][0].cpu()
    table = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float32)
    want = torch.zeros(HID)
    want[: len(codes)] = table[codes] * ws[: len(codes)]
    assert torch.equal(y, want), [(hex(codes[i]), float(y[i]), float(want[i])) for i in (y != want).nonzero().flatten().tolist()[:6]]
    i7e, i80 = codes.index(0x7E), codes.index(0x80)
    assert float(y[i7e]) == 448.0 * float(ws[i7e]) and float(y[i80]) == 0.0      # fnuz would read 0x7E as 240 and 0x80 as NaN


# ---------------------------------------------------------------------------------------------- 3. every row form
@functools.lru_cache(maxsize=None)
def data():
    from edgerunner_amd import kernels as K
    d = SimpleNamespace(q={}, ws={}, w16={})
    for i, (name, n) in enumerate(ROWS.items()):
        w = rnd(n, INTER if name == "fc2" else HID, seed=201 + i, scale=0.02)
        w[5] *= 40.0
        w[6] *= 1e-4                                                       # rows of other exponents
        d.q[name], _, d.w16[name], d.ws[name] = K.w8_quantize(w, device=DEV)
    d.bias = {name: rnd(n, seed=211 + i, scale=0.02).to(DEV) for i, (name, n) in enumerate(ROWS.items())}
    d.x = (rnd(4, HID, seed=221) * 2 + 0.3).to(DEV)
    d.lw, d.lb = (1 + 0.1 * rnd(HID, seed=222)).to(DEV), (0.05 * rnd(HID, seed=223)).to(DEV)
    d.att, d.f = rnd(4, HID, seed=224).to(DEV), torch.relu(rnd(4, INTER, seed=225)).to(DEV)
    d.r = {"out": rnd(4, HID, seed=226).to(DEV), "fc2": rnd(4, ROWS["fc2"], seed=227).to(DEV)}
    d.embd, d.posemb = rnd(VOCAB, HID, seed=228).to(DEV), rnd(NPOS, HID, seed=229).to(DEV)
    d.pos, d.tok = [0, LCAP - 1, 5, 17], [0, VOCAB - 1, 7, 300]
    return d


def sentinel_caches(B):
    kc = torch.full((B, HEADS, LCAP, HD), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    q = torch.full((B, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    return kc, kc.clone(), q


def run_pair(name, B, nw, rw, pro="ln"):
    """The same launch through er_k_gemv_form (fp16 dequantised matrix) and er_k_gemv_form_w8 (bytes + scales): two dicts of outputs."""
    from edgerunner_amd import kernels as K, native as nat
    d = data()
    epi = {"qkv": nat.ER_EPI_QKV, "out": nat.ER_EPI_RESID, "fc1": nat.ER_EPI_RELU, "fc2": nat.ER_EPI_RESID}[name]
    outs = []
    for w8 in (False, True):
        kw = dict(bias=d.bias[name], nw=nw, rw=rw)
        if name in ("qkv", "fc1"):
            if pro == "embed":
                kw["embed"] = (d.embd, d.posemb, d.tok[:B], d.pos[:B])
            else:
                kw.update(x=d.x[:B].contiguous(), ln=(d.lw, d.lb))
            kw["return_xnorm"] = True
        else:
            kw.update(x=(d.att if name == "out" else d.f)[:B].contiguous(), resid=d.r[name][:B].contiguous())
        if name == "qkv":
            kc, vc, q = sentinel_caches(B)
            kw["qkv"] = (kc, vc, d.pos[:B], q)
        o = (K.gemv_form_w8(nat.ER_FORM_ROW, epi, d.q[name], d.ws[name], B, **kw) if w8
             else K.gemv_form(nat.ER_FORM_ROW, epi, d.w16[name], B, **kw))
        if name == "qkv":
            o["kc"], o["vc"] = kc, vc
        outs.append(o)
    return outs


def assert_pair_equal(ref, got, what):
    assert set(ref) == set(got), what
    for k in ref:
        assert same_bits(ref[k], got[k]), f"{what}: {k} differs in {int((ref[k].float() != got[k].float()).sum())} places"
        assert k in ("kc", "vc") or not bool(torch.isnan(got[k]).any()), (what, k)


@pytest.mark.parametrize("pro", ["ln", "embed"])
@pytest.mark.parametrize("nw,rw", [(4, 1), (6, 1), (9, 2)])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_qkv_row_forms_equal_the_fp16_kernels(B, nw, rw, pro):
    ref, got = run_pair("qkv", B, nw, rw, pro)
    assert_pair_equal(ref, got, f"qkv B={B} {nw}x{rw} {pro}")
    d = data()
    for c in (got["kc"], got["vc"]):                                        # the fp16 cache is written at pos and nowhere else
        bits = c.view(torch.int16)
        for b in range(B):
            rest = torch.ones(LCAP, dtype=torch.bool)
            rest[d.pos[b]] = False
            assert bool((bits[b][:, rest.to(DEV)] == NAN16).all()) and not bool((bits[b][:, d.pos[b]] == NAN16).any())


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_out_proj_row_form_equals_the_fp16_kernel(B):
    assert_pair_equal(*run_pair("out", B, 3, 1), f"out_proj B={B}")


@pytest.mark.parametrize("nw", [4, 12])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_fc1_row_forms_equal_the_fp16_kernels(B, nw):
    assert_pair_equal(*run_pair("fc1", B, nw, 2), f"fc1 B={B} {nw}x2")


@pytest.mark.parametrize("B,rw", [(1, 6), (1, 4), (1, 2), (2, 2), (3, 2), (4, 2)])
def test_fc2_split_k_row_forms_equal_the_fp16_kernels(B, rw):
    assert_pair_equal(*run_pair("fc2", B, 4, rw), f"fc2 B={B} rw={rw}")


def test_refused_combinations_write_nothing():
    from edgerunner_amd import kernels as K, native as nat
    d = data()
    for B, nw, rw in [(2, 5, 1), (2, 9, 1), (5, 6, 1)]:                      # no such shape; batch 5 has no row form
        kc, vc, q = sentinel_caches(B)
        pos = (d.pos * 2)[:B]
        with pytest.raises(nat.NativeError):
            K.gemv_form_w8(nat.ER_FORM_ROW, nat.ER_EPI_QKV, d.q["qkv"], d.ws["qkv"], B, x=(rnd(B, HID, seed=1) + 0).to(DEV), ln=(d.lw, d.lb),
                           bias=d.bias["qkv"], nw=nw, rw=rw, qkv=(kc, vc, pos, q))
        for t, s in ((kc, NAN16), (vc, NAN16), (q, NAN32)):
            assert bool((t.view(torch.int16 if s == NAN16 else torch.int32) == s).all())
    with pytest.raises(nat.NativeError):                                      # fc2 with 6 rows per workgroup is a one-row form
        K.gemv_form_w8(nat.ER_FORM_ROW, nat.ER_EPI_RESID, d.q["fc2"], d.ws["fc2"], 2, x=d.f[:2].contiguous(), resid=d.r["fc2"][:2].contiguous(),
                       bias=d.bias["fc2"], nw=4, rw=6)
    with pytest.raises(nat.NativeError):                                      # the batched forms stream the fp16 copy, never the bytes
        K.gemv_form_w8(nat.ER_FORM_VALU, nat.ER_EPI_RELU, d.q["fc1"], d.ws["fc1"], 5, x=(rnd(5, HID, seed=2) + 0).to(DEV), ln=(d.lw, d.lb),
                       bias=d.bias["fc1"])
    with pytest.raises(nat.NativeError):                                      # the lm_head is not quantised
        K.gemv_form_w8(nat.ER_FORM_ROW, nat.ER_EPI_STORE, d.q["fc1"], d.ws["fc1"], 1, x=d.x[:1].contiguous(), ln=(d.lw, d.lb), nw=4, rw=1)


# ---------------------------------------------------------------------------------------------- 4. merge + out_proj, version 3
@pytest.mark.parametrize("length", [1, 17, 300])
def test_outproj3_w8_equals_outproj3_on_the_dequantised_matrix(length):
    from edgerunner_amd import kernels as K
    d = data()
    lcap = 320
    q = rnd(HID, seed=301).to(DEV)
    kc, vc = rnd(HEADS, lcap, HD, seed=302).half().to(DEV), rnd(HEADS, lcap, HD, seed=303).half().to(DEV)
    resid = rnd(HID, seed=304).to(DEV)
    ref = K.attn_outproj3(q, kc, vc, length, d.w16["out"], d.bias["out"], resid)
    got = K.attn_outproj3_w8(q, kc, vc, length, d.q["out"], d.ws["out"], d.bias["out"], resid)
    assert same_bits(ref, got) and bool(torch.isfinite(got).all()), int((ref != got).sum())


# ---------------------------------------------------------------------------------------------- 5. end to end
@functools.lru_cache(maxsize=None)
def fp8_pair():
    """A 2-layer fp8 LMM and the fast-mode LMM on the checkpoint w8_ref dequantises (sd: the source state dict, deq: the dequantised)."""
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
    sd = dict(W.make_state_dict(opt, 0, "perturbed"))
    for k in [k for k in sd if ".layers." in k and k.endswith(w8_ref.W8_SUFFIXES)]:      # rows of other exponents than their neighbours,
        t = sd[k].clone()                                                                  # so that a scale on the wrong row shows
        t[3::97] *= 6.0
        t[5::89] *= 0.02
        sd[k] = t
    deq = w8_ref.dequantized_state_dict(sd)
    assert all(len(set(w8_ref.row_exponents(sd[k]).tolist())) >= 3 for k in sd if ".layers.1." in k and k.endswith(w8_ref.W8_SUFFIXES))
    p = SimpleNamespace(opt=opt, sd=sd, deq=deq, w8=LMM(opt, DEV, precision="fp8"), h=LMM(opt, DEV, precision="fp16"))
    p.w8.load_state_dict(sd, strict=True)
    p.h.load_state_dict(deq, strict=True)
    assert p.w8.precision == "fp8" and p.h.precision == "fp16"
    return p


def clouds(B):
    from edgerunner_amd import weights as W
    return torch.cat([W.synthetic_point_cloud(i, 256) for i in range(B)]).to(DEV)


def teacher_forced(lmm, pc, ids, T):
    """logits [T, B, V] in front of tokens 0 .. T - 1, feeding ids [B, T]."""
    B = pc.shape[0]
    dec = lmm.mesh_decoder
    cond = lmm.encode_cond(pc, [1000] * B)["cond_embeds"]
    bos = torch.full((B, 1), lmm.opt.bos_token_id, dtype=torch.long)
    dec.prefill(torch.cat((cond, dec.embd(bos)), dim=1), T + 2)
    out = []
    for t in range(T):
        out.append(dec.logits().clone())
        if t + 1 < T:
            dec.feed([int(v) for v in ids[:, t]])
    return torch.stack(out)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_fp8_context_equals_fast_mode_on_the_dequantised_checkpoint(B):
    """B = 1 and 3 stream the bytes (the row forms; B = 1 also the fused merge + out_proj), B = 8 runs the fp16 copy."""
    p = fp8_pair()
    T = 24
    pc = clouds(B)
    _, toks = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    ids = np.stack([np.asarray(t[:T]) for t in toks])
    ref, got = teacher_forced(p.h, pc, ids, T), teacher_forced(p.w8, pc, ids, T)
    assert bool(torch.isfinite(got).all())
    assert same_bits(ref, got), f"B={B}: logits differ at steps {sorted(set((ref != got).nonzero()[:, 0].tolist()))[:8]}"
    plan = p.w8.mesh_decoder.plan()
    assert plan["batched"] == (1 if B > 4 else 0)


def test_fp8_greedy_ids_under_the_step_graph():
    p = fp8_pair()
    pc = clouds(1)
    _, ref = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    _, got = p.w8.generate(pc, 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    assert len(got[0]) == 48 and np.array_equal(np.asarray(got[0]), np.asarray(ref[0]))


# ---------------------------------------------------------------------------------------------- 6. straight to the oracle
def test_fp8_context_against_the_cpu_oracle_on_dequantised_weights():
    """The one check that does not go through the fp16 kernels: the CPU oracle on the dequantised weights, at the bound fast mode is held
    to for one row (ids exact, logits 5e-6).  That bound is fast mode's on the project's synthetic checkpoint, so this runs on that
    checkpoint as it is (rounded to e4m3 rows) - not on fp8_pair()'s, whose re-scaled rows make the logits larger."""
    import arae_oracle as O
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    opt = fp8_pair().opt
    src = W.make_state_dict(opt, 0, "perturbed")
    lmm = LMM(opt, DEV, precision="fp8")
    lmm.load_state_dict(src, strict=True)
    T = 24
    sd = O.round_streamed_weights(w8_ref.dequantized_state_dict(src), torch.float16)      # the other streamed tensors as fast mode stores them
    pc = W.synthetic_point_cloud(0, 256)
    rec = {}
    want = O.lmm_generate_ids(sd, opt, pc, 1000, max_new_tokens=T, min_new_tokens=T, fwd=O.make_forward(sd, opt, kv_round=torch.float16),
                              record_logits=lambda t, s: rec.__setitem__(t, s.numpy()[0].copy())).numpy()[0]
    _, toks = lmm.generate(pc.to(DEV), 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    got = teacher_forced(lmm, pc.to(DEV), want[None, :], T).cpu().numpy()[:, 0]
    lmm.mesh_decoder.close()
    err = max(float(np.abs(got[t] - rec[t]).max()) for t in range(T))
    print(f"fp8 context vs the oracle on dequantised weights: max|dlogit| {err:.3e} over {T} steps (largest |logit| {float(np.abs(got).max()):.2f})")
    assert np.array_equal(np.asarray(toks[0]), want), (toks[0], want)
    assert err <= 5e-6


# ---------------------------------------------------------------------------------------------- 7. mode validation
def test_create_refuses_fp8_weights_with_an_fp32_cache():
    from edgerunner_amd import native
    from edgerunner_amd.shape_opt import NativeShapeOPT
    p = fp8_pair()
    for wd, kd in (("fp8", torch.float32), ("fp8", torch.bfloat16), (torch.float16, torch.float32), (torch.float32, torch.float16)):
        with pytest.raises(native.NativeError, match=r"exact.*fast.*fp8"):
            NativeShapeOPT(p.w8.dims, p.opt, torch.device(DEV), weight_dtype=wd, kv_dtype=kd)


def test_fp8_cast_follows_the_checkpoint_rule():
    from edgerunner_amd import native
    from edgerunner_amd.models import LMM
    p = fp8_pair()
    m = LMM(p.opt, DEV, precision=None)
    m.load_state_dict(p.sd, strict=True)
    pc = clouds(1)
    _, a = m.half().generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    _, b = m.fp8().generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)      # rebuilt from the retained checkpoint
    _, want = p.w8.generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    assert m.precision == "fp8" and np.array_equal(np.asarray(b[0]), np.asarray(want[0])) and len(a[0]) == 8
    m.release_checkpoint()
    assert m.fp8() is m                                                                               # no change: nothing to rebuild
    with pytest.raises(native.NativeError, match="cannot be re-stored"):
        m.half()
    m.mesh_decoder.close()
    r = LMM(p.opt, DEV, precision="fp16")
    r.load_state_dict(p.sd, strict=True)
    r.release_checkpoint()
    with pytest.raises(native.NativeError, match=r"LMM\.fp8\(\)"):
        r.fp8()
    r.mesh_decoder.close()


def test_closed_fp8_contexts_give_their_memory_back():
    import test_gpu_lifetime as L
    opt = L.opt_small()
    from edgerunner_amd import weights as W
    sd = W.make_state_dict(opt, 0, "perturbed")
    L.touch_stream_pool()
    L.lmm_cycle(opt, sd, "fp8")
    warm = L.free_bytes()
    after = []
    for _ in range(3):
        L.lmm_cycle(opt, sd, "fp8")
        after.append(L.free_bytes())
    print(f"fp8: free after warm-up {warm}, after cycles 2..4 {after}")
    assert abs(warm - after[-1]) <= L.GRANULE, f"free memory moved by {warm - after[-1]} bytes over three create / run / close cycles"
