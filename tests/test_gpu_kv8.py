"""kv8 mode on the device: the KV cache as one OCP e4m3fn byte per element, no scale (csrc/er_w8.h kv8_encode; the QUAD lane mapping
of csrc/er_kv8_map.h in attn_decode2_kernel and attn_stream_kernel).

Exact statements where the mode allows them - the device encoder against the host's, the producers' bytes against the torch cast of what
they store into an fp32 cache, a row alone against the row in a batch, fp8 weights against fp16 weights on the dequantised checkpoint -
float64 on the decoded bytes for the two attention kernels at the fp16-cache tests' tolerance, and the CPU oracle with
kv_round=float8_e4m3fn for the model.

The oracle bound (section 5).  A K/V value that GPU and CPU compute a few ulp apart can round to neighbouring e4m3 codes - a 6 % step -
so the logits are not held to fast mode's 5e-6.  Measured on the MI355X (profiles/kv8_parity_values.log), max |dlogit| over 24 steps:
    B = 1: cloud 0 2.126e-05, cloud 1 3.600e-05;  B = 8, teacher-forced: 2.149e-05 (cloud 0 rows), 3.612e-05 (cloud 1 rows)
ORACLE_BOUND = 8e-5 is twice the largest of them (7.2e-5), rounded up to one digit (the factor 2: a compiler release may change a summation order and
with it which values flip).  It must stay <= 2.2e-4, a tenth of what e4m3 K/V itself moves these logits against fp16 K/V, and the
oracle's top-2 gap at every step must be >= 100 x the bound; both are asserted."""
import dataclasses
import functools
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref  # noqa: E402
import w8_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
HID, HEADS, HD = 1536, 16, 96
ORACLE_BOUND = 8e-5        # 2 x 3.612e-05, rounded up to one digit (module docstring)
ORACLE_CAP = 2.2e-4        # a tenth of the 2.2e-3 by which e4m3 K/V itself moves these logits against fp16 K/V
NAN32 = 0x7FC00123


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def close(a, b, atol, rtol=0.0, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol) | torch.isnan(a)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err {float(err.max()):.3e}, " \
                          f"first bad index {bad.nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------- 1. the device encoder
def test_device_encoder_equals_the_host_encoder():
    """The expected bytes are torch's clamped e4m3 cast (NaN kept), which tests/test_kv8_cpu.py proves equal to the host build of
    kv8_encode over the same sweep; nothing is compiled here."""
    from edgerunner_amd import kernels as K
    v = kv8_ref.torch_sweep()
    want = kv8_ref.torch_kv8(v)
    got = K.kv8_encode(v.to(DEV)).cpu()
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:8]]
    assert len(v) > 1000 and int(torch.isnan(v).sum()) == 6 and int(torch.isinf(v).sum()) == 2
    assert set(want[torch.isfinite(v)].tolist()) == set(range(256)) - {0x7F, 0xFF}                      # all 254 finite codes
    assert int(((v.abs() < 1.17549435e-38) & (v != 0)).sum()) >= 6                                     # fp32 subnormals
    assert want[torch.isnan(v)].tolist() == [0x7F, 0xFF] * 3 and want[torch.isinf(v)].tolist() == [0x7E, 0xFE]


# ---------------------------------------------------------------------------------------------- 2. the producers
def qkv_pair(form, B, nw=4, rw=1, pro="ln"):
    """The same QKV launch into fp32 caches and into byte caches pre-filled with 0x7F: (fp32 run, byte run), each with q / kc / vc / pos."""
    import test_gpu_decode_proj as P
    from edgerunner_amd import kernels as K, native as nat
    d = P.data()
    pos, tok = d.pos[:B], d.tok[:B]
    outs = []
    for byte in (False, True):
        if byte:
            kc = torch.full((B, HEADS, P.LCAP, HD), 0x7F, dtype=torch.uint8, device=DEV)
        else:
            kc = torch.full((B, HEADS, P.LCAP, HD), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
        vc = kc.clone()
        q = torch.full((B, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
        kw = dict(bias=d.bias["qkv"], nw=nw, rw=rw, qkv=(kc, vc, pos, q))
        if pro == "embed":
            kw["embed"] = (d.embd, d.posemb, tok, pos)
        else:
            kw.update(x=d.x[:B].contiguous(), ln=(d.lw, d.lb))
        K.gemv_form(getattr(nat, P.FORMS[form]), nat.ER_EPI_QKV, d.wh["qkv"], B, prep_xt=(form == "xt"), **kw)
        outs.append(SimpleNamespace(q=q, kc=kc, vc=vc, pos=pos))
    return outs


def assert_byte_producer(form, B, **kw):
    import test_gpu_decode_proj as P
    f32, byt = qkv_pair(form, B, **kw)
    what = f"qkv {form} B={B} {kw}"
    assert same_bits(f32.q, byt.q) and not bool(torch.isnan(byt.q).any()), what + ": q"
    for name in ("kc", "vc"):
        want = kv8_ref.torch_kv8(P.cache_rows(getattr(f32, name), f32.pos).cpu())
        got = P.cache_rows(getattr(byt, name), byt.pos).cpu()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (what, name, bad[:4].tolist())
        assert not bool(((got & 0x7F) == 0x7F).any()), what + ": a NaN byte was stored"
        c = getattr(byt, name)
        for b in range(B):                                              # every byte outside position pos[b] is still 0x7F
            rest = torch.ones(P.LCAP, dtype=torch.bool)
            rest[byt.pos[b]] = False
            assert bool((c[b][:, rest.to(DEV)] == 0x7F).all()), f"{what}: {name} row {b} written outside position {byt.pos[b]}"


@pytest.mark.parametrize("pro", ["ln", "embed"])
@pytest.mark.parametrize("nw,rw", [(4, 1), (6, 1), (9, 2)])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_qkv_row_forms_store_the_torch_cast(B, nw, rw, pro):
    assert_byte_producer("row", B, nw=nw, rw=rw, pro=pro)


@pytest.mark.parametrize("form", ["valu", "mfma", "xt"])
@pytest.mark.parametrize("B", [5, 33])
def test_qkv_batched_forms_store_the_torch_cast(B, form):
    assert_byte_producer(form, B)


# ---------------------------------------------------------------------------------------------- 3. the attention kernels
BATCH_LENS = [1, 3, 4, 5, 127, 128, 129, 255, 256, 257, 2050]      # every residue of a quad, one key, the chunk and the tile edges
LONG_LENS = [18050, 8193]


@functools.lru_cache(maxsize=None)
def attn_case(lens):
    """q, byte caches with the unused tail 0x7F (NaN), and the float64 attention over the decoded bytes - computed once per set of lengths."""
    B = len(lens)
    Lcap = (max(lens) + 31) // 32 * 32
    q = rnd(B, HID, seed=401).to(DEV)
    kc = kv8_ref.torch_kv8(rnd(B, HEADS, Lcap, HD, seed=402)).to(DEV)
    vc = kv8_ref.torch_kv8(rnd(B, HEADS, Lcap, HD, seed=403) * 2.0).to(DEV)
    assert not bool(((kc & 0x7F) == 0x7F).any())
    for b, n in enumerate(lens):
        kc[b, :, n:] = 0x7F
        vc[b, :, n:] = 0xFF if b % 2 else 0x7F
    ref = []
    for b, n in enumerate(lens):
        kd, vd = kv8_ref.kv8_decode(kc[b, :, :n]).double(), kv8_ref.kv8_decode(vc[b, :, :n]).double()
        w = torch.softmax(q[b].view(HEADS, 1, HD).double() @ kd.transpose(1, 2) / math.sqrt(HD), dim=-1)
        ref.append((w @ vd).reshape(HID))
    return SimpleNamespace(q=q, kc=kc, vc=vc, ref=torch.stack(ref), lens=list(lens))


@pytest.mark.parametrize("lens", [tuple(BATCH_LENS), tuple(LONG_LENS)], ids=["edges", "long"])
@pytest.mark.parametrize("variant", ["split2", "stream"])
def test_attention_on_bytes_against_float64(variant, lens):
    from edgerunner_amd import kernels as K, native
    c = attn_case(lens)
    v = native.ER_ATTN_SPLIT2 if variant == "split2" else native.ER_ATTN_STREAM
    out = K.attn_decode(c.q, c.kc, c.vc, c.lens, 4, v)
    for b, n in enumerate(c.lens):
        close(out[b], c.ref[b], 2e-6, 1e-5, f"kv8 {variant} row {b} len {n}")
    # the same bytes through a float8 view of the cache
    out8 = K.attn_decode(c.q, c.kc.view(torch.float8_e4m3fn), c.vc.view(torch.float8_e4m3fn), c.lens, 4, v)
    assert torch.equal(out, out8)


@pytest.mark.parametrize("variant", ["split2", "stream"])
def test_attention_row_alone_equals_the_row_in_the_batch(variant):
    from edgerunner_amd import kernels as K, native
    c = attn_case(tuple(reversed(BATCH_LENS)))                      # row 0 holds 2050 keys: several chunks / tiles and a ragged quad
    v = native.ER_ATTN_SPLIT2 if variant == "split2" else native.ER_ATTN_STREAM
    batch = K.attn_decode(c.q, c.kc, c.vc, c.lens, 4, v)
    alone = K.attn_decode(c.q[:1].contiguous(), c.kc[:1].contiguous(), c.vc[:1].contiguous(), c.lens[:1], 4, v)
    assert not bool(torch.isnan(alone).any()) and torch.equal(alone[0], batch[0])
    close(batch, c.ref, 2e-6, 1e-5, f"kv8 {variant} reversed batch")


def test_attention_entry_refuses_what_has_no_byte_form():
    from edgerunner_amd import kernels as K, native
    c = attn_case(tuple(BATCH_LENS))
    with pytest.raises(native.NativeError):
        K.attn_decode(c.q, c.kc, c.vc, c.lens, 4, native.ER_ATTN_SPLIT1)      # the round-1 split kernel
    with pytest.raises(native.NativeError):
        K.attn_decode(c.q, c.kc, c.vc, c.lens, 8, native.ER_ATTN_SPLIT2)      # one chunking only


# ---------------------------------------------------------------------------------------------- 4. end to end, exact statements
def small_opt():
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")


@functools.lru_cache(maxsize=None)
def kv8_models():
    """2-layer contexts on one checkpoint: kv8 with fp16 weights, kv8 with fp8 weights, kv8 with fp16 weights on the checkpoint w8_ref
    dequantises (what the fp8 context must equal), and plain fast mode."""
    from edgerunner_amd import weights as W
    from edgerunner_amd.models import LMM
    opt = small_opt()
    sd = dict(W.make_state_dict(opt, 0, "perturbed"))
    deq = w8_ref.dequantized_state_dict(sd)
    p = SimpleNamespace(opt=opt, sd=sd, deq=deq)
    p.kv8 = LMM(opt, DEV, precision="fp16", kv_precision="fp8")
    p.w8kv8 = LMM(opt, DEV, precision="fp8", kv_precision="fp8")
    p.kv8_deq = LMM(opt, DEV, precision="fp16", kv_precision="fp8")
    p.fast = LMM(opt, DEV, precision="fp16")
    for m, s in ((p.kv8, sd), (p.w8kv8, sd), (p.kv8_deq, deq), (p.fast, sd)):
        m.load_state_dict(s, strict=True)
    assert (p.kv8.precision, p.kv8.kv_precision) == ("fp16", "fp8") and (p.w8kv8.precision, p.w8kv8.kv_precision) == ("fp8", "fp8")
    assert p.fast.kv_precision is None
    return p


def clouds(B, first=0):
    from edgerunner_amd import weights as W
    return torch.cat([W.synthetic_point_cloud(first + i, 256) for i in range(B)]).to(DEV)


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


@functools.lru_cache(maxsize=None)
def greedy_ids(T=24):
    """ids [8, T] the kv8 context generates for clouds 0 .. 7 one by one: what the teacher-forced runs feed"""
    p = kv8_models()
    out = []
    for i in range(8):
        _, toks = p.kv8.generate(clouds(1, i), 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
        out.append(np.asarray(toks[0][:T]))
    return np.stack(out)


@pytest.mark.parametrize("Ba,Bb", [(1, 3), (6, 8)])
def test_row_0_does_not_depend_on_its_batch(Ba, Bb):
    """B = 1 and 3 run the row kernels and the split attention, B = 6 and 8 the batched forms and the streaming attention: inside a
    class a row's logits are the same bits whatever shares the batch."""
    p, T = kv8_models(), 24
    ids = greedy_ids()
    a = teacher_forced(p.kv8, clouds(Ba), ids[:Ba], T)
    plan_a = p.kv8.mesh_decoder.plan()
    b = teacher_forced(p.kv8, clouds(Bb), ids[:Bb], T)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert same_bits(a[:, 0], b[:, 0]), f"row 0 at B={Ba} and B={Bb}: steps {sorted(set((a[:, 0] != b[:, 0]).nonzero()[:, 0].tolist()))[:8]}"
    assert plan_a["batched"] == (1 if Ba > 4 else 0) and p.kv8.mesh_decoder.plan()["batched"] == (1 if Bb > 4 else 0)


def test_greedy_ids_under_the_step_graph_and_without(monkeypatch):
    from edgerunner_amd.models import LMM
    p = kv8_models()
    pc = clouds(1)
    _, graph = p.kv8.generate(pc, 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    monkeypatch.setenv("ER_NO_GRAPH", "1")                          # read by er_create
    eager = LMM(p.opt, DEV, precision="fp16", kv_precision="fp8")
    eager.load_state_dict(p.sd, strict=True)
    _, plain = eager.generate(pc, 1000, tokenizer=object(), max_new_tokens=48, min_new_tokens=48)
    eager.mesh_decoder.close()
    assert len(graph[0]) == 48 and np.array_equal(np.asarray(graph[0]), np.asarray(plain[0]))


@pytest.mark.parametrize("B", [1, 3])
def test_fp8_weights_on_a_byte_cache_equal_fp16_weights_on_the_dequantised_checkpoint(B):
    p, T = kv8_models(), 24
    ids = greedy_ids()[:B]
    ref, got = teacher_forced(p.kv8_deq, clouds(B), ids, T), teacher_forced(p.w8kv8, clouds(B), ids, T)
    assert bool(torch.isfinite(got).all())
    assert same_bits(ref, got), f"B={B}: logits differ at steps {sorted(set((ref != got).nonzero()[:, 0].tolist()))[:8]}"


# ---------------------------------------------------------------------------------------------- 5. end to end, the oracle
@functools.lru_cache(maxsize=None)
def oracle_run(cloud, T=24):
    """(ids [T], logits [T, V]) of the CPU oracle with fast mode's fp16 weights and K/V rounded through e4m3"""
    import arae_oracle as O
    from edgerunner_amd import weights as W
    p = kv8_models()
    sd = O.round_streamed_weights(p.sd, torch.float16)
    rec = {}
    ids = O.lmm_generate_ids(sd, p.opt, W.synthetic_point_cloud(cloud, 256), 1000, max_new_tokens=T, min_new_tokens=T,
                             fwd=O.make_forward(sd, p.opt, kv_round=torch.float8_e4m3fn),
                             record_logits=lambda t, s: rec.__setitem__(t, s.numpy()[0].copy())).numpy()[0]
    return ids, np.stack([rec[t] for t in range(T)])


def top2_gap(logits):
    s = np.sort(logits, axis=-1)
    return float((s[:, -1] - s[:, -2]).min())


def test_oracle_bound_is_honest():
    assert ORACLE_BOUND <= ORACLE_CAP
    for c in (0, 1):
        gap = top2_gap(oracle_run(c)[1])
        print(f"kv8 oracle, cloud {c}: smallest top-2 gap over 24 steps {gap:.3e} (bound {ORACLE_BOUND:.1e})")
        assert gap >= 100 * ORACLE_BOUND, (c, gap)


@pytest.mark.parametrize("cloud", [0, 1])
def test_single_row_against_the_cpu_oracle(cloud):
    p, T = kv8_models(), 24
    want, ref = oracle_run(cloud)
    pc = clouds(1, cloud)
    _, toks = p.kv8.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    got = teacher_forced(p.kv8, pc, want[None, :], T).cpu().numpy()[:, 0]
    err = float(np.abs(got - ref).max())
    print(f"kv8 vs the oracle, B = 1, cloud {cloud}: max|dlogit| {err:.3e} over {T} steps (largest |logit| {float(np.abs(got).max()):.2f})")
    assert np.array_equal(np.asarray(toks[0][:T]), want), (toks[0], want)
    assert err <= ORACLE_BOUND


def test_batch_of_8_against_the_cpu_oracle():
    p, T = kv8_models(), 24
    runs = [oracle_run(c) for c in (0, 1)]
    which = [0, 1, 1, 0, 0, 1, 0, 1]
    pc = torch.cat([clouds(1, c) for c in which])
    ids = np.stack([runs[c][0] for c in which])
    got = teacher_forced(p.kv8, pc, ids, T).cpu().numpy()
    assert p.kv8.mesh_decoder.plan()["attn_kernel"] == 4
    errs = [float(np.abs(got[:, b] - runs[c][1]).max()) for b, c in enumerate(which)]
    print(f"kv8 vs the oracle, B = 8 teacher-forced: max|dlogit| per row {['%.3e' % e for e in errs]}")
    assert max(errs) <= ORACLE_BOUND
    # the ids: the batch generating on its own (greedy under the token grammar, as the oracle generates)
    _, toks = p.kv8.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    for b, c in enumerate(which):
        assert np.array_equal(np.asarray(toks[b][:T]), runs[c][0]), f"row {b} (cloud {c}): greedy ids differ from the oracle's"


# ---------------------------------------------------------------------------------------------- 6. the surface
def test_create_accepts_and_refuses():
    from edgerunner_amd import native
    from edgerunner_amd.options import config_defaults
    from edgerunner_amd.shape_opt import NativeShapeOPT
    from edgerunner_amd.weights import dims_from_options
    p = kv8_models()
    dims = p.kv8.dims
    for wd in (torch.float16, "fp8"):
        NativeShapeOPT(dims, p.opt, torch.device(DEV), weight_dtype=wd, kv_dtype="fp8").close()
        NativeShapeOPT(dims, p.opt, torch.device(DEV), weight_dtype=wd, kv_dtype=torch.float8_e4m3fn).close()
    refused = [("fp8", torch.float32), ("fp8", torch.bfloat16), (torch.float16, torch.float32), (torch.float32, torch.float16),
               (torch.float32, "fp8"), (torch.bfloat16, "fp8")]
    for wd, kd in refused:
        with pytest.raises(native.NativeError, match=r"exact.*fast.*fp8"):
            NativeShapeOPT(dims, p.opt, torch.device(DEV), weight_dtype=wd, kv_dtype=kd)
    opt64 = dataclasses.replace(config_defaults["ArAE"], num_layers=2, num_heads=24)      # head_dim 64
    d64 = dims_from_options(opt64)
    assert d64.hidden_dim // d64.num_heads == 64
    NativeShapeOPT(d64, opt64, torch.device(DEV), weight_dtype=torch.float16, kv_dtype=torch.float16).close()
    with pytest.raises(native.NativeError, match=r"\(-5\).*head_dim 96"):                  # ER_ERR_UNSUPPORTED
        NativeShapeOPT(d64, opt64, torch.device(DEV), weight_dtype=torch.float16, kv_dtype="fp8")


def test_prefix_groups_are_refused_and_the_context_stays_usable():
    from edgerunner_amd import native
    p = kv8_models()
    pc = clouds(6)
    _, before = p.kv8.generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    dec = p.kv8.mesh_decoder
    with pytest.raises(native.NativeError, match="prefix"):
        dec.set_prefix_groups(([0, 0, 0, 3, 3, 3], 4))
    dec.set_prefix_groups(None)                                      # clearing nothing is fine
    _, after = p.kv8.generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(before, after))


def test_plan_reports_what_runs():
    from edgerunner_amd import native
    p = kv8_models()
    dec = p.kv8.mesh_decoder
    dec.reserve(1, 512)
    plan = dec.plan()
    assert (plan["decode_version"], plan["attn_kernel"], plan["merge_launch"]) == (2, native.ER_ATTN_SPLIT2, 1)
    dec.reserve(5, 512)
    plan = dec.plan()
    assert (plan["batched"], plan["attn_kernel"], plan["merge_launch"]) == (1, native.ER_ATTN_STREAM, 0)
    fast = p.fast.mesh_decoder
    fast.reserve(1, 512)
    assert fast.plan()["decode_version"] == 3
    fast.reserve(5, 512)
    assert fast.plan()["attn_kernel"] == native.ER_ATTN_SPLIT1


def test_reserve_takes_half_the_memory():
    import test_gpu_lifetime as L
    p = kv8_models()
    drops = {}
    for name, lmm in (("fp16", p.fast), ("kv8", p.kv8)):
        dec = lmm.mesh_decoder
        dec.reserve(1, 64)
        dec.reserve(8, 64)                                           # the batched workspace and the tiled weight copies exist before the measurement
        dec.reserve(1, 64)
        free0 = L.free_bytes()
        dec.reserve(8, 4096)
        drops[name] = free0 - L.free_bytes()
        dec.reserve(1, 64)
    print(f"free-memory drop of reserve(8, 4096): fp16 cache {drops['fp16']}, byte cache {drops['kv8']}")
    assert drops["fp16"] > 0 and drops["kv8"] <= 0.55 * drops["fp16"]


def test_closed_kv8_contexts_give_their_memory_back():
    import test_gpu_lifetime as L
    from edgerunner_amd.models import LMM
    p = kv8_models()

    def cycle():
        lmm = LMM(p.opt, DEV, precision="fp16", kv_precision="fp8")
        lmm.load_state_dict(p.sd, strict=True)
        pc = clouds(6)
        _, one = lmm.generate(pc[:1], 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
        _, six = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
        assert len(six) == 6 and len(one[0]) == 8
        lmm.mesh_decoder.close()

    L.touch_stream_pool()
    cycle()
    warm = L.free_bytes()
    after = []
    for _ in range(3):
        cycle()
        after.append(L.free_bytes())
    print(f"kv8: free after warm-up {warm}, after cycles 2..4 {after}")
    assert abs(warm - after[-1]) <= L.GRANULE, f"free memory moved by {warm - after[-1]} bytes over three create / run / close cycles"


def test_queue_of_three_jobs_over_two_rows():
    p = kv8_models()
    jobs = [(clouds(1, i), 1000) for i in (0, 1, 2)]
    want = []
    for pc, nf in jobs:
        _, toks = p.kv8.generate(pc, nf, tokenizer=object(), max_new_tokens=20, min_new_tokens=20)
        want.append(np.asarray(toks[0]))
    _, got = p.kv8.generate_queue(jobs, slots=2, tokenizer=object(), max_new_tokens=20, min_new_tokens=20, check_every=4)
    assert p.kv8.last_queue_stats["admissions"] == 3
    for j in range(3):
        assert np.array_equal(np.asarray(got[j]).reshape(-1), want[j].reshape(-1)), (j, got[j], want[j])


def test_infer_py_with_a_byte_cache(tmp_path):
    from safetensors.torch import save_file
    from edgerunner_amd import weights as W
    p = kv8_models()
    ckpt = str(tmp_path / "arae_2layers.safetensors")
    save_file({k: v.contiguous() for k, v in p.sd.items()}, ckpt)
    inp = tmp_path / "a.npy"
    np.save(inp, W.synthetic_point_cloud(0, 256)[0].numpy())
    out = tmp_path / "out"
    env = dict(os.environ)
    env.pop("ER_NO_GRAPH", None)
    env["EDGERUNNER_KV_PRECISION"] = "fp8"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "ArAE", "--num_layers", "2", "--resume", ckpt, "--test_path", str(inp),
                        "--generate_mode", "greedy", "--test_num_face", "1000", "--test_max_seq_length", "24", "--workspace", str(out)],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    got = np.load(out / "a_0_1000f_tokens.npy")
    assert got.ndim == 1 and len(got) > 0 and (out / "tokens_all.npz").exists()
    from edgerunner_amd.utils import trim_tokens
    _, toks = p.kv8.generate(clouds(1), 1000, tokenizer=object(), max_new_tokens=24)
    assert np.array_equal(got, trim_tokens(np.asarray(toks[0])))
