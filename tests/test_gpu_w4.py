"""fp4 mode on the device: MXFP4 (e2m1 nibbles, one e8m0 scale byte per block of 32 along a row; csrc/er_w4.h) for the six decoder
matrices of a layer, streamed by the single-row forms of qkv, fc1 and fc2 (csrc/er_w4_map.h, csrc/k_gemv.h).

Like fp8 mode the mode needs no numerical oracle of its own: an fp4 context computes, bit for bit, what a fast-mode (fp16) context
computes on the checkpoint that tests/w4_ref.py dequantises.  So the hardware conversion is compared exactly with the header's decode, the
quantiser exactly with w4_ref, the nibble kernels with the fp16 kernels on the dequantised matrix (same bits), the model with a
fast-mode model on the dequantised state dict (same bits, with the nibble kernels on and off), and one check goes straight to the CPU
oracle at the bound tests/test_gpu_w8.py holds fp8 mode to in the same comparison (ids exact, logits 5e-6)."""
import contextlib
import dataclasses
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w4_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID, INTER, VOCAB, NPOS = 1536, 6144, 518, 64
HEADS, HD, LCAP = 16, 96, 64
NAN32, NAN16, NAN8 = 0x7FC00123, 0x7E01, 0x7F       # sentinels: NaN patterns no kernel produces (0x7F: the e4m3 NaN byte)
ORACLE_BOUND = 5e-6                                 # tests/test_gpu_w8.py, the same comparison for fp8 mode: fast mode's single-row bound


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


@contextlib.contextmanager
def env(**kw):
    """environment knobs that er_create reads, for the creation of one context"""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------- 1. the conversion instruction
def test_hardware_conversion_is_the_headers_decode_times_the_scale():
    """v_cvt_scalef32_pk_f32_fp4 on all 256 byte values x 4 byte selects x every exponent of the clamp range: the low nibble first, OCP
    e2m1, times 2^e exactly (the sign of zero included)."""
    from edgerunner_amd import kernels as K
    got = K.w4_cvt_probe(DEV).cpu()
    assert got.shape == (23, 256, 4, 2)
    table = w4_ref.decode_table()
    byte = torch.arange(256)
    pair = torch.stack((table[byte & 15], table[byte >> 4]), dim=1)                          # [256, 2]: low nibble = the even element
    want = torch.ldexp(pair[None, :, None, :].expand(23, 256, 4, 2), torch.arange(-15, 8, dtype=torch.int32)[:, None, None, None])
    bad = (got.view(torch.int32) != want.contiguous().view(torch.int32)).nonzero()
    assert bad.numel() == 0, [(b, float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:6].tolist()]
    assert float(got[22, 0x7F, 3, 1]) == 768.0 and float(got[0, 0x19, 0, 0]) == -2.0 ** -16   # the largest and the smallest magnitude


# ---------------------------------------------------------------------------------------------- 2. the quantiser
def quant_source(n, k, dtype):
    w = rnd(n, k, seed=n + k, scale=0.02)
    w[:8] = w4_ref.crafted_matrix(8, k, seed=3)
    w[8] = -w[8].abs()                                           # a row of negative values
    w[9, 32:64] *= 300.0                                         # blocks of other exponents than their neighbours
    w[9, 64:96] *= 1e-3
    return w.to(dtype)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n,k", [(20, HID), (8, INTER)])
def test_quantiser_equals_the_reference_exactly(n, k, dtype, where):
    from edgerunner_amd import kernels as K
    w = quant_source(max(n, 10), k, dtype)[:n].contiguous()
    nib_ref, sc_ref, e_ref, w16_ref = w4_ref.quantize(w)
    block, e, w16 = K.w4_quantize(w.to(DEV) if where == "device" else w, device=DEV)
    nib, sc = K.w4_block_parts(block.cpu(), n, k)
    assert e.cpu().tolist() == e_ref.tolist()
    assert torch.equal(sc, sc_ref)
    bad = (nib != nib_ref).nonzero()
    assert bad.numel() == 0, (bad[:4].tolist(), [(w[i, 2 * j: 2 * j + 2].tolist(), hex(int(nib[i, j])), hex(int(nib_ref[i, j]))) for i, j in bad[:4].tolist()])
    assert same_bits(w16.cpu(), w16_ref)                         # -0 stays -0
    assert set(e_ref.flatten().tolist()) >= {-15, 7, -7, -6, 0}  # the crafted blocks reach both clamps and both sides of a boundary


def test_non_finite_source_is_refused_with_the_keys_name():
    from edgerunner_amd import kernels as K, native
    p = models()
    lmm = p.on
    key = "mesh_decoder.model.layers.1.fc1.weight"
    for poison in (float("nan"), float("inf"), -float("inf")):
        w = rnd(INTER, HID, seed=9, scale=0.02)
        w[4097, 13] = poison
        with pytest.raises(native.NativeError, match=key.replace(".", r"\.")):
            native.load_tensor(lmm.mesh_decoder.lib.er_load_tensor, lmm.mesh_decoder._ctx, key, w)
        with pytest.raises(native.NativeError):
            K.w4_quantize(w[4090:4100].contiguous(), device=DEV)
    # the context is whole again once the real tensor is back
    native.load_tensor(lmm.mesh_decoder.lib.er_load_tensor, lmm.mesh_decoder._ctx, key, p.sd[key])
    assert lmm.mesh_decoder.lib.er_finalize_weights(lmm.mesh_decoder._ctx) == 0
    pc = clouds(1)
    _, a = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    _, b = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    assert np.array_equal(np.asarray(a[0]), np.asarray(b[0]))


# ---------------------------------------------------------------------------------------------- 3. the nibble kernels
# fc1 / fc2 rows: 20 = five quads (an fc1 workgroup holds 6: it is partly out of range), 48 fills whole workgroups; qkv has its real
# size (n = 3 k)
@functools.lru_cache(maxsize=None)
def data():
    from edgerunner_amd import kernels as K
    d = SimpleNamespace(blk={}, w16={}, n={}, k={})
    shapes = {"qkv": (3 * HID, HID), "fc1_20": (20, HID), "fc1_48": (48, HID), "fc2_20": (20, INTER), "fc2_48": (48, INTER), "fc1_22": (22, HID)}
    for i, (name, (n, k)) in enumerate(shapes.items()):
        w = rnd(n, k, seed=401 + i, scale=0.02)
        w[5] *= 40.0
        w[6] *= 1e-4                                             # rows and blocks of other exponents
        w[:, 96:128] *= 9.0
        w[7, 32:64] = 0.0
        d.blk[name], _, d.w16[name] = K.w4_quantize(w, device=DEV)
        d.n[name], d.k[name] = n, k
    d.bias = {name: rnd(n, seed=411 + i, scale=0.02).to(DEV) for i, (name, (n, _)) in enumerate(shapes.items())}
    d.x = (rnd(4, HID, seed=421) * 2 + 0.3).to(DEV)
    d.lw, d.lb = (1 + 0.1 * rnd(HID, seed=422)).to(DEV), (0.05 * rnd(HID, seed=423)).to(DEV)
    d.f = torch.relu(rnd(4, INTER, seed=425)).to(DEV)
    d.r = {name: rnd(4, n, seed=427).to(DEV) for name, (n, _) in shapes.items()}
    d.embd, d.posemb = rnd(VOCAB, HID, seed=428).to(DEV), rnd(NPOS, HID, seed=429).to(DEV)
    d.pos, d.tok = [0, LCAP - 1, 5, 17], [0, VOCAB - 1, 7, 300]
    return d


def sentinel_caches(B, byte_cache):
    if byte_cache:
        kc = torch.full((B, HEADS, LCAP, HD), NAN8, dtype=torch.uint8, device=DEV)
    else:
        kc = torch.full((B, HEADS, LCAP, HD), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    q = torch.full((B, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    return kc, kc.clone(), q


def launch(name, B, w4, nw, rw, pro="ln", byte_cache=False, rows=None):
    """One projection through er_k_gemv_form (the fp16 dequantised matrix) or er_k_gemv_form_w4 (the canonical block): dict of outputs."""
    from edgerunner_amd import kernels as K, native as nat
    d = data()
    proj = name.split("_")[0]
    epi = {"qkv": nat.ER_EPI_QKV, "fc1": nat.ER_EPI_RELU, "fc2": nat.ER_EPI_RESID}[proj]
    rows = list(range(B)) if rows is None else rows
    kw = dict(bias=d.bias[name], nw=nw, rw=rw)
    if proj in ("qkv", "fc1"):
        if pro == "embed":
            kw["embed"] = (d.embd, d.posemb, [d.tok[b] for b in rows], [d.pos[b] for b in rows])
        else:
            kw.update(x=d.x[rows].contiguous(), ln=(d.lw, d.lb))
        kw["return_xnorm"] = True
    else:
        kw.update(x=d.f[rows].contiguous(), resid=d.r[name][rows].contiguous())
    if proj == "qkv":
        kc, vc, q = sentinel_caches(B, byte_cache)
        kw["qkv"] = (kc, vc, [d.pos[b] for b in rows], q)
    o = (K.gemv_form_w4(nat.ER_FORM_ROW, epi, d.blk[name], d.n[name], d.k[name], B, **kw) if w4
         else K.gemv_form(nat.ER_FORM_ROW, epi, d.w16[name], B, **kw))
    if proj == "qkv":
        o["kc"], o["vc"] = kc, vc
    return o


def assert_same(ref, got, what):
    assert set(ref) == set(got), what
    for k in ref:
        assert same_bits(ref[k], got[k]), f"{what}: {k} differs in {int((ref[k].float() != got[k].float()).sum())} places"
        assert k in ("kc", "vc") or not bool(torch.isnan(got[k]).any()), (what, k)


@pytest.mark.parametrize("byte_cache", [False, True])
@pytest.mark.parametrize("pro", ["ln", "embed"])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_qkv_nibble_forms_equal_the_fp16_kernel(B, pro, byte_cache):
    """qkv at its real size only: er_k_gemv_form's checks fix n = 3 k = 4608 for the QKV epilogue (288 whole workgroups), so the partly
    out-of-range last workgroup - the clamped quad - is exercised through fc1 (n = 20) below, the same load and store guards."""
    ref = launch("qkv", B, False, 9, 2, pro, byte_cache)
    d = data()
    got = launch("qkv", B, True, 9, 2, pro, byte_cache)
    assert_same(ref, got, f"qkv B={B} {pro} byte_cache={byte_cache}")
    for c in (got["kc"], got["vc"]):                              # the cache is written at pos and nowhere else
        bits, s = (c, NAN8) if byte_cache else (c.view(torch.int16), NAN16)
        for b in range(B):
            rest = torch.ones(LCAP, dtype=torch.bool)
            rest[d.pos[b]] = False
            assert bool((bits[b][:, rest.to(DEV)] == s).all()) and not bool((bits[b][:, d.pos[b]] == s).any())


@pytest.mark.parametrize("n", [20, 48])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_fc1_nibble_forms_equal_the_fp16_kernels(B, n):
    for nw in (12, 4):                                            # the fp16 row forms the step launches
        assert_same(launch(f"fc1_{n}", B, False, nw, 2), launch(f"fc1_{n}", B, True, nw, 2), f"fc1 n={n} B={B} fp16 {nw}x2")


@pytest.mark.parametrize("n", [20, 48])
@pytest.mark.parametrize("B,rw", [(1, 6), (1, 2), (2, 2), (3, 2), (4, 2)])
def test_fc2_split_k_nibble_form_equals_the_fp16_kernels(B, rw, n):
    assert_same(launch(f"fc2_{n}", B, False, 4, rw), launch(f"fc2_{n}", B, True, 4, rw), f"fc2 n={n} B={B} rw={rw}")


@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("name,nw", [("fc1_20", 12), ("fc2_20", 4)])
def test_a_row_of_a_batch_equals_the_row_alone(name, nw, B):
    batch = launch(name, B, True, nw, 2)["y"]
    for b in range(B):
        assert same_bits(launch(name, 1, True, nw, 2, rows=[b])["y"][0], batch[b]), (name, b)


@pytest.mark.parametrize("byte_cache", [False, True])
@pytest.mark.parametrize("pro", ["ln", "embed"])
@pytest.mark.parametrize("B", [3, 4])
def test_a_qkv_row_of_a_batch_equals_the_row_alone(B, pro, byte_cache):
    """q, the LayerNorm'd / embedded input and both cache rows of batch row b, launched with B - 1 others and launched alone."""
    batch = launch("qkv", B, True, 9, 2, pro, byte_cache)
    for b in range(B):
        alone = launch("qkv", 1, True, 9, 2, pro, byte_cache, rows=[b])
        for k in ("q", "xnorm", "kc", "vc"):
            assert same_bits(alone[k][0], batch[k][b]), (k, b, B, pro, byte_cache)


def test_refusals_come_before_any_launch():
    from edgerunner_amd import kernels as K, native as nat
    d = data()
    ln = dict(x=d.x[:1].contiguous(), ln=(d.lw, d.lb))
    with pytest.raises(nat.NativeError, match="multiple of 4"):                # N % 4 != 0
        K.gemv_form_w4(nat.ER_FORM_ROW, nat.ER_EPI_RELU, d.blk["fc1_22"], 22, HID, 1, bias=d.bias["fc1_22"], nw=12, rw=2, **ln)
    with pytest.raises(nat.NativeError, match="out_proj"):                     # out_proj has no nibble form
        K.gemv_form_w4(nat.ER_FORM_ROW, nat.ER_EPI_RESID, d.blk["fc1_48"], 48, HID, 1, x=d.x[:1].contiguous(), resid=d.r["fc1_48"][:1].contiguous(),
                       bias=d.bias["fc1_48"], nw=3, rw=1)
    with pytest.raises(nat.NativeError, match="lm_head"):                      # the lm_head is not quantised
        K.gemv_form_w4(nat.ER_FORM_ROW, nat.ER_EPI_STORE, d.blk["fc1_48"], 48, HID, 1, nw=4, rw=1, **ln)
    with pytest.raises(nat.NativeError, match="row forms"):                    # the batched forms run the fp16 copy
        K.gemv_form_w4(nat.ER_FORM_VALU, nat.ER_EPI_RELU, d.blk["fc1_48"], 48, HID, 5, x=(rnd(5, HID, seed=2) + 0).to(DEV), ln=(d.lw, d.lb),
                       bias=d.bias["fc1_48"])
    with pytest.raises(nat.NativeError):                                       # batch 5 has no row form
        K.gemv_form_w4(nat.ER_FORM_ROW, nat.ER_EPI_RELU, d.blk["fc1_48"], 48, HID, 5, x=(rnd(5, HID, seed=2) + 0).to(DEV), ln=(d.lw, d.lb),
                       bias=d.bias["fc1_48"], nw=12, rw=2)
    # an fp32 cache, and a shape the step never launches: nothing is written
    for cache_dtype, nw in ((torch.float32, 9), (torch.float16, 5)):
        kc = torch.full((2, HEADS, LCAP, HD), NAN32, dtype=torch.int32, device=DEV).view(torch.float32).to(cache_dtype) if cache_dtype == torch.float32 \
            else torch.full((2, HEADS, LCAP, HD), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
        vc = kc.clone()
        q = torch.full((2, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
        before = (kc.clone(), vc.clone())
        with pytest.raises(nat.NativeError, match="fp32" if cache_dtype == torch.float32 else None):
            K.gemv_form_w4(nat.ER_FORM_ROW, nat.ER_EPI_QKV, d.blk["qkv"], 3 * HID, HID, 2, x=d.x[:2].contiguous(), ln=(d.lw, d.lb),
                           bias=d.bias["qkv"], nw=nw, rw=2 if nw == 9 else 1, qkv=(kc, vc, d.pos[:2], q))
        assert same_bits(kc, before[0]) and same_bits(vc, before[1]) and bool((q.view(torch.int32) == NAN32).all())


# ---------------------------------------------------------------------------------------------- 4. end to end
def small_opt():
    from edgerunner_amd.options import config_defaults
    return dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")


@functools.lru_cache(maxsize=None)
def checkpoint():
    from edgerunner_amd import weights as W
    sd = dict(W.make_state_dict(small_opt(), 0, "perturbed"))
    for k in [k for k in sd if ".layers." in k and k.endswith(w4_ref.W4_SUFFIXES)]:      # blocks of other exponents than their neighbours,
        t = sd[k].clone()                                                                  # so that a scale on the wrong block or row shows
        t[3::97] *= 6.0
        t[:, 64:96] *= 0.05
        t[5::89, 32:64] *= 11.0
        sd[k] = t
    return sd, w4_ref.dequantized_state_dict(sd)


def make_lmm(sd, precision, kv=None, rows=None):
    """A 2-layer LMM on sd; rows: ER_W4_ROWS at er_create (None: unset)."""
    from edgerunner_amd.models import LMM
    with env(ER_W4_ROWS=rows):
        m = LMM(small_opt(), DEV, precision=precision, kv_precision=kv)
    m.load_state_dict(sd, strict=True)
    return m


@functools.lru_cache(maxsize=None)
def models(kv=None):
    """fp4 contexts with the nibble kernels on (ER_W4_ROWS=1) and off (=0), and the fast-mode context on the checkpoint w4_ref
    dequantises; kv = None (fp16 cache) or "fp8" (byte cache)."""
    sd, deq = checkpoint()
    p = SimpleNamespace(opt=small_opt(), sd=sd, deq=deq, on=make_lmm(sd, "mxfp4", kv, 1), off=make_lmm(sd, "mxfp4", kv, 0), h=make_lmm(deq, "fp16", kv))
    assert (p.on.precision, p.on.kv_precision, p.h.precision) == ("mxfp4", kv, "fp16")
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


NIBBLES = {"qkv": 1, "out_proj": 0, "fc1": 1, "fc2": 1}
NONE = dict.fromkeys(NIBBLES, 0)


@pytest.mark.parametrize("kv", [None, "fp8"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_fp4_context_equals_fast_mode_on_the_dequantised_checkpoint(B, kv):
    """B = 1 and 3 stream the nibbles under ER_W4_ROWS=1 (the row forms of qkv, fc1, fc2), B = 8 runs the fp16 copies; under ER_W4_ROWS=0
    everything does.  Logits and greedy ids are the same bits in all three contexts."""
    p = models(kv)
    T = 16
    pc = clouds(B)
    _, toks = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    ids = np.stack([np.asarray(t[:T]) for t in toks])
    ref = teacher_forced(p.h, pc, ids, T)
    for name, lmm, want in (("ER_W4_ROWS=1", p.on, NIBBLES if B <= 4 else NONE), ("ER_W4_ROWS=0", p.off, NONE)):
        got = teacher_forced(lmm, pc, ids, T)
        assert bool(torch.isfinite(got).all())
        assert same_bits(ref, got), f"{name} B={B} kv={kv}: logits differ at steps {sorted(set((ref != got).nonzero()[:, 0].tolist()))[:8]}"
        assert lmm.mesh_decoder.w4_streams() == want and lmm.mesh_decoder.plan()["batched"] == (1 if B > 4 else 0)
        _, own = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)       # the step graph
        assert all(np.array_equal(np.asarray(a[:T]), np.asarray(b[:T])) for a, b in zip(own, toks)), name
    assert p.h.mesh_decoder.w4_streams() == NONE


@functools.lru_cache(maxsize=None)
def single_row_model(kv):
    """The fp4 context with the nibble kernels on whose ONE-row plan runs the attention the 2 .. 4-row plans run (ER_DECODE_V=2: fixed
    chunks + merge launch).  By default one row on an fp16 cache decodes with version 3 (balanced chunks, merge fused into out_proj), which
    sums a head's keys in another order: fast mode's logits at B = 1 and at B = 3 differ in the last places for that reason, with fp16
    weights as with nibbles.  A byte cache decodes with version 2 at every row count already."""
    sd, _ = checkpoint()
    with env(ER_DECODE_V=2):
        return make_lmm(sd, "mxfp4", kv, 1)


@pytest.mark.parametrize("kv", [None, "fp8"])
@pytest.mark.parametrize("B", [3, 4])
def test_a_row_of_a_batch_equals_the_row_alone_end_to_end(B, kv):
    """The 2-layer fp4 model with the nibble kernels on (ER_W4_ROWS=1), fp16 and byte caches: logits and greedy ids of row b of a batch of
    B are, bit for bit, those of the same cloud run at B = 1 through the same attention kernels (single_row_model)."""
    lmm, single = models(kv).on, single_row_model(kv)
    T = 16
    pc = clouds(B)
    _, toks = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    ids = np.stack([np.asarray(t[:T]) for t in toks])
    batch = teacher_forced(lmm, pc, ids, T)
    assert lmm.mesh_decoder.w4_streams() == NIBBLES and lmm.mesh_decoder.plan()["decode_version"] == 2
    for b in range(B):
        one = clouds(1, b)
        _, own = single.generate(one, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
        assert np.array_equal(np.asarray(own[0][:T]), ids[b]), f"B={B} kv={kv}: greedy ids of row {b} differ from the row alone"
        alone = teacher_forced(single, one, ids[b: b + 1], T)
        assert single.mesh_decoder.w4_streams() == NIBBLES and single.mesh_decoder.plan()["decode_version"] == 2
        assert same_bits(alone[:, 0], batch[:, b]), f"B={B} kv={kv} row {b}: logits differ at steps {sorted(set((alone[:, 0] != batch[:, b]).nonzero()[:, 0].tolist()))[:8]}"


def test_the_measured_rule_is_what_an_unset_knob_gives():
    """ER_W4_ROWS unset: csrc/er_w4_rule.h w4_streams (profiles/w4_bench.json) - the same rule tests/test_w4_cpu.py enumerates."""
    from test_w4_cpu import MEASURED_RULE
    p = models()
    lmm = make_lmm(p.sd, "mxfp4")
    names = ("qkv", "out_proj", "fc1", "fc2")
    for B in (1, 2, 4, 5):
        lmm.mesh_decoder.reserve(B, 64)
        assert lmm.mesh_decoder.w4_streams() == {n: int((i, B) in MEASURED_RULE) for i, n in enumerate(names)}, B
    pc = clouds(1)
    _, a = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=12, min_new_tokens=12)
    _, b = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=12, min_new_tokens=12)
    lmm.mesh_decoder.close()
    assert np.array_equal(np.asarray(a[0]), np.asarray(b[0]))


def test_queue_mode_and_score_match_the_fp16_run():
    from edgerunner_amd.provider import collate_fn
    p = models()
    jobs = [(clouds(1, i), 1000) for i in (0, 1, 2)]
    _, want = p.h.generate_queue(jobs, slots=2, tokenizer=object(), max_new_tokens=16, min_new_tokens=16, check_every=4)
    _, got = p.on.generate_queue(jobs, slots=2, tokenizer=object(), max_new_tokens=16, min_new_tokens=16, check_every=4)
    assert p.on.last_queue_stats["admissions"] == 3
    for j in range(3):
        assert np.array_equal(np.asarray(got[j]).reshape(-1), np.asarray(want[j]).reshape(-1)), (j, got[j], want[j])
    from edgerunner_amd import weights as W
    pc = W.synthetic_point_cloud(0, 2048)
    ids = np.asarray(want[0], dtype=np.int64).reshape(-1)
    data = collate_fn([{"cond": pc[0].numpy(), "num_faces": 1000, "coords": ids, "len": len(ids), "azimuth": 0, "path": None}], p.opt)
    ref, out = p.h.score(data), p.on.score(data)
    assert same_bits(ref["logits"], out["logits"]) and float(ref["loss_ce"]) == float(out["loss_ce"])


# ---------------------------------------------------------------------------------------------- 5. straight to the oracle
def test_fp4_context_against_the_cpu_oracle_on_dequantised_weights():
    """The one check that does not go through the fp16 kernels: the CPU oracle on the dequantised weights (K/V rounded to fp16 as the
    cache rounds them), at the bound tests/test_gpu_w8.py applies to this comparison for fp8 mode - fp4 mode is fast mode's arithmetic on
    another checkpoint.  On the project's synthetic checkpoint as it is (rounded to MXFP4), with the nibble kernels on."""
    import arae_oracle as O
    from edgerunner_amd import weights as W
    opt = small_opt()
    src = W.make_state_dict(opt, 0, "perturbed")
    lmm = make_lmm(src, "mxfp4", rows=1)
    T = 24
    sd = O.round_streamed_weights(w4_ref.dequantized_state_dict(src), torch.float16)      # the other streamed tensors as fast mode stores them
    pc = W.synthetic_point_cloud(0, 256)
    rec = {}
    want = O.lmm_generate_ids(sd, opt, pc, 1000, max_new_tokens=T, min_new_tokens=T, fwd=O.make_forward(sd, opt, kv_round=torch.float16),
                              record_logits=lambda t, s: rec.__setitem__(t, s.numpy()[0].copy())).numpy()[0]
    _, toks = lmm.generate(pc.to(DEV), 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    got = teacher_forced(lmm, pc.to(DEV), want[None, :], T).cpu().numpy()[:, 0]
    assert lmm.mesh_decoder.w4_streams() == NIBBLES
    lmm.mesh_decoder.close()
    err = max(float(np.abs(got[t] - rec[t]).max()) for t in range(T))
    print(f"fp4 context vs the oracle on dequantised weights: max|dlogit| {err:.3e} over {T} steps (largest |logit| {float(np.abs(got).max()):.2f})")
    assert np.array_equal(np.asarray(toks[0]), want), (toks[0], want)
    assert err <= ORACLE_BOUND


# ---------------------------------------------------------------------------------------------- 6. mode validation
def test_create_accepts_fp16_and_byte_caches_and_refuses_fp32():
    from edgerunner_amd import native
    from edgerunner_amd.shape_opt import NativeShapeOPT
    p = models()
    for kd in (torch.float16, "fp8"):
        NativeShapeOPT(p.on.dims, p.opt, torch.device(DEV), weight_dtype="fp4", kv_dtype=kd).close()
    for kd in (torch.float32, torch.bfloat16, "fp4"):
        with pytest.raises(native.NativeError, match=r"\(-5\).*fp4"):                  # ER_ERR_UNSUPPORTED
            NativeShapeOPT(p.on.dims, p.opt, torch.device(DEV), weight_dtype="fp4", kv_dtype=kd)


def test_fp4_cast_follows_the_checkpoint_rule():
    from edgerunner_amd import native
    from edgerunner_amd.models import LMM
    p = models()
    with env(ER_W4_ROWS=1):
        m = LMM(p.opt, DEV, precision=None)
        m.load_state_dict(p.sd, strict=True)
        pc = clouds(1)
        _, a = m.half().generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
        _, b = m.fp4().generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)      # rebuilt from the retained checkpoint
    _, want = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=8, min_new_tokens=8)
    assert m.precision == "mxfp4" and np.array_equal(np.asarray(b[0]), np.asarray(want[0])) and len(a[0]) == 8
    m.release_checkpoint()
    assert m.fp4() is m                                                                               # no change: nothing to rebuild
    with pytest.raises(native.NativeError, match="cannot be re-stored"):
        m.half()
    m.mesh_decoder.close()
