"""fp4 mode in the matrix-core batched forms: gemv_mfma_kernel<w4_t> on the tiled nibble copy (csrc/k_gemv_mfma.h, er_w4_tile_map.h).

Like tests/test_gpu_w4.py and tests/test_gpu_w8_batched.py this needs no numerical oracle and no tolerance: every e2m1 code times its
block's 2^e is an fp16 number, the nibble kernel rebuilds in registers the operand the fp16 kernel loads, and everything behind the
operand is the same code - so each comparison is bit equality with the fp16 form on the dequantised matrix (``kernels.gemv_form_w4``
against ``kernels.gemv_form``), and with a fast-mode context on the checkpoint tests/w4_ref.py dequantises.  Inputs are those of
tests/test_gpu_decode_proj.py, sentinels those of tests/test_gpu_w8_batched.py.

One deviation from the letter of the issue, on purpose: under ER_W4_BATCHED=1 ``w4_streams_batched()`` is all ones only where all four
projections run a matrix-core form.  At 5 .. 8 rows out_proj is the eight-row VALU pass (ER_FORM_ROWS8), which has no nibble form (out of
scope) and runs the fp16 copy, so the report says out_proj = 0 there - as ``w8_streams()`` does for fp8 mode."""
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
HID, INTER = 1536, 6144
HEADS, HD, LCAP = 16, 96, 64
NAN32, NAN16, NAN8 = 0x7FC00123, 0x7E01, 0x7F      # sentinels: NaN patterns no kernel produces
BATCHES = [5, 16, 17, 32, 33]                       # one half, a full half, two halves, a full group, a second group of one row
RAGGED = 501                                        # rows of the fc2 / out_proj matrices that are no multiple of 32 (nor of 16)
NAMES = ("qkv", "out_proj", "fc1", "fc2")


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def nat():
    from edgerunner_amd import native
    return native


# ---------------------------------------------------------------------------------------------- 1. the conversion table
def test_every_code_exponent_and_nibble_position_converts_to_the_fp16_copys_bits():
    """[1536][1536]: nibble position j of piece p of row r holds code (j + p + r) % 16, so every row has all 16 codes at all 8 positions;
    block b of row r has e = (b + 5 r + 11 * (r / 16 % 2)) % 23 - 15: all of -15 .. 7 along a row, another one in the neighbouring blocks
    and rows, and never the same in rows li and li + 16 of a 32-row tile (the difference is 91 = 22 mod 23) - a scale taken from the
    wrong block, row or row tile shows.  Rows 0, 23, 46, 69 hold only the codes +-1 .. +-7 at e = -15 and -14 (values 2^-16 .. 6 * 2^-14,
    the small ones fp16 subnormals).  Inputs O(1), mostly one sign."""
    from edgerunner_amd import kernels as K
    F = nat()
    r, k = torch.arange(HID)[:, None], torch.arange(HID)[None, :]
    codes = ((k % 8) + (k // 8) + r) % 16
    e = ((torch.arange(HID // 32)[None, :] + 5 * r + 11 * ((r // 16) % 2)) % 23 - 15).to(torch.int32)
    sub_rows = [0, 23, 46, 69]
    sub = torch.tensor([1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15])
    for i in sub_rows:
        codes[i] = sub[(torch.arange(HID) + i) % len(sub)]
        e[i] = (torch.arange(HID // 32) % 2 - 15).to(torch.int32)
    for p in range(8):
        assert all(set(codes[row, p::8].tolist()) == set(range(16)) for row in (1, 2, 700, 1535)), "every code at every nibble position"
    assert set(e[1].tolist()) == set(range(-15, 8)) and not bool((e[:-1] == e[1:]).all(dim=1).any())
    rows = torch.arange(HID)
    lo = rows[(rows % 32 < 16) & ~torch.isin(rows, torch.tensor(sub_rows))]
    lo = lo[~torch.isin(lo + 16, torch.tensor(sub_rows))]
    assert not bool((e[lo] == e[lo + 16]).any()), "rows li and li + 16 of a tile share an exponent"
    codes = codes.to(torch.uint8)
    nib = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    block = w4_ref.canonical_block(nib, (e + 127).to(torch.uint8))
    w32 = w4_ref.dequantize(nib, e)
    w16 = w32.half()
    assert torch.equal(w16.float(), w32) and bool(torch.isfinite(w16).all())                  # every value is an fp16 number
    tiny = w16[sub_rows].float().abs()
    assert float(tiny.min()) == 2.0 ** -16 and float(tiny.max()) == 6 * 2.0 ** -14 and bool((tiny < 2.0 ** -14).any())
    B = 5
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, HID, generator=g) + 1.5).to(DEV)                                      # O(1), mostly one sign: no row sums to zero
    zero = torch.zeros(B, HID, device=DEV)
    ref = K.gemv_form(F.ER_FORM_MFMA, F.ER_EPI_RESID, w16.to(DEV), B, x=x, bias=zero[0].clone(), resid=zero)["y"]
    got = K.gemv_form_w4(F.ER_FORM_MFMA, F.ER_EPI_RESID, block.to(DEV), HID, HID, B, x=x, bias=zero[0].clone(), resid=zero)["y"]
    assert bool(torch.isfinite(ref).all()) and float(ref[:, sub_rows].abs().min()) > 0.0, "the subnormal rows must show in the reference"
    bad = (ref.view(torch.int32) != got.view(torch.int32)).nonzero()
    assert bad.numel() == 0, (len(bad), [(b, r_, float(ref[b, r_]), float(got[b, r_])) for b, r_ in bad[:6].tolist()])
    assert torch.equal(ref, got)


# ---------------------------------------------------------------------------------------------- 2. every matrix-core form
@functools.lru_cache(maxsize=None)
def data():
    """test_gpu_decode_proj's matrices (real N: 4608 / 1536 / 6144 / 1536) quantised by the library's own quantiser, with rows and blocks
    of other exponents, plus the first RAGGED rows of fc2 / out_proj as matrices of their own."""
    import test_gpu_decode_proj as P
    from edgerunner_amd import kernels as K
    d = P.data()
    w = SimpleNamespace(blk={}, w16={}, n={}, k={}, bias=dict(d.bias), base=d)
    for name in ("qkv", "out", "fc1", "fc2"):
        m = d.w[name].clone()
        m[5] *= 40.0
        m[6] *= 1e-4
        m[37::97] *= 6.0
        m[:, 96:128] *= 9.0
        m[21, 32:64] *= 300.0
        m[7, 64:96] = 0.0
        w.blk[name], e, w.w16[name] = K.w4_quantize(m, device=DEV)
        w.n[name], w.k[name] = m.shape
        assert len(set(e.flatten().cpu().tolist())) >= 6
    for name in ("out", "fc2"):
        n, k = w.n[name], w.k[name]
        nib, sc = K.w4_block_parts(w.blk[name], n, k)
        w.blk[name + "_r"] = torch.cat((nib[:RAGGED].reshape(-1), sc[:RAGGED].reshape(-1))).contiguous()
        w.w16[name + "_r"] = w.w16[name][:RAGGED].contiguous()
        w.n[name + "_r"], w.k[name + "_r"] = RAGGED, k
        w.bias[name + "_r"] = d.bias[name][:RAGGED].contiguous()
    return w


def sentinel_caches(B, cache):
    if cache == "fp8":
        kc = torch.full((B, HEADS, LCAP, HD), NAN8, dtype=torch.uint8, device=DEV)
    elif cache == "fp32":
        kc = torch.full((B, HEADS, LCAP, HD), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    else:
        kc = torch.full((B, HEADS, LCAP, HD), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    return kc, kc.clone(), torch.full((B, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)


def launch(name, form, B, nibbles, cache="fp16", pro="ln", rows=None):
    """One launch through er_k_gemv_form (the fp16 dequantised matrix) or er_k_gemv_form_w4 (the canonical block) on rows `rows`
    (default: the first B) of the shared inputs: dict of outputs.  Caller-visible buffers the kernels write sparsely (caches, q, the fc1
    image) start as sentinels."""
    import test_gpu_decode_proj as P
    from edgerunner_amd import kernels as K
    F, w = nat(), data()
    d, base = w.base, name.split("_")[0]
    rows = list(range(B)) if rows is None else list(rows)
    epi = {"qkv": F.ER_EPI_QKV, "out": F.ER_EPI_RESID, "fc1": F.ER_EPI_RELU, "fc2": F.ER_EPI_RESID}[base]
    n = w.n[name]
    pos = [d.pos[i] for i in rows]
    kw = dict(bias=w.bias[name])
    if base in ("qkv", "fc1"):
        if pro == "embed":
            kw.update(embed=(d.embd, d.posemb, [d.tok[i] for i in rows], pos))
        else:
            kw.update(x=d.x[rows].contiguous(), ln=(d.lw, d.lb))
        kw.update(return_xnorm=True, prep_xt=(form == "xt"))
    else:
        x = (d.att if base == "out" else d.f)[rows].contiguous()
        kw.update(x=K.xt_pack_image(x) if form in ("narrow", "defer") else x, resid=d.r[rows][:, :n].contiguous())
    if base == "qkv":
        kc, vc, qo = sentinel_caches(B, cache)
        kw["qkv"] = (kc, vc, pos, qo)
    if base == "fc1" and form == "xt":
        kw["xt_out_image"] = torch.full(((B + 31) // 32, n // 4, 32, 8), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    f = getattr(F, P.FORMS[form])
    o = K.gemv_form_w4(f, epi, w.blk[name], n, w.k[name], B, **kw) if nibbles else K.gemv_form(f, epi, w.w16[name], B, **kw)
    if base == "qkv":
        o["kc"], o["vc"] = kc, vc
    if "part" in o:                                            # the rows of the block the launch defines (the rest is torch.empty)
        o["part"] = P.part_rows(o["part"], B, w.k[name] // 384, n)
    return o


def assert_pair_equal(ref, got, what):
    assert set(ref) == set(got) and len(ref) > 0, (what, sorted(ref), sorted(got))
    for k in ref:
        assert same_bits(ref[k], got[k]), f"{what}: {k} differs in {int((ref[k].contiguous().view(torch.uint8) != got[k].contiguous().view(torch.uint8)).sum())} bytes"


def assert_cache_written_at_pos_only(o, B, cache):
    sentinel_dtype, sentinel = (torch.uint8, NAN8) if cache == "fp8" else (torch.int16, NAN16)
    pos = data().base.pos[:B]
    for c in (o["kc"], o["vc"]):
        bits = c.view(sentinel_dtype)
        outside = torch.ones((B, HEADS, LCAP, HD), dtype=torch.bool, device=DEV)
        for b, p in enumerate(pos):
            outside[b, :, p, :] = False
        assert bool((bits[outside] == sentinel).all()), "the cache was written outside [b, :, pos[b], :]"
        assert not bool((bits[~outside] == sentinel).any()), "an element of the new key row was not written"
    assert not bool((o["q"].view(torch.int32) == NAN32).any())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("pro", ["ln", "embed"])
@pytest.mark.parametrize("cache", ["fp16", "fp8"])
@pytest.mark.parametrize("form", ["mfma", "xt"])
def test_qkv_forms_equal_the_fp16_kernels(form, cache, pro, B):
    ref, got = launch("qkv", form, B, False, cache, pro), launch("qkv", form, B, True, cache, pro)
    assert {"q", "kc", "vc", "xnorm"} <= set(got) and ("prep_xt" in got) == (form == "xt")
    assert_pair_equal(ref, got, f"qkv {form} {cache} cache {pro} B={B}")
    assert_cache_written_at_pos_only(got, B, cache)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("form", ["mfma", "xt"])
def test_fc1_forms_equal_the_fp16_kernels(form, B):
    from edgerunner_amd import kernels as K
    ref, got = launch("fc1", form, B, False), launch("fc1", form, B, True)
    assert ("xt_out" if form == "xt" else "y") in got
    assert_pair_equal(ref, got, f"fc1 {form} B={B}")
    if form == "xt":                                              # rows the batch does not have: untouched
        hi, lo = K.xt_unpack_image(got["xt_out"])
        assert bool((hi[B:].view(torch.int16) == NAN16).all()) and bool((lo[B:].view(torch.int16) == NAN16).all())
        assert not bool((hi[:B].view(torch.int16) == NAN16).any())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name,form", [("fc2", "mfma"), ("fc2", "narrow"), ("fc2", "defer"), ("out", "mfma"), ("out", "defer"),
                                       ("fc2_r", "mfma"), ("fc2_r", "narrow"), ("fc2_r", "defer"), ("out_r", "mfma"), ("out_r", "defer")])
def test_fc2_and_out_proj_forms_equal_the_fp16_kernels(name, form, B):
    """fc2 mfma: 4 K-ranges + the finish kernel; narrow: 16 + the finish; defer: the raw partials, compared slice by slice.  *_r: 501 rows."""
    ref, got = launch(name, form, B, False), launch(name, form, B, True)
    assert ("part" if form == "defer" else "y") in got
    assert_pair_equal(ref, got, f"{name} {form} B={B}")
    assert not bool(torch.isnan(got["part" if form == "defer" else "y"]).any())


# ---------------------------------------------------------------------------------------------- 3. row invariance
def test_a_row_of_a_batch_of_33_equals_the_row_in_a_batch_of_5():
    """fc1 ER_FORM_MFMA and qkv ER_FORM_MFMA_XT into a byte cache: rows 0, 14, 15 (first half), 16, 31 (second half) and 32 (second group)
    of a batch of 33, launched again as a batch of 5 / as rows of their own."""
    big = launch("fc1", "mfma", 33, True)["y"]
    for rows in ([0, 14, 15, 16, 31], [32, 1, 17, 30, 2]):
        small = launch("fc1", "mfma", 5, True, rows=rows)["y"]
        for i, b in enumerate(rows):
            assert same_bits(small[i], big[b]), ("fc1", b)
    big = launch("qkv", "xt", 33, True, cache="fp8")
    pos = data().base.pos
    for rows in ([0, 14, 15, 16, 31], [32, 1, 17, 30, 2]):
        small = launch("qkv", "xt", 5, True, cache="fp8", rows=rows)
        for i, b in enumerate(rows):
            assert same_bits(small["q"][i], big["q"][b]) and same_bits(small["xnorm"][i], big["xnorm"][b]), ("qkv", b)
            for c in ("kc", "vc"):
                assert same_bits(small[c][i, :, pos[b]], big[c][b, :, pos[b]]), (c, b)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_come_before_any_launch():
    from edgerunner_amd import kernels as K
    F, w = nat(), data()
    d = w.base
    B = 5
    kc, vc, qo = sentinel_caches(B, "fp16")
    ln = dict(x=d.x[:B].contiguous(), ln=(d.lw, d.lb))
    y = dict(x=d.f[:B].contiguous(), resid=d.r[:B].contiguous(), bias=w.bias["fc2"])
    with pytest.raises(F.NativeError, match="row forms"):                        # the VALU batched kernel has no nibble form
        K.gemv_form_w4(F.ER_FORM_VALU, F.ER_EPI_QKV, w.blk["qkv"], 3 * HID, HID, B, bias=w.bias["qkv"], qkv=(kc, vc, d.pos[:B], qo), **ln)
    with pytest.raises(F.NativeError, match="row forms"):
        K.gemv_form_w4(F.ER_FORM_VALU, F.ER_EPI_RESID, w.blk["fc2"], HID, INTER, B, **y)
    with pytest.raises(F.NativeError, match="er_k_gemv_form_w4"):                # nor has the eight-row out_proj
        K.gemv_form_w4(F.ER_FORM_ROWS8, F.ER_EPI_RESID, w.blk["out"], HID, HID, B, x=d.att[:B].contiguous(), resid=d.r[:B].contiguous(),
                       bias=w.bias["out"], nw=3, rw=1)
    with pytest.raises(F.NativeError):                                           # the lm_head: not quantised, and no matrix-core form
        K.gemv_form_w4(F.ER_FORM_MFMA, F.ER_EPI_STORE, w.blk["out"], HID, HID, B, **ln)
    with pytest.raises(F.NativeError, match="lm_head"):
        K.gemv_form_w4(F.ER_FORM_ROW, F.ER_EPI_STORE, w.blk["out"], HID, HID, 1, x=d.x[:1].contiguous(), ln=(d.lw, d.lb), nw=4, rw=1)
    out = torch.full((B, 48), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    for k_bad in (1536 + 96, 1536 + 768, 3072):                                  # K that is no multiple of the K-range of 1536 (the first two: multiples of 96 / 384)
        blk = torch.zeros(48 * k_bad // 2 + 48 * k_bad // 32, dtype=torch.uint8, device=DEV)
        with pytest.raises(F.NativeError):
            K.gemv_form_w4(F.ER_FORM_MFMA, F.ER_EPI_RESID, blk, 48, k_bad, B, x=torch.zeros(B, k_bad, device=DEV), resid=out.clone(), bias=torch.zeros(48, device=DEV))
    kc32, vc32, _ = sentinel_caches(B, "fp32")
    with pytest.raises(F.NativeError, match="fp32"):                             # an fp32 cache
        K.gemv_form_w4(F.ER_FORM_MFMA, F.ER_EPI_QKV, w.blk["qkv"], 3 * HID, HID, B, bias=w.bias["qkv"], qkv=(kc32, vc32, d.pos[:B], qo), **ln)
    torch.cuda.synchronize()
    assert bool((kc.view(torch.int16) == NAN16).all()) and bool((vc.view(torch.int16) == NAN16).all()) and bool((qo.view(torch.int32) == NAN32).all())
    assert bool((kc32.view(torch.int32) == NAN32).all()) and bool((vc32.view(torch.int32) == NAN32).all())


# ---------------------------------------------------------------------------------------------- 5. end to end
T = 16
ALL = dict.fromkeys(NAMES, 1)
NONE = dict.fromkeys(NAMES, 0)


def mfma_forms(B):
    """The projections whose batched form is a matrix-core form at B rows: out_proj is the eight-row VALU pass up to 8 rows."""
    return {n: int(B > 4 and (n != "out_proj" or B > 8)) for n in NAMES}


def make_lmm(sd, precision, kv=None, knob=None):
    """A 2-layer LMM on sd; knob: ER_W4_BATCHED at er_create (None: unset)."""
    import test_gpu_w4 as W4T
    from edgerunner_amd.models import LMM
    with W4T.env(ER_W4_BATCHED=knob, ER_W4_ROWS=None):
        m = LMM(W4T.small_opt(), DEV, precision=precision, kv_precision=kv)
    m.load_state_dict(sd, strict=True)
    return m


_MODELS = {}


def models(kv=None):
    """fp4 contexts under ER_W4_BATCHED=1 and =0 on the checkpoint of tests/test_gpu_w4.py (blocks of very different exponents), and the
    fast-mode context on the checkpoint w4_ref dequantises.  Made once per cache type and closed when this file is done."""
    import test_gpu_w4 as W4T
    if kv not in _MODELS:
        sd, deq = W4T.checkpoint()
        _MODELS[kv] = SimpleNamespace(opt=W4T.small_opt(), sd=sd, deq=deq, on=make_lmm(sd, "mxfp4", kv, 1), off=make_lmm(sd, "mxfp4", kv, 0),
                                      h=make_lmm(deq, "fp16", kv))
    return _MODELS[kv]


@pytest.fixture(scope="module", autouse=True)
def release_contexts():
    """A context holds several GiB of device memory (caches and workspaces of the shapes it reserved), and the suite runs in one
    process: the six of this file are given back when it is done."""
    yield
    for p in _MODELS.values():
        for m in (p.on, p.off, p.h):
            m.mesh_decoder.close()
    _MODELS.clear()
    torch.cuda.empty_cache()


def ids_of(toks, n):
    return np.stack([np.asarray(t[:n]) for t in toks])


@pytest.mark.parametrize("kv", [None, "fp8"])
@pytest.mark.parametrize("B", [8, 17])
def test_fp4_context_streams_nibbles_in_the_batched_step(B, kv):
    """THE test that fails without the feature: ER_W4_BATCHED=1 streams nibbles in every matrix-core form of the step (B = 8: qkv, fc1, fc2
    - out_proj is the eight-row VALU pass; B = 17: all four, out_proj and fc2 in their narrow forms) and the logits are, bit for bit,
    those of the same context under =0 and of fast mode on the dequantised checkpoint; so are the graph-replayed greedy ids."""
    import test_gpu_w4 as W4T
    p = models(kv)
    pc = W4T.clouds(B)
    _, toks = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    ids = ids_of(toks, T)
    ref = W4T.teacher_forced(p.h, pc, ids, T)
    for name, lmm, want in (("ER_W4_BATCHED=1", p.on, mfma_forms(B)), ("ER_W4_BATCHED=0", p.off, NONE)):
        got = W4T.teacher_forced(lmm, pc, ids, T)
        dec = lmm.mesh_decoder
        assert dec.plan()["batched"] == 1 and bool(torch.isfinite(got).all())
        assert dec.w4_streams_batched() == want, (name, B, dec.w4_streams_batched())
        assert dec.w4_streams() == NONE, "er_ctx_w4_streams reports the row forms only"
        assert same_bits(ref, got), f"{name} B={B} kv={kv}: logits differ at steps {sorted(set((ref != got).nonzero()[:, 0].tolist()))[:8]}"
        _, own = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)       # the step graph
        assert np.array_equal(ids_of(own, T), ids), name
    assert mfma_forms(17) == ALL and p.h.mesh_decoder.w4_streams_batched() == NONE


def test_fp4_context_on_row_major_inputs(monkeypatch):
    """ER_XT=0 at the reserve: ER_FORM_MFMA everywhere, fc2 with its finish kernel - the forms the tiled path does not launch."""
    import test_gpu_w4 as W4T
    monkeypatch.setenv("ER_XT", "0")
    p = models()
    B, n = 17, 8
    pc = W4T.clouds(B)
    for m in (p.h, p.on):
        m.mesh_decoder.reserve(1, 64)                              # the next reserve reads the reserve switches again
    _, toks = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=n, min_new_tokens=n)
    ids = ids_of(toks, n)
    ref, got = W4T.teacher_forced(p.h, pc, ids, n), W4T.teacher_forced(p.on, pc, ids, n)
    assert p.on.mesh_decoder.w4_streams_batched() == ALL and same_bits(ref, got)
    for m in (p.h, p.on):
        m.mesh_decoder.reserve(1, 64)


# ---------------------------------------------------------------------------------------------- 6. the unset knob
def test_the_measured_rule_is_what_an_unset_knob_gives():
    """ER_W4_BATCHED unset: csrc/er_w4_rule.h w4_streams_batched(proj, B, -1) (profiles/w4_batched_bench.json), as tests/test_w4_tile_cpu.py
    enumerates it, for the projections that run a matrix-core form at B rows."""
    import test_gpu_w4 as W4T
    from test_w4_tile_cpu import measured_batched_rule
    p = models()
    lmm = make_lmm(p.sd, "mxfp4")
    dec = lmm.mesh_decoder
    for B in (5, 8, 16, 32):
        dec.reserve(B, 64)
        forms = mfma_forms(B)
        assert dec.plan()["batched"] == 1
        assert dec.w4_streams_batched() == {n: int(bool(forms[n]) and measured_batched_rule(i, B)) for i, n in enumerate(NAMES)}, B
        assert dec.w4_streams() == NONE
    dec.reserve(4, 64)
    assert dec.w4_streams_batched() == NONE and dec.plan()["batched"] == 0
    pc = W4T.clouds(8)
    _, a = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=12, min_new_tokens=12)
    _, b = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=12, min_new_tokens=12)
    dec.close()
    assert np.array_equal(ids_of(a, 12), ids_of(b, 12))


# ---------------------------------------------------------------------------------------------- 7. memory
def test_nibble_streamed_projections_get_no_fp16_tiled_copy():
    """reserve(8, 64) on fresh fp4 contexts: under ER_W4_BATCHED=0 the fp16 tiled copies of all four matrices (2 bytes per weight), under =1
    tiled nibbles for qkv, fc1 and fc2 (1664 bytes per 32 x 96 weights) and fp16 for out_proj only.  Strictly smaller, nothing more is
    asserted; both drops are printed."""
    import test_gpu_lifetime as L
    p = models()
    L.touch_stream_pool()
    drops = {}
    for knob in (0, 1):
        lmm = make_lmm(p.sd, "mxfp4", knob=knob)
        dec = lmm.mesh_decoder
        dec.reserve(1, 64)
        free0 = L.free_bytes()
        dec.reserve(8, 64)
        drops[knob] = free0 - L.free_bytes()
        assert dec.w4_streams_batched() == (mfma_forms(8) if knob else NONE)
        dec.close()
    print(f"free-memory drop of reserve(8, 64) in fp4 mode: ER_W4_BATCHED=0 {drops[0]} bytes, =1 {drops[1]} bytes")
    assert drops[1] < drops[0], drops


# ---------------------------------------------------------------------------------------------- 8. reload and the other modes
def test_reload_invalidates_the_tiled_nibble_copies():
    """A tensor loaded behind a prefill leaves the tiled nibble copies stale: the next step of that plan is an error (never the old
    nibbles, never the fp16 copy quietly).  A full reload and the next batched generate() equal fast mode on the new dequantised
    checkpoint."""
    import test_gpu_w4 as W4T
    from edgerunner_amd import native
    p = models()
    lmm = make_lmm(p.sd, "mxfp4", knob=1)
    dec = lmm.mesh_decoder
    B = 9
    pc = W4T.clouds(B)
    cond = lmm.encode_cond(pc, [1000] * B)["cond_embeds"]
    bos = torch.full((B, 1), lmm.opt.bos_token_id, dtype=torch.long)
    dec.prefill(torch.cat((cond, dec.embd(bos)), dim=1), 8)
    assert dec.w4_streams_batched() == ALL
    dec.feed([5] * B)                                               # the copies are there: a step runs
    sd2, deq2 = dict(p.sd), dict(p.deq)                              # other weights in two matrices (only those are dequantised again)
    key = "mesh_decoder.model.layers.0.fc1.weight"
    for i, k in enumerate((key, "mesh_decoder.model.layers.1.self_attn.q_proj.weight")):
        g = torch.Generator().manual_seed(900 + i)
        t = p.sd[k] + 0.03 * torch.randn(p.sd[k].shape, generator=g)
        t[:, 32:64] *= 7.0
        sd2[k] = t
        nib, _, e, _ = w4_ref.quantize(t)
        deq2[k] = w4_ref.dequantize(nib, e)
    native.load_tensor(dec.lib.er_load_tensor, dec._ctx, key, sd2[key])
    with pytest.raises(native.NativeError):
        dec.feed([5] * B)
    lmm.load_state_dict(sd2, strict=True)
    h2 = make_lmm(deq2, "fp16")
    _, a = lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=12, min_new_tokens=12)
    _, b = h2.generate(pc, 1000, tokenizer=object(), max_new_tokens=12, min_new_tokens=12)
    _, old = p.h.generate(pc, 1000, tokenizer=object(), max_new_tokens=12, min_new_tokens=12)
    assert dec.w4_streams_batched() == ALL
    dec.close()
    h2.mesh_decoder.close()
    assert np.array_equal(ids_of(a, 12), ids_of(b, 12))
    assert not np.array_equal(ids_of(a, 12), ids_of(old, 12)), "the two checkpoints must decode differently for the comparison to mean anything"


def test_queue_mode_and_score_match_the_fp16_run():
    from edgerunner_amd import weights as W
    from edgerunner_amd.provider import collate_fn
    import test_gpu_w4 as W4T
    p = models()
    jobs = [(W4T.clouds(1, i), 1000) for i in range(8)]
    _, want = p.h.generate_queue(jobs, slots=6, tokenizer=object(), max_new_tokens=16, min_new_tokens=16, check_every=4)
    _, got = p.on.generate_queue(jobs, slots=6, tokenizer=object(), max_new_tokens=16, min_new_tokens=16, check_every=4)
    assert p.on.last_queue_stats["admissions"] == 8
    assert p.on.mesh_decoder.w4_streams_batched() == mfma_forms(6) and p.on.mesh_decoder.plan()["batched"] == 1
    for j in range(8):
        assert np.array_equal(np.asarray(got[j]).reshape(-1), np.asarray(want[j]).reshape(-1)), (j, got[j], want[j])
    pc = W.synthetic_point_cloud(0, 2048)
    ids = np.asarray(want[0], dtype=np.int64).reshape(-1)
    data_ = collate_fn([{"cond": pc[0].numpy(), "num_faces": 1000, "coords": ids, "len": len(ids), "azimuth": 0, "path": None}], p.opt)
    ref, out = p.h.score(data_), p.on.score(data_)
    assert same_bits(ref["logits"], out["logits"]) and float(ref["loss_ce"]) == float(out["loss_ce"])
