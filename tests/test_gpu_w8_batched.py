"""fp8 mode in the matrix-core batched forms: gemv_mfma_kernel<w8_t> on the tiled byte copy (csrc/k_gemv_mfma.h, er_w8_tile_map.h).

Like tests/test_gpu_w8.py this needs no numerical oracle and no tolerance: every e4m3 byte times its row's 2^e is an fp16 number, the
byte kernel rebuilds in registers the operand the fp16 kernel loads, and everything behind the operand is the same code - so each
comparison is bit equality with the fp16 form on the dequantised matrix (``kernels.gemv_form_w8`` against ``kernels.gemv_form``), and
with a fast-mode context on the checkpoint tests/w8_ref.py dequantises.  Inputs are those of tests/test_gpu_decode_proj.py."""
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

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID, INTER = 1536, 6144
HEADS, HD, LCAP = 16, 96, 64
NAN32, NAN16, NAN8 = 0x7FC00123, 0x7E01, 0x7F      # sentinels: NaN patterns no kernel produces
BATCHES = [5, 16, 17, 32, 33]                       # one half, a full half, two halves, a full group, a second group of one row
RAGGED = 501                                        # rows of the fc2 / out_proj matrices that are no multiple of 32 (nor of 16)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def nat():
    from edgerunner_amd import native
    return native


# ---------------------------------------------------------------------------------------------- 1. the conversion table
def test_every_code_and_exponent_converts_to_the_fp16_copys_bits():
    """All 254 finite e4m3 codes in every row, rows cycling e = -15 .. 7, and rows 0, 23, 46, 69 (e = -15) holding nothing but the bytes
    0x01 .. 0x07 and 0x81 .. 0x87: every weight of those rows is an fp16 subnormal (2^-24 .. 7 * 2^-24).  Inputs of O(1): a conversion
    that flushed or rounded a subnormal would change those rows' fp32 sums (about 1e-4 against a resolution of 1e-11)."""
    from edgerunner_amd import kernels as K
    F = nat()
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.int64)
    assert len(codes) == 254
    r, k = torch.arange(HID)[:, None], torch.arange(HID)[None, :]
    q = codes[(k + 37 * r) % 254]                                   # every code in every row, at shifting byte lanes
    sub = torch.tensor([1, 2, 3, 4, 5, 6, 7, 0x81, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87], dtype=torch.int64)
    sub_rows = [0, 23, 46, 69]
    for i in sub_rows:
        q[i] = sub[(torch.arange(HID) + i) % len(sub)]
    q = q.to(torch.uint8)
    e = (torch.arange(HID) % 23 - 15).to(torch.int32)
    assert set(e.tolist()) == set(range(-15, 8)) and all(int(e[i]) == -15 for i in sub_rows)
    ws = torch.ldexp(torch.ones(HID), e)
    w32 = w8_ref.dequantize(q, e)
    w16 = w32.half()
    assert torch.equal(w16.float(), w32) and bool(torch.isfinite(w16).all())                 # every value is an fp16 number
    tiny = w16[sub_rows].float().abs()
    assert float(tiny.max()) <= 7 * 2.0 ** -24 and float(tiny.min()) >= 2.0 ** -24            # fp16 subnormals, none of them zero
    B = 5
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, HID, generator=g) + 1.5).to(DEV)                                      # O(1), mostly one sign: no row sums to zero
    zero = torch.zeros(B, HID, device=DEV)
    ref = K.gemv_form(F.ER_FORM_MFMA, F.ER_EPI_RESID, w16.to(DEV), B, x=x, bias=zero[0].clone(), resid=zero)["y"]
    got = K.gemv_form_w8(F.ER_FORM_MFMA, F.ER_EPI_RESID, q.to(DEV), ws.to(DEV), B, x=x, bias=zero[0].clone(), resid=zero)["y"]
    assert bool(torch.isfinite(ref).all()) and float(ref[:, sub_rows].abs().min()) > 0.0, "the subnormal rows must show in the reference"
    bad = (ref.view(torch.int32) != got.view(torch.int32)).nonzero()
    assert bad.numel() == 0, [(b, r_, int(e[r_]), float(ref[b, r_]), float(got[b, r_])) for b, r_ in bad[:6].tolist()]
    assert torch.equal(ref, got)


# ---------------------------------------------------------------------------------------------- 2. every matrix-core form
@functools.lru_cache(maxsize=None)
def data():
    """test_gpu_decode_proj's matrices (real N: 4608 / 1536 / 6144 / 1536) quantised by the library's own quantiser, with rows of other
    exponents, plus the first RAGGED rows of fc2 / out_proj as matrices of their own."""
    import test_gpu_decode_proj as P
    from edgerunner_amd import kernels as K
    d = P.data()
    w = SimpleNamespace(q={}, ws={}, w16={}, bias=dict(d.bias), base=d)
    for name in ("qkv", "out", "fc1", "fc2"):
        m = d.w[name].clone()
        m[5] *= 40.0
        m[6] *= 1e-4
        m[37::97] *= 6.0
        w.q[name], e, w.w16[name], w.ws[name] = K.w8_quantize(m, device=DEV)
        assert len(set(e.cpu().tolist())) >= 3
    for name in ("out", "fc2"):
        w.q[name + "_r"], w.ws[name + "_r"], w.w16[name + "_r"] = (t[:RAGGED].contiguous() for t in (w.q[name], w.ws[name], w.w16[name]))
        w.bias[name + "_r"] = d.bias[name][:RAGGED].contiguous()
    return w


def run_pair(name, form, B, cache="fp16"):
    """The same launch through er_k_gemv_form (fp16 dequantised matrix) and er_k_gemv_form_w8 (bytes + scales): two dicts of outputs.
    Caller-visible buffers the kernels write sparsely (caches, q, the fc1 image) start as sentinels."""
    import test_gpu_decode_proj as P
    from edgerunner_amd import kernels as K
    F, w = nat(), data()
    d, base = w.base, name.split("_")[0]
    epi = {"qkv": F.ER_EPI_QKV, "out": F.ER_EPI_RESID, "fc1": F.ER_EPI_RELU, "fc2": F.ER_EPI_RESID}[base]
    n = w.q[name].shape[0]
    outs = []
    for bytes_ in (False, True):
        kw = dict(bias=w.bias[name])
        if base in ("qkv", "fc1"):
            kw.update(x=d.x[:B].contiguous(), ln=(d.lw, d.lb), return_xnorm=True, prep_xt=(form == "xt"))
        else:
            x = (d.att if base == "out" else d.f)[:B].contiguous()
            kw.update(x=K.xt_pack_image(x) if form in ("narrow", "defer") else x, resid=d.r[:B, :n].contiguous())
        if base == "qkv":
            if cache == "fp8":
                kc = torch.full((B, HEADS, LCAP, HD), NAN8, dtype=torch.uint8, device=DEV)
            else:
                kc = torch.full((B, HEADS, LCAP, HD), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
            vc = kc.clone()
            qo = torch.full((B, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
            kw["qkv"] = (kc, vc, d.pos[:B], qo)
        if base == "fc1" and form == "xt":
            kw["xt_out_image"] = torch.full(((B + 31) // 32, n // 4, 32, 8), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
        f = getattr(F, P.FORMS[form])
        o = K.gemv_form_w8(f, epi, w.q[name], w.ws[name], B, **kw) if bytes_ else K.gemv_form(f, epi, w.w16[name], B, **kw)
        if base == "qkv":
            o["kc"], o["vc"] = kc, vc
        if "part" in o:                                            # the rows of the block the launch defines (the rest is torch.empty)
            o["part"] = P.part_rows(o["part"], B, (INTER if base == "fc2" else HID) // 384, n)
        outs.append(o)
    return outs


def assert_pair_equal(ref, got, what):
    assert set(ref) == set(got) and len(ref) > 0, (what, sorted(ref), sorted(got))
    for k in ref:
        assert same_bits(ref[k], got[k]), f"{what}: {k} differs in {int((ref[k].contiguous().view(torch.uint8) != got[k].contiguous().view(torch.uint8)).sum())} bytes"


def assert_cache_written_at_pos_only(o, B, sentinel_dtype, sentinel):
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
@pytest.mark.parametrize("cache", ["fp16", "fp8"])
@pytest.mark.parametrize("form", ["mfma", "xt"])
def test_qkv_forms_equal_the_fp16_kernels(form, cache, B):
    ref, got = run_pair("qkv", form, B, cache)
    assert {"q", "kc", "vc", "xnorm"} <= set(got)
    assert_pair_equal(ref, got, f"qkv {form} {cache} cache B={B}")
    assert_cache_written_at_pos_only(got, B, torch.uint8 if cache == "fp8" else torch.int16, NAN8 if cache == "fp8" else NAN16)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("form", ["mfma", "xt"])
def test_fc1_forms_equal_the_fp16_kernels(form, B):
    from edgerunner_amd import kernels as K
    ref, got = run_pair("fc1", form, B)
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
    ref, got = run_pair(name, form, B)
    assert ("part" if form == "defer" else "y") in got
    assert_pair_equal(ref, got, f"{name} {form} B={B}")
    assert not bool(torch.isnan(got["part" if form == "defer" else "y"]).any())


# ---------------------------------------------------------------------------------------------- 3. what has no byte kernel
def test_valu_and_rows8_forms_are_refused_and_write_nothing():
    from edgerunner_amd import kernels as K
    F, w = nat(), data()
    d = w.base
    B = 5
    kc = torch.full((B, HEADS, LCAP, HD), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    vc, qo = kc.clone(), torch.full((B, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    with pytest.raises(F.NativeError, match="er_k_gemv_form_w8"):
        K.gemv_form_w8(F.ER_FORM_VALU, F.ER_EPI_QKV, w.q["qkv"], w.ws["qkv"], B, x=d.x[:B].contiguous(), ln=(d.lw, d.lb), bias=w.bias["qkv"],
                       qkv=(kc, vc, d.pos[:B], qo))
    with pytest.raises(F.NativeError, match="er_k_gemv_form_w8"):
        K.gemv_form_w8(F.ER_FORM_ROWS8, F.ER_EPI_RESID, w.q["out"], w.ws["out"], B, x=d.att[:B].contiguous(), resid=d.r[:B].contiguous(),
                       bias=w.bias["out"], nw=3, rw=1)
    with pytest.raises(F.NativeError, match="er_k_gemv_form_w8"):
        K.gemv_form_w8(F.ER_FORM_VALU, F.ER_EPI_RESID, w.q["fc2"], w.ws["fc2"], B, x=d.f[:B].contiguous(), resid=d.r[:B].contiguous(), bias=w.bias["fc2"])
    torch.cuda.synchronize()
    assert bool((kc.view(torch.int16) == NAN16).all()) and bool((vc.view(torch.int16) == NAN16).all()) and bool((qo.view(torch.int32) == NAN32).all())


# ---------------------------------------------------------------------------------------------- 4. end to end
T = 8


@functools.lru_cache(maxsize=None)
def checkpoint():
    from edgerunner_amd import weights as W
    from edgerunner_amd.options import config_defaults
    opt = dataclasses.replace(config_defaults["ArAE"], num_layers=2, generate_mode="greedy")
    sd = dict(W.make_state_dict(opt, 0, "perturbed"))
    for k in [k for k in sd if ".layers." in k and k.endswith(w8_ref.W8_SUFFIXES)]:      # rows of other exponents than their neighbours
        t = sd[k].clone()
        t[3::97] *= 6.0
        t[5::89] *= 0.02
        sd[k] = t
    return SimpleNamespace(opt=opt, sd=sd, deq=w8_ref.dequantized_state_dict(sd))


@functools.lru_cache(maxsize=None)
def model(precision, kv=None, knob=None):
    """A 2-layer context; fp8 ones on the source checkpoint, fp16 ones on the dequantised one.  knob: ER_W8_BATCHED as er_create reads it."""
    from edgerunner_amd.models import LMM
    c = checkpoint()
    old = os.environ.get("ER_W8_BATCHED")
    try:
        os.environ.pop("ER_W8_BATCHED", None)
        if knob is not None:
            os.environ["ER_W8_BATCHED"] = knob
        lmm = LMM(c.opt, DEV, precision=precision, kv_precision=kv)
    finally:
        os.environ.pop("ER_W8_BATCHED", None)
        if old is not None:
            os.environ["ER_W8_BATCHED"] = old
    lmm.load_state_dict(c.sd if precision == "fp8" else c.deq, strict=True)
    return lmm


def clouds(B):
    from edgerunner_amd import weights as W
    return torch.cat([W.synthetic_point_cloud(i, 256) for i in range(B)]).to(DEV)


def teacher_forced(lmm, pc, ids):
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
    return torch.stack(out), dec.w8_streams(), dec.plan()


def assert_context_pair(ref_lmm, w8_lmm, B, want_streams):
    pc = clouds(B)
    for m in (ref_lmm, w8_lmm):
        m.mesh_decoder.reserve(1, 64)                               # the next reserve reads the reserve switches (ER_XT) again
    _, ref_toks = ref_lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)      # greedy, under the step graph
    _, got_toks = w8_lmm.generate(pc, 1000, tokenizer=object(), max_new_tokens=T, min_new_tokens=T)
    ids = np.stack([np.asarray(t[:T]) for t in ref_toks])
    assert np.array_equal(ids, np.stack([np.asarray(t[:T]) for t in got_toks])), f"B={B}: greedy ids differ"
    ref, ref_streams, _ = teacher_forced(ref_lmm, pc, ids)
    got, streams, plan = teacher_forced(w8_lmm, pc, ids)
    assert plan["batched"] == 1 and bool(torch.isfinite(got).all())
    assert same_bits(ref, got), f"B={B}: logits differ at steps {sorted(set((ref != got).nonzero()[:, 0].tolist()))[:8]}"
    assert ref_streams == dict(qkv=0, out_proj=0, fc1=0, fc2=0), ref_streams
    assert streams == want_streams, (B, streams)


ALL = dict(qkv=1, out_proj=1, fc1=1, fc2=1)
NONE = dict(qkv=0, out_proj=0, fc1=0, fc2=0)


@pytest.mark.parametrize("B", [8, 17, 33])
def test_fp8_context_streams_bytes_in_the_batched_step(B):
    """ER_W8_BATCHED=1: every projection with a matrix-core form streams bytes (at B = 8 out_proj runs the eight-row VALU pass on fp16)."""
    assert_context_pair(model("fp16"), model("fp8", knob="1"), B, dict(ALL, out_proj=0) if B == 8 else ALL)


def test_fp8_context_on_row_major_inputs(monkeypatch):
    monkeypatch.setenv("ER_XT", "0")                                 # read by er_kv_reserve: ER_FORM_MFMA everywhere, fc2 with its finish kernel
    assert_context_pair(model("fp16"), model("fp8", knob="1"), 17, ALL)


def test_fp8_context_on_a_byte_cache():
    assert_context_pair(model("fp16", kv="fp8"), model("fp8", kv="fp8", knob="1"), 17, ALL)


def test_knob_0_keeps_the_fp16_copies():
    assert_context_pair(model("fp16"), model("fp8", knob="0"), 17, NONE)


@pytest.mark.parametrize("B", [8, 17])
def test_default_rule_streams_qkv_fc1_fc2(B):
    """ER_W8_BATCHED unset: what profiles/w8_batched_bench.json supports (csrc/er_weight_source.h w8_streams_batched) - out_proj keeps fp16."""
    assert_context_pair(model("fp16"), model("fp8"), B, dict(ALL, out_proj=0))


def test_row_forms_still_report_their_bytes():
    lmm = model("fp8", knob="0")
    dec = lmm.mesh_decoder
    dec.reserve(1, 64)
    dec.reserve(2, 64)
    assert dec.w8_streams() == ALL and dec.plan()["batched"] == 0     # w8_streams(proj, 2): all four row forms
    dec.reserve(4, 64)
    assert dec.w8_streams() == dict(ALL, out_proj=0)


# ---------------------------------------------------------------------------------------------- 5. memory
def test_byte_streamed_projections_get_no_fp16_tiled_copy(monkeypatch):
    """reserve(8, 64) on fresh contexts: fast mode makes the fp16 tiled copies of all four matrices (2 bytes per weight), the fp8 context
    under ER_W8_BATCHED=1 tiled bytes for qkv, fc1 and fc2 (1 byte per weight + 4 per padded row) and fp16 for out_proj only.  The byte
    context's drop must be smaller by those three matrices' bytes, up to the allocator's granule per allocation."""
    import test_gpu_lifetime as L
    from edgerunner_amd.models import LMM
    c = checkpoint()
    L.touch_stream_pool()
    monkeypatch.setenv("ER_W8_BATCHED", "1")
    drops = {}
    for prec, sd in (("fp16", c.deq), ("fp8", c.sd)):
        lmm = LMM(c.opt, DEV, precision=prec)
        lmm.load_state_dict(sd, strict=True)
        dec = lmm.mesh_decoder
        dec.reserve(1, 64)
        free0 = L.free_bytes()
        dec.reserve(8, 64)
        drops[prec] = free0 - L.free_bytes()
        if prec == "fp8":
            assert dec.w8_streams() == dict(ALL, out_proj=0)
        dec.close()
    layers = c.opt.num_layers
    streamed = layers * (3 * HID * HID + 2 * INTER * HID)            # weights of qkv, fc1, fc2
    scales = layers * 4 * (3 * HID + INTER + HID)
    saved = drops["fp16"] - drops["fp8"]
    print(f"free-memory drop of reserve(8, 64): fast mode {drops['fp16']}, fp8 with byte copies {drops['fp8']}; saved {saved}, the three matrices' bytes {streamed}")
    assert saved >= streamed - scales - 2 * 3 * layers * L.GRANULE, (drops, streamed)
