"""The fast-mode decode projections form by form, through ``er_k_gemv_form``: the entry runs the decode step's own launch table
(run_proj / launch_proj, csrc/er_decode_proj.h) and refuses what the step's own rule (proj_form_legal, csrc/er_decode_plan.h) does not
allow, so a test here runs the launch the step runs.  Against float64 torch on the device, and against each other where the kernels
promise equal bits.

Inputs as in test_gpu_kernels.py: seeded CPU generator, weights at scale 0.02, pre-LayerNorm rows randn * 2 + 0.3, relu(randn)
in front of fc2.  fp16 weights are ``w.half()`` and the reference multiplies the stored values ``w.half().double()``.  One set of
40 rows serves every batch size (a batch of B rows is the first B), so the float64 references are computed once per projection.

Bounds.  The row and VALU-batched forms run the fmaf chains of the fp32-weight tests: 2e-6 + 1e-5 |ref| at K = 1536, 4e-6 + 1e-5 |ref|
at K = 6144 (test_gpu_kernels.py).  The fp16 matrix-core forms consume hi + lo instead of x; their bound is the same figure plus
slack[b, n] = sum_k |w[n, k]| |x[b, k] - (hi + lo)[b, k]| with hi / lo from kernels.xt_pack_image applied to the float32 input on the
reference side (for a LayerNorm'd input: the float64 LayerNorm rounded to float32) - the exact representation error of the split,
independent of the code under test.  Every accuracy check prints its largest error and largest slack.

(projection, form) -> test.  One line per form proj_form returns and launch_proj launches; waves x rows and weight types are the ones
tests/host/decode_plan_check.cpp reaches (tests/test_decode_plan_cpu.py holds every reached tuple against this table).  fp16 lines are
tested here; fp32 lines name the test that runs the form, or say that none does.
  qkv  row     4x1,6x1,9x2  fp16  gemv_nw<PRO_LN | PRO_EMBED, EPI_QKV>          test_qkv_row_kernel, test_row_kernels_of_different_widths_give_equal_bits,
                                                                                test_qkv_epilogue_writes_exactly_one_key_row[row-*], test_embed_prologue_fused_row_kernel
  qkv  row     4x1,6x1      fp32  the same                                      test_gpu_parity.py: exact mode runs 6x1, test_decode_v2_and_4wave_qkv_small 4x1
  qkv  row     9x2          fp32  the same                                      no test (ER_NW_QKV=9 in exact mode)
  qkv  valu    -            fp16  prologue launch, VALU <1, 3, EPI_QKV>         test_batched_forms[qkv-valu], ...exactly_one_key_row[valu], test_valu_batch_rows_equal_single_row_kernel
  qkv  mfma    -            fp16  prologue launch, wide                         test_batched_forms[qkv-mfma], ...exactly_one_key_row[mfma]
  qkv  xt      -            fp16  prologue launch + image, wide XT              test_batched_forms[qkv-xt], ...exactly_one_key_row[xt], test_wide_form_on_tiled_input_equals_row_major,
                                                                                test_embed_prologue_prep_rows_and_its_image; 16 deferred slices: test_deferred_finish...[fc2-16-*]
  qkv  valu    -            fp32  as fp16                                       test_qkv_valu_fp32_weights
  qkv  mfma    -            fp32  as fp16                                       test_gpu_parity.py test_batched_kernels_teacher_forced_logits_24_layers[fp32]
  out  row     3x1          fp16  gemv_groups<1, 1, PRO_NONE, EPI_RESID, 3>     test_out_proj_three_wave_row_kernel
  out  row     3x1          fp32  the same                                      test_gpu_parity.py test_decode_v2_and_4wave_qkv_small[ER_DECODE_V=2] (version 3 fuses out_proj into the merge)
  out  rows8   3x1          fp16  gemv_outproj_rows8 NB = 5..8                  test_out_proj_rows8[*-False]
  out  rows8   3x1          fp32  the same                                      test_out_proj_rows8[*-True]
  out  valu    -            fp16  VALU <1, 1, EPI_RESID>                        test_batched_forms[out-valu]
  out  mfma    -            fp16  wide                                          test_batched_forms[out-mfma]
  out  defer   -            fp16  narrow, 4 slices, deferred                    test_batched_forms[out-defer], test_deferred_finish...[out-4-*]
  out  valu    -            fp32  as fp16                                       test_gpu_kernels.py test_gemv_batched_matrix_core_rows, test_gemv_batched_valu_rows_bit_identical_to_single
  out  mfma    -            fp32  as fp16                                       test_gpu_parity.py test_batched_kernels_teacher_forced_logits_24_layers[fp32]
  fc1  row     4x2,12x2     fp16  gemv_nw<PRO_LN, EPI_RELU>                     test_fc1_row_kernel, test_row_kernels_of_different_widths_give_equal_bits
  fc1  row     4x2          fp32  the same                                      test_gpu_kernels.py test_gemv_fc1_ln_relu
  fc1  row     12x2         fp32  the same                                      no test (ER_NW_FC1=12 in exact mode)
  fc1  valu    -            fp16  prologue launch, VALU <1, 3, EPI_RELU>        test_batched_forms[fc1-valu]
  fc1  mfma    -            fp16  prologue launch, wide                         test_batched_forms[fc1-mfma]
  fc1  xt      -            fp16  prologue launch + image, wide XT writing the  test_batched_forms[fc1-xt], test_wide_form_on_tiled_input_equals_row_major;
                                  next image (DPP quad permute)                 4 deferred slices: test_deferred_finish...[out-4-*]
  fc1  valu    -            fp32  as fp16                                       test_gpu_kernels.py test_gemv_batched_valu_rows_bit_identical_to_single
  fc1  mfma    -            fp32  as fp16                                       test_gpu_kernels.py test_gemv_batched_matrix_core_rows
  fc2  row     4x2,4x4,4x6  fp16  gemv_groups<4, 2> / launch_gemv<4, 1, 4 | 6>  test_fc2_row_kernel, test_row_kernels_of_different_widths_give_equal_bits
  fc2  row     4x2          fp32  gemv_groups<4, 2, PRO_NONE, EPI_RESID>        test_gpu_kernels.py test_gemv_fc2_ksplit_resid
  fc2  valu    -            fp16  VALU <4, 1, EPI_RESID>                        test_batched_forms[fc2-valu]
  fc2  mfma    -            fp16  wide + splitk_finish S = 4                    test_batched_forms[fc2-mfma]
  fc2  narrow  -            fp16  narrow + splitk_finish S = 16                 test_batched_forms[fc2-narrow], test_deferred_finish...[fc2-16-*]
  fc2  defer   -            fp16  narrow, 16 slices, deferred                   test_batched_forms[fc2-defer], test_deferred_finish...[fc2-16-*]
  fc2  valu    -            fp32  as fp16                                       test_gpu_kernels.py test_gemv_batched_valu_rows_bit_identical_to_single
  fc2  mfma    -            fp32  as fp16                                       test_gpu_kernels.py test_gemv_batched_matrix_core_rows
  head row     4x1          fp16  gemv_groups<1, 1, PRO_LN, EPI_STORE>          test_lm_head_ragged_rows[1-row / 4-row]
  head row     4x1          fp32  the same                                      test_gpu_kernels.py test_gemv_head_ln_store_ragged_rows
  head valu    -            fp16  prologue launch, VALU <1, 1, EPI_STORE>       test_lm_head_ragged_rows[5-valu / 19-valu], test_batched_forms[head-valu]
  head valu    -            fp32  as fp16                                       test_gpu_kernels.py test_gemv_batched_matrix_core_rows
every batched form: test_batched_row_independent_of_neighbours, test_valu_batch_rows_equal_single_row_kernel.  The streaming attention
that writes out_proj's image (launch_kind_t case 1, attn_stream_kernel with out_xt): test_attn_stream_writes_tiled_image.
Not reachable through the entry because the decode step never launches them: splitk_finish_kernel<EPI_QKV> (the qkv matrix has one
K-range of 1536, so no split precedes its epilogue) and splitk_finish_kernel behind the narrow out_proj (always deferred).  The balanced
single-row attention + merged out_proj (launch_kind_t case 3, v3: no GEMV form) has its own entry and tests in test_gpu_kernels.py.

Largest error / largest slack seen on an MI355X (B = 40 unless noted; bounds 2e-6 resp. 4e-6 + 1e-5 |ref| + slack): row kernels 4.5e-7
(fc1), 5.6e-7 (fc2 rw = 6), rows8 5.5e-7 (fp32) / 4.3e-7 (fp16); VALU qkv 5.9e-7, fc1 6.1e-7, out 5.3e-7, fc2 7.0e-7, head 4.7e-7;
wide qkv 6.9e-7 / 6.5e-7 (tiled input: the same), fc1 7.5e-7 / 6.6e-7 (tiled 7.9e-7: the image holds hi + lo of the output), out
8.6e-7 / 6.5e-7, fc2 8.4e-7 / 1.26e-6; narrow out deferred 4.2e-7 / 6.5e-7, fc2 finished 9.0e-7, deferred 5.4e-7 / 1.26e-6.  No
form uses more than a fifth of its bound.

Mutations tried on a scratch copy (none committed), each passing the suite as it stood before this file: see the commit message."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HID, INTER, VOCAB, NPOS = 1536, 6144, 518, 64
HEADS, HD, LCAP = 16, 96, 64
NMAX = 40                                       # rows of the shared inputs
BATCHES = [5, 16, 17, 32, 33, 40]               # 16 -> 17 crosses NBH, 32 -> 33 opens a second group, 40 = a partial second group of 8
NAN32, NAN16 = 0x7FC00123, 0x7E01               # sentinels: quiet-NaN patterns no kernel produces


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def F():
    from edgerunner_amd import native
    return native


@functools.lru_cache(maxsize=None)
def data():
    d = SimpleNamespace()
    d.w = {"qkv": rnd(3 * HID, HID, seed=101, scale=0.02), "out": rnd(HID, HID, seed=102, scale=0.02),
           "fc1": rnd(INTER, HID, seed=103, scale=0.02), "fc2": rnd(HID, INTER, seed=104, scale=0.02),
           "head": rnd(VOCAB, HID, seed=105, scale=0.02)}              # 518 rows: ragged against every rows-per-workgroup
    d.wh = {k: v.half() for k, v in d.w.items()}
    d.bias = {"qkv": rnd(3 * HID, seed=106, scale=0.02), "out": rnd(HID, seed=107, scale=0.02), "fc1": rnd(INTER, seed=108, scale=0.02),
              "fc2": rnd(HID, seed=109, scale=0.02), "head": None}
    d.x = rnd(NMAX, HID, seed=110) * 2 + 0.3                           # pre-LayerNorm rows (qkv, fc1, lm_head)
    d.lw, d.lb = 1 + 0.1 * rnd(HID, seed=111), 0.05 * rnd(HID, seed=112)
    d.att = rnd(NMAX, HID, seed=113)                                   # out_proj input
    d.f = torch.relu(rnd(NMAX, INTER, seed=114))                       # fc2 input
    d.r = rnd(NMAX, HID, seed=115)                                     # residual rows
    d.embd, d.posemb = rnd(VOCAB, HID, seed=116), rnd(NPOS, HID, seed=117)
    g = torch.Generator().manual_seed(118)
    d.pos = [0, LCAP - 1, 5] + [p for p in torch.randperm(LCAP, generator=g).tolist() if p not in (0, LCAP - 1, 5)][:NMAX - 3]   # distinct
    d.tok = [0, VOCAB - 1, 7] + torch.randint(0, VOCAB, (NMAX - 3,), generator=g).tolist()
    d.xr = torch.nn.functional.layer_norm(d.x.double(), (HID,), d.lw.double(), d.lb.double(), 1e-5)
    d.emb = d.embd[d.tok] + d.posemb[d.pos]                            # one fp32 add per element: exact reference of PRO_EMBED
    return d


PROJ = {   # name -> (epilogue, K, absolute bound of test_gpu_kernels.py, has a LayerNorm prologue)
    "qkv": ("QKV", HID, 2e-6, True), "out": ("RESID", HID, 2e-6, False), "fc1": ("RELU", HID, 2e-6, True),
    "fc2": ("RESID", INTER, 4e-6, False), "head": ("STORE", HID, 2e-6, True)}


def proj_input64(name, pro="ln"):
    """What the projection multiplies, float64 [NMAX, K]."""
    d = data()
    if name == "out":
        return d.att.double()
    if name == "fc2":
        return d.f.double()
    return d.emb.double() if pro == "embed" else d.xr


@functools.lru_cache(maxsize=None)
def reference(name, w32=False, pro="ln"):
    """float64 [NMAX, N] of the projection over the stored weights (qkv: the columns are q | k | v)."""
    d = data()
    w = (d.w if w32 else d.wh)[name].double()
    y = proj_input64(name, pro) @ w.T
    if d.bias[name] is not None:
        y = y + d.bias[name].double()
    epi = PROJ[name][0]
    if epi == "RESID":
        y = y + d.r.double()
    return torch.relu(y) if epi == "RELU" else y


@functools.lru_cache(maxsize=None)
def slack(name, pro="ln"):
    """sum_k |w| |x - (hi + lo)| per output, from the reference side only (module docstring)."""
    from edgerunner_amd import kernels as K
    x32 = proj_input64(name, pro).float()
    hi, lo = K.xt_unpack_image(K.xt_pack_image(x32), NMAX)
    return data().wh[name].abs().double() @ (x32 - (hi.float() + lo.float())).abs().double().T


def check(got, ref, atol, what, slk=None, rtol=1e-5):
    err = (got.double() - ref).abs()
    tol = atol + rtol * ref.abs() + (0 if slk is None else slk)
    print(f"{what}: max err {float(err.max()):.3e} (largest err / bound {float((err / tol).max()):.3f})"
          + ("" if slk is None else f", max slack {float(slk.max()):.3e}"))
    bad = (err > tol) | torch.isnan(got.double())
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} beyond the bound, max abs err {float(err.max()):.3e}, " \
                          f"first bad index {bad.nonzero()[0].tolist()}"


def rows_of(t, rows):
    return t[list(rows)].contiguous()


def part_rows(part, B, S, N):
    """[B, S, N] of a deferred split-K block [groups, S * 32 * N]: group g holds [S][rows of the group][N] (k_gemv.h sk_part)."""
    out = []
    for g in range((B + 31) // 32):
        nbg = min(32, B - 32 * g)
        out.append(part[g, :S * nbg * N].view(S, nbg, N).permute(1, 0, 2))
    return torch.cat(out).contiguous()


def sentinel_caches(B, half):
    if half:
        kc = torch.full((B, HEADS, LCAP, HD), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    else:
        kc = torch.full((B, HEADS, LCAP, HD), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    q = torch.full((B, HID), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    return kc, kc.clone(), q


def cache_rows(c, pos):
    return torch.stack([c[b, :, p, :].reshape(HID) for b, p in enumerate(pos)])


FORMS = {"row": "ER_FORM_ROW", "rows8": "ER_FORM_ROWS8", "valu": "ER_FORM_VALU", "mfma": "ER_FORM_MFMA", "xt": "ER_FORM_MFMA_XT",
         "narrow": "ER_FORM_NARROW", "defer": "ER_FORM_NARROW_DEFER"}


@functools.lru_cache(maxsize=None)
def run(name, form, B, rows=None, nw=4, rw=1, kv_half=False, w32=False, pro="ln"):
    """One launch of projection `name` in `form` on rows `rows` (default: the first B) of the shared inputs.  Returns a namespace:
    val = the output rows [B, N] (fp32; the tiled fc1: hi + lo in float64; deferred: the partials finished in float64),
    bits = what a bit comparison looks at, plus the raw pieces (xnorm, q / kc / vc / pos, image, part)."""
    from edgerunner_amd import kernels as K
    nat, d = F(), data()
    rows = tuple(range(B)) if rows is None else rows
    assert len(rows) == B
    epi, kk, _, has_ln = PROJ[name]
    w = (d.w if w32 else d.wh)[name]
    kw = dict(bias=d.bias[name], nw=nw, rw=rw)
    tiled_in = form in ("narrow", "defer")
    if has_ln and pro == "embed":
        kw["embed"] = (d.embd, d.posemb, [d.tok[i] for i in rows], [d.pos[i] for i in rows])
    elif has_ln:
        kw.update(x=rows_of(d.x, rows), ln=(d.lw, d.lb))
    else:
        x = rows_of(d.att if name == "out" else d.f, rows)
        kw.update(x=K.xt_pack_image(x) if tiled_in else x, resid=rows_of(d.r, rows))
    r = SimpleNamespace(pos=[d.pos[i] for i in rows])
    if epi == "QKV":
        r.kc, r.vc, q = sentinel_caches(B, kv_half)
        kw["qkv"] = (r.kc, r.vc, r.pos, q)
    o = K.gemv_form(getattr(nat, FORMS[form]), getattr(nat, "ER_EPI_" + epi), w, B, return_xnorm=has_ln, prep_xt=(form == "xt"), **kw)
    r.xnorm, r.image = o.get("xnorm"), o.get("prep_xt")
    if epi == "QKV":
        r.q = o["q"]
        r.val = r.bits = torch.cat((r.q, cache_rows(r.kc, r.pos).float(), cache_rows(r.vc, r.pos).float()), dim=1)
    elif form == "xt":        # fc1: the output exists as the next projection's image only
        r.xt_out = o["xt_out"]
        hi, lo = K.xt_unpack_image(r.xt_out, B)
        r.bits = torch.cat((hi, lo), dim=1)
        r.val = hi.double() + lo.double()
    elif form == "defer":
        S, N = kk // 384, w.shape[0]
        r.part = o["part"]
        r.bits = part_rows(r.part, B, S, N)
        r.val = r.bits.double().sum(dim=1) + d.bias[name].double() + rows_of(d.r, rows).double()
    else:
        r.val = r.bits = o["y"]
    return r


def accuracy(name, form, B, **kw):
    r = run(name, form, B, **kw)
    d = data()
    pro = kw.get("pro", "ln")
    slk = slack(name, pro).T[:B] if form in ("mfma", "xt", "narrow", "defer") and not kw.get("w32") else None
    what = f"{name} {form} B={B} " + " ".join(f"{k}={v}" for k, v in kw.items())
    if r.xnorm is not None:
        if pro == "embed":
            assert torch.equal(r.xnorm, d.emb[:B]), f"{what}: embedding rows"
        else:
            check(r.xnorm, d.xr[:B], 2e-6, what + " LayerNorm rows", rtol=2e-6)       # test_gpu_kernels.py's bound for the prologue
    check(r.val, reference(name, bool(kw.get("w32")), pro)[:B], PROJ[name][2], what, slk)
    return r


# ------------------------------------------------------------------ A. accuracy against float64, fp16 weights, every form
@pytest.mark.parametrize("nw", [4, 12])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_fc1_row_kernel(B, nw):
    accuracy("fc1", "row", B, nw=nw, rw=2)


@pytest.mark.parametrize("pro", ["ln", "embed"])
@pytest.mark.parametrize("nw", [4, 6, 9])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_qkv_row_kernel(B, nw, pro):
    accuracy("qkv", "row", B, nw=nw, rw=2 if nw == 9 else 1, pro=pro)


@pytest.mark.parametrize("B", [1, 3])
def test_out_proj_three_wave_row_kernel(B):
    accuracy("out", "row", B, nw=3, rw=1)


@pytest.mark.parametrize("w32", [True, False])
@pytest.mark.parametrize("B", [5, 6, 7, 8])
def test_out_proj_rows8(B, w32):
    accuracy("out", "rows8", B, w32=w32)


@pytest.mark.parametrize("B,rw", [(1, 2), (1, 4), (1, 6), (2, 2), (4, 2)])
def test_fc2_row_kernel(B, rw):
    accuracy("fc2", "row", B, nw=4, rw=rw)


@pytest.mark.parametrize("B,form", [(1, "row"), (4, "row"), (5, "valu"), (19, "valu")])
def test_lm_head_ragged_rows(B, form):
    accuracy("head", form, B)


BATCHED_FORMS = [("qkv", "valu"), ("qkv", "mfma"), ("qkv", "xt"), ("fc1", "valu"), ("fc1", "mfma"), ("fc1", "xt"),
                 ("out", "valu"), ("out", "mfma"), ("out", "defer"),                      # out_proj: narrow, 4 slices, always deferred
                 ("fc2", "valu"), ("fc2", "mfma"), ("fc2", "narrow"), ("fc2", "defer"),   # fc2: narrow, 16 slices
                 ("head", "valu")]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name,form", BATCHED_FORMS)
def test_batched_forms(name, form, B):
    r = accuracy(name, form, B)
    if form == "xt":          # rows the batch does not have stay zero in both images
        for img in (r.image, getattr(r, "xt_out", None)):
            if img is not None:
                from edgerunner_amd import kernels as K
                hi, lo = K.xt_unpack_image(img)
                assert not hi[B:].any() and not lo[B:].any(), "image rows >= B written"


@pytest.mark.parametrize("B", [5, 19])
def test_qkv_valu_fp32_weights(B):
    """The one fp32-weight form no other test launches: er_k_gemv has no QKV epilogue, and no whole-step test reserves with ER_BATCHED_VALU=1."""
    accuracy("qkv", "valu", B, w32=True)


# ------------------------------------------------------------------ B. stated bit identities
@pytest.mark.parametrize("B", [5, 17, 40])
def test_wide_form_on_tiled_input_equals_row_major(B):
    """k_gemv_mfma.h: XT reads the same values and issues the same MFMA sequence.  qkv: q and both (fp16) caches, whole buffers; fc1: the
    tiled output image decodes to xt_pack of the row-major output; the LayerNorm image decodes to xt_pack of the LayerNorm rows."""
    from edgerunner_amd import kernels as K
    a, b = run("qkv", "xt", B, kv_half=True), run("qkv", "mfma", B, kv_half=True)
    for got, want, what in ((a.q, b.q, "q"), (a.kc, b.kc, "k cache"), (a.vc, b.vc, "v cache")):
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"qkv {what}: tiled and row-major inputs differ"
    assert torch.equal(a.image, K.xt_pack_image(a.xnorm)), "LayerNorm image != xt_pack(LayerNorm rows)"
    a, b = run("fc1", "xt", B), run("fc1", "mfma", B)
    assert torch.equal(a.xt_out, K.xt_pack_image(b.val)), "fc1 image != xt_pack(row-major fc1 output)"


@pytest.mark.parametrize("B", [5, 19])
def test_valu_batch_rows_equal_single_row_kernel(B):
    """fp16 weights: a row of a VALU batch has the bits of the same row through the B = 1 kernel (same fmaf chains, same tree)."""
    single = {"qkv": dict(nw=4, rw=1), "fc1": dict(nw=4, rw=2), "out": dict(nw=3, rw=1), "fc2": dict(nw=4, rw=2), "head": dict(nw=4, rw=1)}
    for name, kw in single.items():
        full = run(name, "valu", B)
        for i in range(B):
            one = run(name, "row", 1, rows=(i,), **kw)
            assert torch.equal(one.bits[0], full.bits[i]), f"{name} row {i}"
            if full.xnorm is not None:
                assert torch.equal(one.xnorm[0], full.xnorm[i]), f"{name} LayerNorm row {i}"


@pytest.mark.parametrize("B", [17, 40])
@pytest.mark.parametrize("name,form", BATCHED_FORMS)
def test_batched_row_independent_of_neighbours(name, form, B):
    """Same bits whether a row runs in a 5-row or a B-row batch, first or second half, first or second group (B = 40: row 39)."""
    idx = (B - 1, 0, B // 2, 1, 2)
    full, sub = run(name, form, B), run(name, form, 5, rows=idx)
    assert torch.equal(sub.bits, full.bits[list(idx)]), f"{name} {form}: a row's bits depend on its batch neighbours"


@pytest.mark.parametrize("B", [5, 33, 40])
@pytest.mark.parametrize("name,S", [("out", 4), ("fc2", 16)])
def test_deferred_finish_equals_finish_then_layernorm(name, S, B):
    """prep_rows reading sk_part == ((p_0 + .. + p_{S-1}) + bias) + resid, then prep_rows<PRO_LN> (k_gemv.h: same order of adds).
    The finished rows are restated here as fp32 torch adds in slice order (adds only: nothing to contract); at 16 slices they must
    also be the bits splitk_finish_kernel<EPI_RESID> leaves behind the narrow fc2.  (The decode step never finishes the narrow
    out_proj with the finish kernel, so at 4 slices the restatement is the only finish.)"""
    from edgerunner_amd import kernels as K
    nat, d = F(), data()
    dfr = run(name, "defer", B)
    p = dfr.bits                                                  # [B, S, 1536]
    y = p[:, 0] + 0.0
    for s in range(1, S):
        y = y + p[:, s]
    y = (y + d.bias[name]) + d.r[:B]
    if S == 16:
        assert torch.equal(run(name, "narrow", B).val, y), "splitk_finish_kernel S=16"
    ln = (d.lw, d.lb)
    want = K.gemv_form(nat.ER_FORM_PREP, 0, None, B, x=y.contiguous(), ln=ln, n=HID, k=HID, w_half=True, prep_xt=True)
    got = K.gemv_form(nat.ER_FORM_PREP, 0, None, B, ln=ln, sk=(dfr.part, d.bias[name], d.r[:B].contiguous(), S), n=HID, k=HID, w_half=True,
                      prep_xt=True)
    assert torch.equal(got["xnorm"], want["xnorm"]), f"deferred finish, {S} slices"
    assert torch.equal(got["prep_xt"], K.xt_pack_image(got["xnorm"])) and torch.equal(want["prep_xt"], got["prep_xt"])
    check(got["xnorm"], torch.nn.functional.layer_norm(y.double(), (HID,), d.lw.double(), d.lb.double(), 1e-5), 2e-6, "LayerNorm of the finish", rtol=2e-6)


@pytest.mark.parametrize("B", [1, 4])
def test_row_kernels_of_different_widths_give_equal_bits(B):
    """Each wave owns whole rows and the prologue always runs on four waves' mapping: the workgroup width cannot change a bit."""
    base = run("qkv", "row", B, nw=4, rw=1, kv_half=True)
    for nw, rw in ((6, 1), (9, 2)):
        o = run("qkv", "row", B, nw=nw, rw=rw, kv_half=True)
        assert torch.equal(o.bits, base.bits) and torch.equal(o.xnorm, base.xnorm), f"qkv nw={nw}"
    assert torch.equal(run("fc1", "row", B, nw=12, rw=2).bits, run("fc1", "row", B, nw=4, rw=2).bits), "fc1 nw=12"
    if B == 1:
        for rw in (4, 6):
            assert torch.equal(run("fc2", "row", 1, nw=4, rw=rw).bits, run("fc2", "row", 1, nw=4, rw=2).bits), f"fc2 rw={rw}"


# ------------------------------------------------------------------ C. the QKV epilogue writes exactly one key row
@pytest.mark.parametrize("form,B,kw", [("row", 3, dict(nw=4, rw=1)), ("row", 3, dict(nw=6, rw=1)), ("row", 3, dict(nw=9, rw=2)),
                                       ("valu", 5, {}), ("mfma", 19, {}), ("xt", 40, {})])
def test_qkv_epilogue_writes_exactly_one_key_row(form, B, kw):
    ref, d = reference("qkv")[:B], data()
    slk = slack("qkv").T[:B] if form in ("mfma", "xt") else None
    r32, r16 = run("qkv", form, B, kv_half=False, **kw), run("qkv", form, B, kv_half=True, **kw)
    pos = d.pos[:B]
    assert pos[0] == 0 and pos[1] == LCAP - 1 and len(set(pos)) == B
    outside = torch.ones((B, HEADS, LCAP, HD), dtype=torch.bool, device=DEV)
    for b, p in enumerate(pos):
        outside[b, :, p, :] = False
    for r, ity, sent in ((r32, torch.int32, NAN32), (r16, torch.int16, NAN16)):
        for c, what in ((r.kc, "k"), (r.vc, "v")):
            ci = c.view(ity)
            assert bool((ci[outside] == sent).all()), f"{what} cache ({ity}): an element outside [b, :, pos[b], :] was written"
            assert not bool((ci[~outside] == sent).any()), f"{what} cache ({ity}): an element of the new key row was not written"
        assert not bool((r.q.view(torch.int32) == NAN32).any()), "q: element not written"
    check(r32.q, ref[:, :HID], 2e-6, f"q {form}", None if slk is None else slk[:, :HID])
    check(cache_rows(r32.kc, pos), ref[:, HID:2 * HID], 2e-6, f"K row {form}", None if slk is None else slk[:, HID:2 * HID])
    check(cache_rows(r32.vc, pos), ref[:, 2 * HID:], 2e-6, f"V row {form}", None if slk is None else slk[:, 2 * HID:])
    assert torch.equal(r16.q, r32.q)
    for c16, c32, what in ((r16.kc, r32.kc, "k"), (r16.vc, r32.vc, "v")):      # round to nearest even of the same fp32 value
        assert torch.equal(cache_rows(c16, pos), cache_rows(c32, pos).half()), f"{what}: fp16 cache != half(fp32 cache)"


# ------------------------------------------------------------------ D. the embed prologue
def test_embed_prologue_fused_row_kernel():
    """tokens {0, V-1, 7} at positions {0, P-1, 5}: hout = embd[tok] + posemb[pos], one fp32 add."""
    d = data()
    assert d.tok[:3] == [0, VOCAB - 1, 7] and d.pos[:3] == [0, NPOS - 1, 5]
    rows = (0, 1, 2)
    for nw, rw in ((4, 1), (6, 1), (9, 2)):
        r = run("qkv", "row", 3, rows=rows, nw=nw, rw=rw, pro="embed")
        assert torch.equal(r.xnorm, d.embd[[0, VOCAB - 1, 7]] + d.posemb[r.pos]), f"nw={nw}"


@pytest.mark.parametrize("B", [5, 33])
def test_embed_prologue_prep_rows_and_its_image(B):
    from edgerunner_amd import kernels as K
    nat, d = F(), data()
    tok, pos = d.tok[:B], d.pos[:B]
    o = K.gemv_form(nat.ER_FORM_PREP, 0, None, B, embed=(d.embd, d.posemb, tok, pos), n=HID, k=HID, w_half=True, prep_xt=True)
    assert torch.equal(o["xnorm"], d.embd[tok] + d.posemb[pos])
    assert torch.equal(o["prep_xt"], K.xt_pack_image(o["xnorm"])), "image != xt_pack(hout), or a row >= B was written"
    hi, lo = K.xt_unpack_image(o["prep_xt"])
    assert not hi[B:].any() and not lo[B:].any()
    accuracy("qkv", "xt", B, pro="embed")      # the same launch in front of the projection (qkv, layer 0)
    # the LayerNorm prologue writes its image the same way
    o = K.gemv_form(nat.ER_FORM_PREP, 0, None, B, x=d.x[:B].contiguous(), ln=(d.lw, d.lb), n=HID, k=HID, w_half=True, prep_xt=True)
    assert torch.equal(o["prep_xt"], K.xt_pack_image(o["xnorm"]))
    check(o["xnorm"], d.xr[:B], 2e-6, "prep_rows LayerNorm", rtol=2e-6)


# ------------------------------------------------------------------ E. attn_stream_kernel out_xt
@pytest.mark.parametrize("lens", [[129, 1, 2051, 64, 700], ([129, 1, 64, 700, 33, 257, 2] * 5)[:33]])
@pytest.mark.parametrize("half", [False, True])
def test_attn_stream_writes_tiled_image(half, lens):
    from edgerunner_amd import kernels as K
    B = len(lens)
    Lcap = (max(lens) + 31) // 32 * 32
    q = rnd(B, HID, seed=70)
    kc, vc = rnd(B, HEADS, Lcap, HD, seed=71), rnd(B, HEADS, Lcap, HD, seed=72)
    if half:
        kc, vc = kc.half(), vc.half()
    for b, n in enumerate(lens):
        kc[b, :, n:] = float("nan")
        vc[b, :, n:] = float("nan")
    img = torch.full(((B + 31) // 32, HID // 4, 32, 8), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    out = K.attn_stream_xt(q, kc, vc, lens, img)
    for b, n in enumerate(lens):
        w = torch.softmax(q[b].view(HEADS, 1, HD).double() @ kc[b, :, :n].double().transpose(1, 2) / math.sqrt(HD), dim=-1)
        check(out[b], (w @ vc[b, :, :n].double()).reshape(HID), 2e-6, f"streaming attn row {b} len {n}")
    want = K.xt_pack_image(out).view(torch.int16)
    hi, lo = K.xt_unpack_image(want.view(torch.float16))
    rows = torch.arange(hi.shape[0], device=DEV) < B
    wh, wl = hi.view(torch.int16), lo.view(torch.int16)
    wh[~rows], wl[~rows] = NAN16, NAN16                           # rows the batch does not have: untouched
    gh, gl = K.xt_unpack_image(img)
    assert torch.equal(gh.view(torch.int16), wh) and torch.equal(gl.view(torch.int16), wl), "image != xt_pack(out), or a row >= B was written"


# ------------------------------------------------------------------ F. what the decode step never launches is refused
def test_unsupported_combinations_are_refused_before_any_launch():
    from edgerunner_amd import kernels as K
    nat, d = F(), data()
    kc, vc, q = sentinel_caches(3, True)
    bad = [
        ("narrow form over fp32 weights", lambda: K.gemv_form(nat.ER_FORM_NARROW, nat.ER_EPI_RESID, d.w["fc2"], 5, x=K.xt_pack_image(d.f[:5]), bias=d.bias["fc2"], resid=d.r[:5].contiguous())),
        ("narrow out_proj through the finish kernel", lambda: K.gemv_form(nat.ER_FORM_NARROW, nat.ER_EPI_RESID, d.wh["out"], 40, x=K.xt_pack_image(d.att), bias=d.bias["out"], resid=d.r)),
        ("12-wave qkv", lambda: K.gemv_form(nat.ER_FORM_ROW, nat.ER_EPI_QKV, d.wh["qkv"], 3, x=d.x[:3].contiguous(), ln=(d.lw, d.lb), bias=d.bias["qkv"], qkv=(kc, vc, d.pos[:3], q), nw=12, rw=2)),
        ("six-row fc2 workgroups at two batch rows", lambda: K.gemv_form(nat.ER_FORM_ROW, nat.ER_EPI_RESID, d.wh["fc2"], 2, x=d.f[:2].contiguous(), bias=d.bias["fc2"], resid=d.r[:2].contiguous(), nw=4, rw=6)),
        ("matrix-core lm_head", lambda: K.gemv_form(nat.ER_FORM_MFMA, nat.ER_EPI_STORE, d.wh["head"], 5, x=d.x[:5].contiguous(), ln=(d.lw, d.lb))),
    ]
    for what, call in bad:
        with pytest.raises(nat.NativeError, match=r"er_k_gemv_form failed \(-5\)"):
            call()
    torch.cuda.synchronize()
    for c in (kc, vc):
        assert bool((c.view(torch.int16) == NAN16).all()), "a refused call wrote the cache"
    assert bool((q.view(torch.int32) == NAN32).all()), "a refused call wrote q"
