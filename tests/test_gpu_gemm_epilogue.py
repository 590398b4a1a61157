"""The plain GEMM epilogue with its adaLN gate rows and its shared residual table, form by form, through ``er_k_gemm_epi`` (the entry
fills GemmArgs and calls the family's own launcher, so a test here runs the kernel the product runs):

    C[m][n] = resid[m % resid_mod if resid_mod else m][n] + gate[m // gate_rows][n] * relu?((A . W^T)[m][n] (/ div) + bias[n]),  c16 = fp16(C)

against float64 torch, and form against form where the kernels promise equal bits.

Forms (17) - every case runs on every form:
  f32r-t1 / t2 / t3     gemm_f32_mfma_kernel   (ER_GEMM_F32_DMA=0, ER_GEMM_TILE=1 / 2 / 3)       scalar epilogue (gemm_epilogue), 32-row blocks
  f32d-t1 / t2 / t3     gemm_f32d_mfma_kernel  (ER_GEMM_F32_DMA=1, ER_GEMM_TILE)                  the same epilogue
  f16-t1 / t2 / t3      gemm_f16_mfma_kernel   (plain form, ER_GEMM_TILE)                         the same epilogue
  f16s-t1 / t2 / t3     gemm_f16_mfma_kernel   (split form, ER_GEMM_TILE)                         the same epilogue
  hh-t1, hh-t4          gemm_hh_mfma_kernel<2, 2> / gemm_hh256_kernel (ER_GEMM_STREAM=0)          row-wise epilogue (hh_epi_rows), 64-row waves:
                                                                                                  gate pair, residual loaded in the pass loop
  hh-t2, hh-t3          gemm_hh_mfma_kernel<1, 2> / <1, 1>                                        hh_epi_rows, 32-row waves: gate pair, the
                                                                                                  residuals of all eight passes requested first
  hh-stream             gemm_hh_stream_kernel  (ER_GEMM_STREAM=2, force_tile 0)                   hh_epi_rows in two parts on 32-row halves, operands
                                                                                                  from gs_load_pre when the wave's 64 columns are whole

Cases (K = 64 or 128; "fast" = RowBatch's compare form, period >= rows of the span; every gated case but 5 also adds a full-size residual):
  case               M    N    gate_rows      gemm_epilogue forms        hh-t1 / t4 (64 rows)       hh-t2 / t3 / stream (32 rows)
  1  boundary        200  256  100            fast, boundary in 96..127  fast, boundary in 64..127  fast; M ragged against 64 / 128 / 256
  2  gr40            200  128  40             fast                       division per row           fast (gate pair)
  3  gr24            192  128  24             division                   division                   division
  3  gr20            192  128  20             division; two boundaries inside the aligned 32-row blocks at 32, 64, 128, 160 (40 and 60, ..) - with
                                              24 rows per batch no aligned block holds two (lcm 96), so a compare form wrongly taken from
                                              16 rows on would pass case gr24; added after a mutation of the threshold passed every other case
  4  per-row         70   128  1              division                   division                   division
  5  one batch       200  128  M              fast, q0 = 0 only          gb0 == gb1                 gb0 == gb1; no residual
  6  past-M-130      130  256  65             rows skipped               wave 192 wholly past M     waves 160 (t2, t3), 160 / 192 / 224 (stream) past M
  6  past-M-100      100  256  50             rows skipped               t4: waves 128, 192 past M  (t1, t2, t3, stream: no wave past M at this shape)
  7  tail-130/-67    200  130 / 67  100       columns >= N skipped       gate_bstride = N rounded up to 4: lanes with 4 whole columns vector, the tail lane
                                                                         scalar; a wave / workgroup column block wholly past N; stream: no pre-fetch there
  8  scalar-130/-67  200  130 / 67  100       odd ldc / ldr              gate_bstride = N, odd ldc / ldr: the scalar path on every lane
  9  mod-33/64/100/M 200  128  no gate        resid_mod: 33 fast         33: division               33 fast; the pre-fetched residual rows (t2, t3,
                                              (64, 100, M fast)          (64, 100, M fast)          stream) go through inner(min(gm, M - 1))
  9  mod-20          200  128  no gate        resid_mod 20: division everywhere, two boundaries per 32-row block (as gr20)
  10 order           200  128  100            resid_mod 100, relu, and div = 8 for the fp32 forms: / div, + bias, relu, * gate, + resid in that order
Case 6: a wave wholly past M with M a whole number of batches computes gate row number-of-batches unless its row is clamped; every
hh form has such a wave in one of the two shapes (table).  The gemm_epilogue forms form no address before the row check.

Inputs.  Gate and residual tables are VIEWS into larger allocations whose other rows are NaN: the gate allocation holds
ceil(roundup(M, 256) / gate_rows) + 1 rows, the residual allocation roundup(M, 256) rows behind the real ones and 256 in front (an
unclamped wave row turned into row -1 of a shared table in the compare form: M = 200, resid_mod = 100, 32-row wave at 224), so every
read stays inside an allocation whatever the state of the clamps, and a spare row that is USED shows up as NaN.  C and c16 are views
into allocations with ldc > N, a guard row in front and two behind, filled with a sentinel bit pattern.

Checks per case and form.
  exact     A, W integers in [-2, 2], bias multiples of 1/8 in [-4, 4], gate[b][n] = 1 + (7 b + 3 n) % 61, resid[r][n] = (131 r + 17 n) % 1021,
            div in {0, 8}: |A.W^T| <= 4 K <= 512, so every intermediate is a multiple of 1/8 below 2^15 - exact in fp16 operands, in the fp32
            accumulator and through any fma contraction: C must EQUAL the float64 reference, c16 its .half().  Both tables are injective in
            (row, column) over the ranges used, so a wrong row or column index changes the value.
            (test_exact_references_are_fp32_values holds the representability on the CPU.)
  random    randn A (fp16-rounded for f16 / hh; the split family keeps fp32 A), W = randn * 0.05 (fp16 for the fp16 families), gate uniform in
            [0.5, 2], randn bias and residual; against float64 with twice the absolute term of test_gpu_kernels.py (the gate is at most 2):
            2 * (2e-6 + 1e-7 K) for fp32 and split-fp16, 2 * (1e-5 + 2e-7 K) for fp16 and LDS-DMA fp16; rtol 1e-5; c16 == C.half().
  bits      on the random operands: the six fp32 forms agree bit for bit, the three fp16 forms, the three split forms, and the five
            LDS-DMA forms (streamed == ER_GEMM_STREAM=0 included, C and c16).
  sentinels every element of the C and c16 allocations outside [0, M) x [0, N) keeps its bits; no NaN inside.
  refusals  test_refusals: ER_ERR_INVALID before any launch, output untouched.

Largest random-operand error seen on an MI355X (printed by test_random): fp32 1.8e-6 (0.05 of its bound), split fp16 1.1e-6 (0.02),
fp16 and LDS-DMA fp16 1.1e-6 (0.01); the bounds are test_gpu_kernels.py's with the absolute term doubled, none widened.  In-bounds mutations tried on scratch builds, each failing
exactly the forms that run the mutated line: the neighbour row's gate in the 64-row pass loop (hh-t1, hh-t4), gb1 = gb0 and
min(gm, resid_mod - 1) in gs_load_pre (hh-stream), the last pre-fetched residual row off by one (hh-t2, hh-t3), bias before / div
(fp32 forms, case 10), the compare form taken from span / 2 rows on (hh-t1 / t4 on gr40 and mod-33; every 32-row form on gr20, mod-20)."""
import contextlib
import functools
import os
from types import SimpleNamespace

import pytest
import torch

DEV = "cuda:0"
NAN32, NAN16 = 0x7FC00123, 0x7E01               # sentinels: quiet-NaN patterns no kernel produces
gpu = pytest.mark.gpu

# name -> (family, environment, force_tile)
FORMS = {}
for t in (1, 2, 3):
    FORMS[f"f32r-t{t}"] = ("F32", {"ER_GEMM_F32_DMA": "0", "ER_GEMM_TILE": str(t)}, 0)
    FORMS[f"f32d-t{t}"] = ("F32", {"ER_GEMM_F32_DMA": "1", "ER_GEMM_TILE": str(t)}, 0)
    FORMS[f"f16-t{t}"] = ("F16", {"ER_GEMM_TILE": str(t)}, 0)
    FORMS[f"f16s-t{t}"] = ("F16S", {"ER_GEMM_TILE": str(t)}, 0)
for t in (1, 2, 3, 4):
    FORMS[f"hh-t{t}"] = ("HH", {"ER_GEMM_STREAM": "0"}, t)
FORMS["hh-stream"] = ("HH", {"ER_GEMM_STREAM": "2"}, 0)
BIT_GROUPS = {"fp32": [f for f in FORMS if f.startswith("f32")], "fp16": [f for f in FORMS if f.startswith("f16-")],
              "split fp16": [f for f in FORMS if f.startswith("f16s")], "LDS-DMA fp16": [f for f in FORMS if f.startswith("hh")]}


def case(M, N, K, gate_rows=0, resid=True, resid_mod=0, pad4=True, odd_ld=False, relu=False, div32=0.0):
    return SimpleNamespace(M=M, N=N, K=K, gate_rows=gate_rows, resid=resid, resid_mod=resid_mod, pad4=pad4, odd_ld=odd_ld, relu=relu,
                           div32=div32)


CASES = {
    "1-boundary": case(200, 256, 64, 100),
    "2-gr40": case(200, 128, 128, 40),
    "3-gr24": case(192, 128, 64, 24),
    "3-gr20": case(192, 128, 64, 20),
    "4-per-row": case(70, 128, 64, 1),
    "5-one-batch": case(200, 128, 64, 200, resid=False),
    "6-past-M-130": case(130, 256, 64, 65),
    "6-past-M-100": case(100, 256, 128, 50),
    "7-tail-130": case(200, 130, 64, 100),
    "7-tail-67": case(200, 67, 128, 100),
    "8-scalar-130": case(200, 130, 64, 100, pad4=False, odd_ld=True),
    "8-scalar-67": case(200, 67, 64, 100, pad4=False, odd_ld=True),
    "9-mod-20": case(200, 128, 64, resid_mod=20),
    "9-mod-33": case(200, 128, 64, resid_mod=33),
    "9-mod-64": case(200, 128, 128, resid_mod=64),
    "9-mod-100": case(200, 128, 64, resid_mod=100),
    "9-mod-M": case(200, 128, 64, resid_mod=200),
    "10-order": case(200, 128, 128, 100, resid_mod=100, relu=True, div32=8.0),
}


def up(x, m):
    return (x + m - 1) // m * m


@functools.lru_cache(maxsize=None)
def operands(cname, kind):
    """CPU operands of a case: a, w, bias fp32; gate [batches, N] and resid [rows, N] (None where the case has none)."""
    c = CASES[cname]
    g = torch.Generator().manual_seed(1000 + 17 * list(CASES).index(cname))
    o = SimpleNamespace()
    nb = -(-c.M // c.gate_rows) if c.gate_rows else 0
    rrows = c.resid_mod if c.resid_mod else c.M
    n = torch.arange(c.N)
    if kind == "exact":
        o.a = torch.randint(-2, 3, (c.M, c.K), generator=g).float()
        o.w = torch.randint(-2, 3, (c.N, c.K), generator=g).float()
        o.bias = torch.randint(-32, 33, (c.N,), generator=g).float() / 8
        o.gate = (1 + (7 * torch.arange(nb)[:, None] + 3 * n[None, :]) % 61).float() if nb else None
        o.resid = ((131 * torch.arange(rrows)[:, None] + 17 * n[None, :]) % 1021).float() if c.resid else None
    else:
        o.a = torch.randn(c.M, c.K, generator=g)
        o.w = torch.randn(c.N, c.K, generator=g) * 0.05
        o.bias = torch.randn(c.N, generator=g)
        o.gate = (0.5 + 1.5 * torch.rand(nb, c.N, generator=g)) if nb else None
        o.resid = torch.randn(rrows, c.N, generator=g) if c.resid else None
    return o


def family_operands(cname, kind, fam):
    """(a, w) as the family consumes them, fp32 values: fp16-rounded where the kernel rounds."""
    o = operands(cname, kind)
    a = o.a.half().float() if fam in ("F16", "HH") else o.a
    w = o.w if fam == "F32" else o.w.half().float()
    return a, w


def reference(cname, kind, fam, dev="cpu"):
    """float64 reference of the case for a family, on `dev`."""
    c, o = CASES[cname], operands(cname, kind)
    a, w = family_operands(cname, kind, fam)
    p = a.to(dev).double() @ w.to(dev).double().T
    if fam == "F32" and c.div32:
        p = p / c.div32
    p = p + o.bias.to(dev).double()
    if c.relu:
        p = torch.relu(p)
    m = torch.arange(c.M, device=dev)
    if c.gate_rows:
        p = p * o.gate.to(dev).double()[m // c.gate_rows]
    if c.resid:
        p = p + o.resid.to(dev).double()[m % c.resid_mod if c.resid_mod else m]
    return p


@functools.lru_cache(maxsize=None)
def reference_dev(cname, kind, fam):
    return reference(cname, kind, fam, DEV)


def test_exact_references_are_fp32_values():
    """The zero-tolerance check is legitimate only if the float64 reference of every exact case is an fp32 number (and the operands fp16
    numbers): held here, on the CPU."""
    for cname in CASES:
        o = operands(cname, "exact")
        assert torch.equal(o.a.half().float(), o.a) and torch.equal(o.w.half().float(), o.w)
        for fam in ("F32", "F16", "F16S", "HH"):
            ref = reference(cname, "exact", fam)
            assert torch.equal(ref.float().double(), ref), (cname, fam)
            assert float(ref.abs().max()) * 8 < 2 ** 24 and torch.equal((ref * 8).round(), ref * 8), (cname, fam)      # multiples of 1/8 below 2^21


def test_exact_tables_are_injective():
    """gate[b][n] = 1 + (7 b + 3 n) % 61 and resid[r][n] = (131 r + 17 n) % 1021: a neighbouring row or a neighbouring column gives another
    value everywhere (what makes a wrong index visible), and no two of the batches / rows a case uses share a value in a column."""
    for cname, c in CASES.items():
        o = operands(cname, "exact")
        for t in (o.gate, o.resid):
            if t is None:
                continue
            if t.shape[0] > 1:
                assert (t[1:] != t[:-1]).all(), cname
            assert (t[:, 1:] != t[:, :-1]).all(), cname
            if t.shape[0] <= (61 if t is o.gate else 1021):
                assert all(len(set(col.tolist())) == t.shape[0] for col in t.T[:4]), cname


@contextlib.contextmanager
def environment(env):
    keys = ("ER_GEMM_TILE", "ER_GEMM_F32_DMA", "ER_GEMM_STREAM")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def nan_rows(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def device_inputs(cname, kind, fam):
    """Device operands of (case, family): gate and resid as views into NaN-padded allocations (module docstring)."""
    c, o = CASES[cname], operands(cname, kind)
    a, w = family_operands(cname, kind, fam)
    d = SimpleNamespace(a=a.to(DEV), w=(w if fam == "F32" else w.half()).to(DEV), bias=o.bias.to(DEV), gate=None, resid=None)
    mpad = up(c.M, 256)
    if c.gate_rows:
        nb = o.gate.shape[0]
        big = nan_rows(-(-mpad // c.gate_rows) + 1, up(c.N, 4) if c.pad4 else c.N)
        big[:nb, :c.N] = o.gate.to(DEV)
        d.gate_alloc, d.gate = big, big[:nb, :c.N]
    if c.resid:
        rr = o.resid.shape[0]
        big = nan_rows(256 + rr + mpad, (c.N + 9) | 1 if c.odd_ld else up(c.N, 4) + 4)
        big[256:256 + rr, :c.N] = o.resid.to(DEV)
        d.resid_alloc, d.resid = big, big[256:256 + rr, :c.N]
    return d


def launch(cname, kind, form):
    """Runs (case, form); returns the C allocation, the c16 allocation (None outside HH) - both with their guard rows and columns."""
    from edgerunner_amd import kernels, native
    fam, env, force_tile = FORMS[form]
    c, d = CASES[cname], device_inputs(cname, kind, fam)
    ldc = (c.N + 9) | 1 if c.odd_ld else up(c.N, 4) + 8
    call = torch.full((c.M + 3, ldc), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    h16 = torch.full((c.M + 3, ldc), NAN16, dtype=torch.int16, device=DEV).view(torch.float16) if fam == "HH" else None
    with environment(env):
        kernels.gemm_epi(getattr(native, "ER_GEMM_" + fam), d.a, d.w, call[1:1 + c.M, :c.N], bias=d.bias, resid=d.resid, resid_mod=c.resid_mod,
                         gate=d.gate, gate_rows=c.gate_rows, c16=None if h16 is None else h16[1:1 + c.M, :c.N], relu=c.relu,
                         div=c.div32 if fam == "F32" else 0.0, force_tile=force_tile)
    torch.cuda.synchronize()
    return call, h16


@functools.lru_cache(maxsize=None)
def random_outputs(cname, form):
    return launch(cname, "random", form)


def check_sentinels(cname, call, h16, what):
    c = CASES[cname]
    for t, bits, sent in ((call, torch.int32, NAN32), (h16, torch.int16, NAN16)):
        if t is None:
            continue
        inside = torch.zeros(t.shape, dtype=torch.bool, device=DEV)
        inside[1:1 + c.M, :c.N] = True
        raw = t.view(bits)
        touched = (raw != sent) & ~inside
        assert not touched.any(), f"{what}: wrote outside [0, M) x [0, N): first at {touched.nonzero()[0].tolist()} (row 1 = m 0)"
        nans = torch.isnan(t[1:1 + c.M, :c.N])
        assert not nans.any(), f"{what}: {int(nans.sum())} NaN inside (an unwritten element or a spare table row used): first at {nans.nonzero()[0].tolist()}"


@gpu
@pytest.mark.parametrize("cname", list(CASES))
@pytest.mark.parametrize("form", list(FORMS))
def test_exact(form, cname):
    c = CASES[cname]
    call, h16 = launch(cname, "exact", form)
    check_sentinels(cname, call, h16, f"{form} {cname}")
    ref = reference_dev(cname, "exact", FORMS[form][0])
    got = call[1:1 + c.M, :c.N]
    bad = got.double() != ref
    assert not bad.any(), f"{form} {cname}: {int(bad.sum())}/{bad.numel()} elements differ from the exact reference, first at (m, n) = " \
                          f"{bad.nonzero()[0].tolist()}: got {float(got[tuple(bad.nonzero()[0])])}, want {float(ref[tuple(bad.nonzero()[0])])}"
    if h16 is not None:
        bad = h16[1:1 + c.M, :c.N] != ref.half()
        assert not bad.any(), f"{form} {cname}: c16 differs from fp16(reference) at {int(bad.sum())} elements, first {bad.nonzero()[0].tolist()}"


@gpu
@pytest.mark.parametrize("cname", list(CASES))
@pytest.mark.parametrize("form", list(FORMS))
def test_random(form, cname):
    c, fam = CASES[cname], FORMS[form][0]
    call, h16 = random_outputs(cname, form)
    check_sentinels(cname, call, h16, f"{form} {cname}")
    ref = reference_dev(cname, "random", fam)
    got = call[1:1 + c.M, :c.N]
    atol = 2 * (2e-6 + 1e-7 * c.K) if fam in ("F32", "F16S") else 2 * (1e-5 + 2e-7 * c.K)
    err = (got.double() - ref).abs()
    tol = atol + 1e-5 * ref.abs()
    print(f"{form} {cname}: max abs err {float(err.max()):.3e}, atol {atol:.3e}, largest err / tol {float((err / tol).max()):.3f}")
    bad = err > tol
    assert not bad.any(), f"{form} {cname}: {int(bad.sum())}/{bad.numel()} beyond {atol:.2e} + 1e-5 |ref|, max abs err {float(err.max()):.3e}, " \
                          f"first at (m, n) = {bad.nonzero()[0].tolist()}"
    if h16 is not None:
        assert torch.equal(h16[1:1 + c.M, :c.N], got.half()), f"{form} {cname}: c16 is not fp16(C)"


@gpu
@pytest.mark.parametrize("cname", list(CASES))
def test_forms_give_equal_bits(cname):
    for group, forms in BIT_GROUPS.items():
        c0, h0 = random_outputs(cname, forms[0])
        for f in forms[1:]:
            c1, h1 = random_outputs(cname, f)
            diff = c1.view(torch.int32) != c0.view(torch.int32)
            assert not diff.any(), f"{cname}, {group}: {f} differs from {forms[0]} at {int(diff.sum())} elements, first {diff.nonzero()[0].tolist()} " \
                                   f"(row 1 = m 0): {float(c1[tuple(diff.nonzero()[0])])!r} vs {float(c0[tuple(diff.nonzero()[0])])!r}"
            if h0 is not None:
                assert torch.equal(h1.view(torch.int16), h0.view(torch.int16)), f"{cname}, {group}: c16 of {f} differs from {forms[0]}"


@gpu
def test_refusals():
    """ER_ERR_INVALID (-1) before any launch: the sentinel output is untouched."""
    from edgerunner_amd import kernels, native
    M, N = 40, 64
    out = torch.full((M, N), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    out16 = torch.full((M, N), NAN16, dtype=torch.int16, device=DEV).view(torch.float16)
    gate = torch.ones((1, N), device=DEV)

    def ops(k, half, ldb=None):
        a = torch.ones((M, k), device=DEV)
        w = torch.ones((N, ldb or k), device=DEV, dtype=torch.float16 if half else torch.float32)[:, :k]
        return a, w

    F32, F16, F16S, HH = native.ER_GEMM_F32, native.ER_GEMM_F16, native.ER_GEMM_F16S, native.ER_GEMM_HH
    refused = [
        ("gate_rows 0", F32, ops(64, False), dict(gate=gate, gate_rows=0)),
        ("gate_rows -3", HH, ops(64, True), dict(gate=gate, gate_rows=-3)),
        ("fp32 k % 16", F32, ops(24, False), {}),
        ("fp16 k % 32", F16, ops(48, True), {}),
        ("split k % 32", F16S, ops(48, True), {}),
        ("hh k % 64", HH, ops(96, True), {}),
        ("hh ldb % 8", HH, ops(64, True, ldb=68), {}),
        ("fp16 ldb % 8", F16, ops(64, True, ldb=68), {}),
        ("fp32 ldb % 4", F32, ops(64, False, ldb=66), {}),
        ("c16 with fp16", F16, ops(64, True), dict(c16=out16)),
        ("c16 with fp32", F32, ops(64, False), dict(c16=out16)),
        ("c16 with split", F16S, ops(64, True), dict(c16=out16)),
    ]
    for what, fam, (a, w), kw in refused:
        with pytest.raises(native.NativeError, match=r"er_k_gemm_epi failed \(-1\)"):
            kernels.gemm_epi(fam, a, w, out, **kw)
        torch.cuda.synchronize()
        assert (out.view(torch.int32) == NAN32).all() and (out16.view(torch.int16) == NAN16).all(), f"{what}: refused, yet the output was written"
    a, w = ops(64, True)
    kernels.gemm_epi(HH, a, w, out, gate=gate, gate_rows=M, c16=out16)      # the same operands are accepted once legal
    torch.cuda.synchronize()
    assert (out == 64).all() and (out16 == 64).all()
