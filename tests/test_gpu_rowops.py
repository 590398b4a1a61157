"""Unit tests of the once-per-sample row, element-wise and K/V scatter kernels of csrc/k_rowops.h and split_rows_f16_kernel, each
through the launcher the product calls.  References, gates, value sweeps and the mutants that show what the cases can see:
tests/rowops_ref.py, tests/test_rowops_ref_cpu.py.  The DiT / CLIP kernels of csrc/k_dit.h: tests/test_gpu_dit_elementwise.py.

  kernel                    launcher                  product call sites                                     test
  kv_scatter_half_kernel    launch_kv_scatter         prefill_run (fast mode)                                test_kv_scatter[half-*]
  kv_scatter_f8_kernel      launch_kv_scatter         prefill_run (kv8 mode)                                 test_kv_scatter[f8-*]
  split_rows_f16_kernel     launch_split_rows_f16     linear_hs (fast prefill), er_k_gemm_f16s               test_split_rows_f16
  add_pos_kernel            launch_add_pos            prefill_run, dit_forward_impl (in place)               test_add_pos
  gather_rows_kernel        launch_gather_rows        er_embed_tokens                                        test_gather_rows
  point_embed_kernel        launch_point_embed        point_latent_chunk                                     test_point_embed
  geglu_kernel              launch_geglu              point_latent_chunk, dit_forward_impl (fp32)            test_geglu
  layernorm_rows_kernel<6>  launch_layernorm          prefill, point encoder (in place), CLIP (in place)...  test_layernorm*
  softmax_rows_kernel       launch_softmax_rows       attention_full (batch stride, causal offset)           test_softmax_*

Every output sits between guards of sentinel bits; whatever the operation does not write must keep them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256                      # elements in front of and behind every output (keeps 16-byte alignment for every width)
WORST = {}                       # operation -> (err / gate, where)


def note(op, r, where):
    if r > WORST.get(op, (-1.0, ""))[0]:
        WORST[op] = (r, where)


class Guarded:
    """n elements of `dtype` between two guards, all sentinel; `live` is the middle."""

    def __init__(self, n, dtype, init=None):
        self.n = n
        self.all = R.filled((GUARD + n + GUARD,), dtype, DEV)
        self.live = self.all[GUARD:GUARD + n]
        if init is not None:
            self.live.copy_(init.reshape(-1))

    def guards_intact(self):
        return bool(R.is_sentinel(self.all[:GUARD]).all()) and bool(R.is_sentinel(self.all[GUARD + self.n:]).all())


def K():
    from edgerunner_amd import kernels
    return kernels


def native_error():
    from edgerunner_amd import native
    return native.NativeError


# ---------------------------------------------------------------------------------------------- K/V scatter
SCATTER_SHAPES = {          # B, S, hidden, head_dim, l_cap, slack of kv_bstride over heads * l_cap * head_dim
    "strided": (32, 2050, 64, 16, 2080, 64),          # 65600 rows: grid.y is capped at 65535, the last 65 tokens of row 31 are strided
    "product_3x5": (3, 5, 1536, 96, 8, 0),
    "product_2x1": (2, 1, 1536, 96, 4, 192),
    "partial_block": (3, 7, 96, 4, 9, 4),             # 2 * hidden / 4 = 48 threads of a 256-thread workgroup
}


def scatter_input(B, S, hidden, f8, seed):
    """q, K and V thirds from three seeds (a swap shows); the value sweep at the start of K and, shifted, of V - and again in the
    last token row, which the strided shape reaches only through the stride loop"""
    M = B * S
    qkv = torch.cat((R.randn(seed, M, hidden), R.randn(seed + 1, M, hidden), R.randn(seed + 2, M, hidden)), dim=1)
    sweep = R.e4m3_sweep() if f8 else R.half_sweep()
    for which, shift in ((1, 0), (2, 5)):
        third = qkv[:, which * hidden:(which + 1) * hidden]
        flat = third.reshape(-1).clone()
        n = min(sweep.numel(), flat.numel() - shift)
        flat[shift:shift + n] = sweep[:n]
        tail = min(sweep.numel(), hidden)
        flat[-tail:] = sweep.flip(0)[:tail]
        third.copy_(flat.view(M, hidden))
    return qkv


@pytest.mark.parametrize("shape", list(SCATTER_SHAPES))
@pytest.mark.parametrize("cache", ["half", "f8"])
def test_kv_scatter(cache, shape):
    """cache == round-to-nearest-even fp16 (e4m3: tests/kv8_ref.py's cast) of the fp32 K / V columns at [b][h][s < S][d]; rows s >= S,
    the gap between batch rows and both guards keep the sentinel; the scratch's q third keeps its bits and its K / V thirds hold the
    stored values widened again."""
    B, S, hidden, hd, l_cap, slack = SCATTER_SHAPES[shape]
    f8 = cache == "f8"
    bstride = hidden * l_cap + slack
    qkv = scatter_input(B, S, hidden, f8, 100)
    want_qkv, want_k, want_v = R.kv_scatter(qkv, B, S, hidden, hd, l_cap, bstride, f8, GUARD)
    dt = torch.uint8 if f8 else torch.float16
    kc, vc = Guarded(B * bstride, dt), Guarded(B * bstride, dt)
    scratch = Guarded(qkv.numel(), torch.float32, qkv.to(DEV))
    K().kv_scatter_(scratch.live, kc.live, vc.live, B * S, S, hidden, hd, l_cap, bstride)
    torch.cuda.synchronize()
    assert R.bits_equal(kc.all, want_k), "K cache (values, untouched rows s >= S, batch gaps, guards)"
    assert R.bits_equal(vc.all, want_v), "V cache (values, untouched rows s >= S, batch gaps, guards)"
    got = scratch.live.view(B * S, 3 * hidden).cpu()
    assert R.bits_equal(got[:, :hidden], qkv[:, :hidden]), "the q third must keep its bits"
    assert R.bits_equal(got, want_qkv), "the K / V thirds of the scratch hold the stored values widened"
    assert scratch.guards_intact()


def test_kv_scatter_refusals():
    kc, vc, qkv = Guarded(4096, torch.float16), Guarded(4096, torch.float16), Guarded(4096, torch.float32)
    bad = [dict(hidden=18, hd=6), dict(hidden=16, hd=2), dict(M=7), dict(S=9), dict(bstride=16 * 8 + 2), dict(bstride=16 * 8 - 4), dict(M=0)]
    for b in bad:
        a = dict(M=6, S=3, hidden=16, hd=4, l_cap=8, bstride=16 * 8)
        a.update(b)
        with pytest.raises(native_error()):
            K().kv_scatter_(qkv.live, kc.live, vc.live, a["M"], a["S"], a["hidden"], a["hd"], a["l_cap"], a["bstride"])
    with pytest.raises(native_error()):
        K().kv_scatter_(None, kc.live, vc.live, 6, 3, 16, 4, 8, 128)
    torch.cuda.synchronize()
    for g in (kc, vc, qkv):
        assert bool(R.is_sentinel(g.all).all()), "a refused call writes nothing"


# ---------------------------------------------------------------------------------------------- split_rows_f16
@pytest.mark.parametrize("rows,cols,ldx", [(70000, 64, 72), (3, 1536, 1536), (5, 6144, 6144)])
def test_split_rows_f16(rows, cols, ldx):
    """hi = fp16(x), lo = fp16(x - hi) bit for bit; 70000 rows reach the stride loop over grid.y; the padding columns of x are NaN"""
    x = torch.full((rows, ldx), float("nan"))
    x[:, :cols] = R.randn(110, rows, cols)
    sweep = R.half_sweep()
    n = min(sweep.numel(), cols)
    x[0, :n], x[rows - 1, :n] = sweep[:n], sweep.flip(0)[:n]
    x[rows // 2, :n] = sweep[-n:]
    hi_want, lo_want = R.split_rows(x[:, :cols].contiguous())
    hi, lo = Guarded(rows * cols, torch.float16), Guarded(rows * cols, torch.float16)
    K().split_rows_f16_(x.to(DEV), hi.live, lo.live, rows, cols, ldx)
    torch.cuda.synchronize()
    assert R.bits_equal(hi.live.view(rows, cols), hi_want) and R.bits_equal(lo.live.view(rows, cols), lo_want)
    assert hi.guards_intact() and lo.guards_intact()
    with pytest.raises(native_error()):
        K().split_rows_f16_(x.to(DEV), hi.live, lo.live, rows, cols - 2, ldx)


# ---------------------------------------------------------------------------------------------- add_pos
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("pos0", [0, 37])
@pytest.mark.parametrize("B,S,C", [(3, 700, 1024), (1, 1, 4)])
def test_add_pos(B, S, C, pos0, in_place):
    """one fp32 add per element, bit for bit; 3 x 700 x 1024 / 4 = 537600 vector elements walk the stride loop (524288 threads); the
    position table is longer than pos0 + S and its other rows are NaN"""
    emb = R.randn(120, B, S, C)
    pos = torch.full((pos0 + S + 5, C), float("nan"))
    pos[pos0:pos0 + S] = R.randn(121, S, C)
    want = R.add_pos(emb, pos, pos0)
    src = Guarded(emb.numel(), torch.float32, emb.to(DEV))
    dst = src if in_place else Guarded(emb.numel(), torch.float32)
    K().add_pos_(src.live, pos.to(DEV), dst.live, B, S, C, pos0)
    torch.cuda.synchronize()
    assert R.bits_equal(dst.live.view(B, S, C), want)
    assert dst.guards_intact() and src.guards_intact()
    if not in_place:
        assert R.bits_equal(src.live.view(B, S, C), emb)
    with pytest.raises(native_error()):
        K().add_pos_(src.live, pos.to(DEV), dst.live, B, S, C + 2, pos0)


# ---------------------------------------------------------------------------------------------- gather_rows
@pytest.mark.parametrize("C,ldo", [(1536, 1536), (1536, 1600), (100, 100), (100, 108)])
def test_gather_rows(C, ldo):
    rows = 11
    table = R.randn(130, rows, C)
    ids = [0, rows - 1, 3, 3, rows - 1, 0, 7, 3]
    want = R.filled((len(ids), ldo), torch.float32)
    want[:, :C] = R.gather_rows(table, ids)
    out = Guarded(len(ids) * ldo, torch.float32)
    K().gather_rows_(table.to(DEV), ids, out.live, C, ldo)
    torch.cuda.synchronize()
    assert R.bits_equal(out.live.view(len(ids), ldo), want), "rows, and sentinels in the padding columns"
    assert out.guards_intact()
    for bad in ([0, rows], [-1]):
        with pytest.raises(native_error()):
            K().gather_rows_(table.to(DEV), bad, out.live, C, ldo)
    torch.cuda.synchronize()
    assert R.bits_equal(out.live.view(len(ids), ldo), want), "a refused call writes nothing"


# ---------------------------------------------------------------------------------------------- point_embed
@pytest.mark.parametrize("M", [8200, 1])
def test_point_embed(M):
    """M = 8200 rows of 64 columns = 524800 elements: the stride loop runs; the basis is the reference's (2^k pi, k < 8, per axis);
    columns 51 .. 63 exactly zero, the xyz columns the input's bits; one gate per column (frequency)"""
    F, ldo = 24, 64
    pts, basis = R.point_cloud(M, 140), R.point_basis()
    out = Guarded(M * ldo, torch.float32)
    K().point_embed_(pts.to(DEV), basis.to(DEV), out.live, M, F, ldo)
    torch.cuda.synchronize()
    got = out.live.view(M, ldo).cpu()
    assert out.guards_intact()
    assert R.bits_equal(got[:, 48:51], pts), "xyz columns"
    assert R.bits_equal(got[:, 51:], torch.zeros(M, ldo - 51)), "padding columns"
    r = R.check(got, R.point_embed(pts, basis, ldo), R.point_embed(pts, basis, ldo, torch.float32), None, (0,), f"point_embed M={M}")
    note("point_embed", r, f"M={M}")
    print(f"point_embed M={M}: worst err / gate {r:.3f}")
    with pytest.raises(native_error()):
        K().point_embed_(pts.to(DEV), basis.to(DEV), out.live, M, F, 50)


# ---------------------------------------------------------------------------------------------- geglu
@pytest.mark.parametrize("rows,F,values", [(257, 2049, "grid"), (257, 2049, "randn"), (1, 3, "randn")])
def test_geglu(rows, F, values):
    """257 x 2049 = 526593 outputs: past the 524288 threads of the capped grid and no multiple of 256"""
    n = rows * F
    gates = (R.ew_values(n, 150) if values == "grid" else R.randn(150, n)).view(rows, F)
    u = torch.cat((R.randn(151, rows, F), gates), dim=1).contiguous()
    out = Guarded(n, torch.float32)
    K().geglu_(u.to(DEV), out.live, rows, F)
    torch.cuda.synchronize()
    assert out.guards_intact()
    r = R.check(out.live.view(rows, F).cpu(), R.geglu(u), R.geglu(u, torch.float32), None, None, f"geglu {rows}x{F} {values}")
    note("geglu", r, f"{rows}x{F} {values}")
    print(f"geglu {rows}x{F} {values}: worst err / gate {r:.3f}")


# ---------------------------------------------------------------------------------------------- layernorm
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("rows", [1, 5, 2051])
@pytest.mark.parametrize("cols", [64, 256, 512, 1024, 1280, 1536])
def test_layernorm(cols, rows, in_place):
    """all six widths of launch_layernorm; N(0, 1) rows next to hard ones (mean 1000; spread 1e-3 around 0.3; one column at 1e4),
    gated as two groups (rowops_ref.check_rows); the constant rows (0.5, -3: exact fp32 sums, tests/test_rowops_ref_cpu.py) must
    give b bit for bit"""
    from edgerunner_amd import native
    x, const, hard = R.layernorm_rows(rows, cols, 160 + cols)
    w, b = 1 + 0.1 * R.randn(161, cols), 0.1 * R.randn(162, cols)
    src = Guarded(x.numel(), torch.float32, x.to(DEV))
    dst = src if in_place else Guarded(x.numel(), torch.float32)
    wd, bd = w.to(DEV), b.to(DEV)
    native.check(native.load_library().er_k_layernorm(native.ptr(src.live), native.ptr(wd), native.ptr(bd), native.ptr(dst.live), rows, cols,
                                                      1e-5, None), "er_k_layernorm")
    torch.cuda.synchronize()
    got = dst.live.view(rows, cols).cpu()
    assert dst.guards_intact() and src.guards_intact()
    for r_ in const:
        assert R.bits_equal(got[r_], b), f"constant row {r_}: the output is b"
    r = R.check_rows(got, R.layernorm(x, w, b, 1e-5), R.layernorm(x, w, b, 1e-5, torch.float32), hard, R.TOL_LAYERNORM, f"layernorm {rows}x{cols}")
    note("layernorm", r, f"{rows}x{cols}{' in place' if in_place else ''}")
    print(f"layernorm {rows}x{cols}: worst err / gate {r:.3f}")


def test_layernorm_refuses_other_widths():
    x = Guarded(5 * 96, torch.float32, R.randn(170, 5, 96).to(DEV))
    y = Guarded(5 * 96, torch.float32)
    w = torch.ones(96, device=DEV)
    with pytest.raises(native_error()):
        K().layernorm(x.live.view(5, 96), w, w)
    from edgerunner_amd import native
    rc = native.load_library().er_k_layernorm(native.ptr(x.live), native.ptr(w), native.ptr(w), native.ptr(y.live), 5, 96, 1e-5, None)
    torch.cuda.synchronize()
    assert rc < 0 and bool(R.is_sentinel(y.all).all()), "width 96 is refused and the output untouched"


# ---------------------------------------------------------------------------------------------- softmax
def softmax_check(got, s, nv, cols, ld_pad, what):
    """got / s [batch, rows, ld]: the gate over the live columns; zeros in [n_valid, ld_pad); sentinels beyond"""
    live = s[..., :cols]
    r = R.check(got[..., :cols], R.softmax_rows(live, nv), R.softmax_rows(live, nv, torch.float32), R.TOL_SOFTMAX, (-1,), what)
    hidden = ~(torch.arange(ld_pad)[None] < nv[:, None])
    assert bool((got[..., :ld_pad][:, hidden] == 0).all()), f"{what}: columns [n_valid, ld_pad) must be zero"
    assert bool(R.is_sentinel(got[..., ld_pad:]).all()), f"{what}: columns beyond ld_pad must stay untouched"
    note("softmax", r, what)
    print(f"{what}: worst err / gate {r:.3f}")


@pytest.mark.parametrize("cols", [15360, 15364])
def test_softmax_lds_rule(cols):
    """the two sides of launch_softmax_rows' LDS rule (a row of up to 15360 columns is staged in LDS, a longer one is not), through
    the old entry: ld_pad == ld there, so the padding becomes zero"""
    ld, rows = 15376, 3
    s, nv = R.softmax_scores(1, rows, cols, ld, ld, 0, False, 180)
    buf = Guarded(rows * ld, torch.float32, s.to(DEV))
    K().softmax_(buf.live.view(rows, ld), cols, False)
    torch.cuda.synchronize()
    assert buf.guards_intact()
    softmax_check(buf.live.view(1, rows, ld).cpu(), s, nv, cols, ld, f"softmax cols={cols}")


@pytest.mark.parametrize("causal,causal_off", [(False, 0), (True, 0), (True, 130)])
def test_softmax_batched(causal, causal_off):
    """as attention_full calls it: 3 score matrices a batch stride apart (larger than rows * ld: the gap keeps its sentinels), N = 70
    queries over M = 200 keys, causal with the offset M - N = 130 and with 0"""
    batch, rows, cols, ld_pad, ld = 3, 70, 200, 208, 216
    bstride = rows * ld + 40
    s, nv = R.softmax_scores(batch, rows, cols, ld_pad, ld, causal_off, causal, 190)
    buf = Guarded(batch * bstride, torch.float32)
    view = buf.live.view(batch, bstride)
    view[:, :rows * ld] = s.view(batch, -1).to(DEV)
    K().softmax_batched_(buf.live, rows, cols, ld, ld_pad, batch, bstride, causal, causal_off)
    torch.cuda.synchronize()
    assert buf.guards_intact() and bool(R.is_sentinel(view[:, rows * ld:]).all()), "guards and the gap between batches"
    softmax_check(view[:, :rows * ld].reshape(batch, rows, ld).cpu(), s, nv, cols, ld_pad, f"softmax batched causal={causal} off={causal_off}")
    for bad in (dict(ld_pad=cols - 4), dict(ld=ld_pad - 8), dict(causal_off=-1), dict(bstride=rows * ld - 8)):
        a = dict(ld=ld, ld_pad=ld_pad, bstride=bstride, causal_off=causal_off)
        a.update(bad)
        with pytest.raises(native_error()):
            K().softmax_batched_(buf.live, rows, cols, a["ld"], a["ld_pad"], batch, a["bstride"], causal, a["causal_off"])


def test_zz_worst_ratios():
    for op in sorted(WORST):
        print(f"rowops worst: {op:16s} {WORST[op][0]:.3f}  at {WORST[op][1]}")
    assert all(r <= 1.0 for r, _ in WORST.values())
