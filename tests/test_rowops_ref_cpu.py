"""CPU side of the row / element-wise / K-V scatter kernel tests (tests/rowops_ref.py; no GPU, no library).

Three things are held here so that the GPU files can lean on them:
  1. the identities the exact operations are compared with are right on the CPU: torch's fp16 cast of the value sweep against
     numpy's, the e4m3 cast against a nearest-code search, unfold against a loop, the constant LayerNorm rows' sums exact;
  2. on every case the float32 reference is finite and inside the gate;
  3. every mutant - a float32 / integer emulation of the operation with ONE plausible bug - is OUTSIDE the gate or the identity on
     at least one case, so the case list can see that bug.  A mutant that passes means the cases are too weak, not the gate."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref  # noqa: E402
import rowops_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ 1. identities
def test_half_sweep_cast_is_round_to_nearest_even():
    x = R.half_sweep()
    with np.errstate(over="ignore"):                                   # 65520 and beyond become infinity: meant
        want = torch.from_numpy(x.numpy().astype(np.float16))
    got = x.half()
    assert R.bits_equal(got, want)
    assert not torch.isnan(x).any() and not torch.isinf(x).any()
    # the sweep holds what it promises: ties resolved down and up, subnormals, -0, the largest, overflow to infinity
    h = got.float()
    up, down = (h.abs() > x.abs()).sum(), (h.abs() < x.abs()).sum()
    assert up > 20 and down > 20
    assert (got.view(torch.int16) == -32768).any() and (h == 65504).any() and torch.isinf(h).any()
    assert ((h != 0) & (h.abs() < 2.0 ** -14)).sum() > 10
    assert not R.bits_equal(R.trunc_half(x), want)
    hi, lo = R.split_rows(x)
    assert (lo[torch.isfinite(hi.float())].float() != 0).any()


def test_e4m3_sweep_cast_is_nearest_code_ties_to_even():
    x = R.e4m3_sweep()
    got = kv8_ref.torch_kv8(x)
    table = kv8_ref.kv8_decode(torch.arange(0x7F, dtype=torch.int32).to(torch.uint8)).double()      # the 127 finite magnitudes, ascending
    a = x.double().abs().clamp(max=448.0)
    d = (a[:, None] - table[None]).abs()
    best = d.min(dim=1).values
    cand = d == best[:, None]
    lo_code = cand.float().argmax(dim=1)
    hi_code = 0x7E - cand.flip(1).float().argmax(dim=1)
    code = torch.where(lo_code % 2 == 0, lo_code, hi_code)             # one candidate: both equal; a tie: the even byte
    sign = (x.view(torch.int32) < 0).to(torch.int64) * 0x80
    assert torch.equal(got.long(), code + sign)
    assert (lo_code != hi_code).sum() > 100                            # the ties are there


def test_unfold_is_the_patch_loop():
    for S, P, lda in ((28, 14, 592), (8, 4, 48)):
        px = R.randn(3, 2, 3, S, S)
        assert torch.equal(R.clip_im2col(px, P, lda), R.im2col_loop(px, P, lda))


@pytest.mark.parametrize("cols", [64, 256, 512, 1024, 1280, 1536])
def test_constant_rows_have_exact_fp32_sums(cols):
    """0.5 and -3 over any of the six widths: every partial sum in any order is a multiple of 0.5 below 2^24 ulps - exact - so the
    fp32 mean is the constant, every difference 0 and LayerNorm's output is b bit for bit."""
    for c in (0.5, -3.0):
        x = torch.full((cols,), c)
        assert float(x.cumsum(0)[-1]) == c * cols and float(x.flip(0).cumsum(0)[-1]) == c * cols
        assert abs(c) * cols < 2 ** 24 * 0.5
        assert float(torch.tensor(c * cols) / cols) == c
        w, b = R.randn(1, cols), R.randn(2, cols)
        y = (x - c) * (1.0 / math.sqrt(1e-5)) * w + b
        assert R.bits_equal(y, b)


# ------------------------------------------------------------------------------------------------ 2. and 3.: exact operations
def _scatter_emulated(qkv, B, S, hidden, hd, l_cap, bstride, f8, guard, s_of, skip=lambda m: False):
    """the K cache allocation by the kernel's own index walk, token by token, with the position rule s_of(m, b)"""
    a = R.filled((guard + B * bstride + guard,), torch.uint8 if f8 else torch.float16)
    stored = R.kv_round(qkv[:, hidden:2 * hidden], f8)[0]
    for m in range(B * S):
        if skip(m):
            continue
        b = m // S
        s = s_of(m, b)
        for h in range(hidden // hd):
            o = guard + b * bstride + (h * l_cap + s) * hd
            a[o:o + hd] = stored[m, h * hd:(h + 1) * hd]
    return a


def _identity_mutants():
    """[(operation, mutant name, identity output(s), mutant output(s))]"""
    out = []
    # gather_rows
    table, ids = R.randn(1, 9, 100), [0, 8, 3, 3, 8, 0, 5]
    ldo = 104
    want = R.filled((len(ids), ldo), torch.float32)
    want[:, :100] = R.gather_rows(table, ids)
    m = R.filled((len(ids), ldo), torch.float32)
    m.view(-1)[:len(ids) * 100] = R.gather_rows(table, ids).reshape(-1)
    out.append(("gather_rows", "ldo ignored", want, m))
    # add_pos
    for pos0 in (0, 37):
        B, S, C = 3, 7, 8
        emb, pos = R.randn(2, B, S, C), R.randn(3, pos0 + S + 3, C)
        want = R.add_pos(emb, pos, pos0)
        row = torch.arange(B * S)
        out.append(("add_pos", "s = row % (S + 1)", want, emb + pos[pos0 + row % (S + 1)].view(B, S, C)))
        if pos0:
            out.append(("add_pos", "pos0 ignored", want, emb + pos[row % S].view(B, S, C)))
    # adaLN gates
    tabs, tada = [R.randn(10 + i, 6, 100) for i in range(2)], R.randn(4, 3, 6, 100)
    out.append(("adaln_gate", "table row idx + 1", R.adaln_gate(tabs[0], tada, 2), tabs[0][3][None] + tada[:, 2]))
    out.append(("adaln_gate_all", "gate chunk 4 for 5", R.adaln_gate_all(tabs, tada),
                torch.stack([torch.stack((R.adaln_gate(t, tada, 2), R.adaln_gate(t, tada, 4))) for t in tabs])))
    # clip_assemble / im2col
    patches, cls, pos = R.randn(5, 2, 4, 16), R.randn(6, 16), R.randn(7, 5, 16)
    mut = torch.cat((cls[None, None].expand(2, 1, -1) + pos[0], patches + pos[None, :4]), dim=1)
    out.append(("clip_assemble", "patch p takes pos[p]", R.clip_assemble(patches, cls, pos), mut))
    px = R.randn(8, 2, 3, 8, 8)
    out.append(("clip_im2col", "ky and kx swapped", R.clip_im2col(px, 4, 48), R.clip_im2col(px.transpose(2, 3), 4, 48).view(2, 2, 2, 48)
                .transpose(1, 2).reshape(8, 48)))
    # fp16 roundings
    x = R.half_sweep()
    hi, lo = R.split_rows(x)
    out.append(("split_rows_f16", "truncating cast", hi, R.trunc_half(x)))
    out.append(("split_rows_f16", "lo dropped", lo, torch.zeros_like(lo)))
    out.append(("ln_modulate y16", "truncating cast", x.half(), R.trunc_half(x)))
    # K/V scatter
    for f8 in (False, True):
        B, S, hidden, hd, l_cap = 2, 3, 16, 4, 5
        bstride = hidden * l_cap + 8
        sweep = R.e4m3_sweep() if f8 else R.half_sweep()
        qkv = torch.cat((R.randn(11, B * S, hidden), R.randn(12, B * S, hidden), R.randn(13, B * S, hidden)), dim=1)
        qkv[0, hidden:2 * hidden] = sweep[:hidden]
        qkv[1, 2 * hidden:] = sweep[hidden:2 * hidden]
        want = R.kv_scatter(qkv, B, S, hidden, hd, l_cap, bstride, f8, 8)
        swapped = torch.cat((qkv[:, :hidden], qkv[:, 2 * hidden:], qkv[:, hidden:2 * hidden]), dim=1)
        ms, mk, mv = R.kv_scatter(swapped, B, S, hidden, hd, l_cap, bstride, f8, 8)
        name = "kv_scatter f8" if f8 else "kv_scatter half"
        out.append((name, "K and V swapped", want[1], mk))
        out.append((name, "scratch left unrounded", want[0], qkv))
        out.append((name, "s = m - b * (S + 1)", want[1], _scatter_emulated(qkv, B, S, hidden, hd, l_cap, bstride, f8, 8,
                                                                            lambda m, b: (m - b * (S + 1)) % l_cap)))
        out.append((name, "row stride one short", want[1], _scatter_emulated(qkv, B, S, hidden, hd, l_cap, bstride, f8, 8,
                                                                             lambda m, b: m - b * S, skip=lambda m: m == B * S - 1)))
        if not f8:
            k = qkv[:, hidden:2 * hidden]
            t = R.filled(want[1].shape, torch.float16)
            t[8:8 + B * bstride].view(B, bstride)[:, :hidden * l_cap].view(B, hidden // hd, l_cap, hd)[:, :, :S] = \
                R.trunc_half(k).view(B, S, hidden // hd, hd).permute(0, 2, 1, 3)
            out.append((name, "truncating cast", want[1], t))
    return out


IDENTITY_MUTANTS = _identity_mutants()


@pytest.mark.parametrize("i", range(len(IDENTITY_MUTANTS)), ids=[f"{m[0]}: {m[1]}" for m in IDENTITY_MUTANTS])
def test_identity_mutant_is_caught(i):
    _, _, want, got = IDENTITY_MUTANTS[i]
    assert not R.bits_equal(got, want)


@pytest.mark.parametrize("f8", [False, True])
def test_scatter_emulation_with_the_right_rule_is_the_identity(f8):
    B, S, hidden, hd, l_cap, bstride = 2, 3, 16, 4, 5, 88
    qkv = R.randn(14, B * S, 3 * hidden)
    assert R.bits_equal(_scatter_emulated(qkv, B, S, hidden, hd, l_cap, bstride, f8, 8, lambda m, b: m - b * S),
                        R.kv_scatter(qkv, B, S, hidden, hd, l_cap, bstride, f8, 8)[1])


def test_every_exact_operation_has_a_mutant():
    ops = {m[0] for m in IDENTITY_MUTANTS}
    assert ops == {"gather_rows", "add_pos", "adaln_gate", "adaln_gate_all", "clip_assemble", "clip_im2col", "split_rows_f16",
                   "ln_modulate y16", "kv_scatter half", "kv_scatter f8"}


# ------------------------------------------------------------------------------------------------ 2. and 3.: rounding operations
def _tanh_gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def _ln_mut(x, w, b, eps, kind):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    if kind == "variance / (n - 1)":
        return d / torch.sqrt((d * d).sum(-1, keepdim=True) / (x.shape[-1] - 1) + eps) * w + b
    if kind == "eps outside the root":
        return d / (torch.sqrt((d * d).mean(-1, keepdim=True)) + eps) * w + b
    raise ValueError(kind)


def _gated_cases():
    """[(operation, case name, ref64, ref32, tol, dims, {mutant name: output})]"""
    cases = []
    # layernorm
    for cols in (64, 1536):
        x, _, _ = R.layernorm_rows(5, cols, 20)
        w, b = 1 + 0.1 * R.randn(21, cols), 0.1 * R.randn(22, cols)
        cases.append(("layernorm", f"5x{cols}", R.layernorm(x, w, b, 1e-5), R.layernorm(x, w, b, 1e-5, torch.float32), R.TOL_LAYERNORM,
                      None, {k: _ln_mut(x, w, b, 1e-5, k) for k in ("variance / (n - 1)", "eps outside the root")}))
    # ln_modulate
    for layout in ("layer", "out"):
        c = R.ln_mod_case(10, 5, layout, 30)
        for sh, sc in c.idx:
            r64 = R.ln_modulate(c.x, c.rpb, c.table, c.tvec, sh, sc)
            r32 = R.ln_modulate(c.x, c.rpb, c.table, c.tvec, sh, sc, dt=torch.float32)
            mod = c.table[None] + c.tvec
            bidx = torch.arange(c.rows) // c.rpb
            n = R.layernorm(c.x, torch.ones(c.C), torch.zeros(c.C), 1e-6, torch.float32)
            cases.append(("ln_modulate", f"{layout} ({sh}, {sc})", r64, r32, R.TOL_LAYERNORM, None, {
                "(1 + scale) -> scale": n * mod[bidx, sc] + mod[bidx, sh],
                "shift and scale swapped": R.ln_modulate(c.x, c.rpb, c.table, c.tvec, sc, sh, dt=torch.float32),
                "batch index r / (rows_per_batch + 1)": n * (1 + mod[torch.arange(c.rows) // (c.rpb + 1), sc]) + mod[torch.arange(c.rows) // (c.rpb + 1), sh],
            }))
    # softmax
    s, nv = R.softmax_scores(2, 9, 20, 32, 40, 13, True, 40)
    live = s[..., :20]
    r64, r32 = R.softmax_rows(live, nv), R.softmax_rows(live, nv, torch.float32)
    x = live.masked_fill(~(torch.arange(20)[None] < nv[:, None]), -R.INF)
    no_max = torch.exp(x) / torch.exp(x).sum(-1, keepdim=True)
    cases.append(("softmax", "causal off 13", r64, r32, R.TOL_SOFTMAX, None, {
        "no maximum subtracted": no_max,
        "causal offset ignored": R.softmax_rows(live, torch.clamp(nv - 13, min=1), torch.float32)}))
    # gelu / geglu / silu
    for name, v in (("grid", R.ew_values(5000, 50)), ("randn", R.randn(51, 5000))):
        cases.append(("gelu", name, R.gelu(v), R.gelu(v, torch.float32), None, None, {"tanh form": _tanh_gelu(v)}))
        cases.append(("silu", name, R.silu(v), R.silu(v, torch.float32), None, None, {"sigmoid(1.702 x)": v * torch.sigmoid(1.702 * v)}))
        u = torch.stack((R.randn(52, 5000), v), dim=1).reshape(2500, 4)[:, [0, 2, 1, 3]].contiguous()      # [rows, 2 F], F = 2
        cases.append(("geglu", name, R.geglu(u), R.geglu(u, torch.float32), None, None, {
            "tanh form": u[:, :2] * _tanh_gelu(u[:, 2:]), "halves exchanged": u[:, 2:] * R.gelu(u[:, :2], torch.float32)}))
    # point_embed
    pts, basis = R.point_cloud(50, 60), R.point_basis()
    r64, r32 = R.point_embed(pts, basis, 64), R.point_embed(pts, basis, 64, torch.float32)
    tail = r32.clone()
    tail[:, 48:] = 0
    tail[:, 49:52] = pts
    cases.append(("point_embed", "50 points", r64, r32, None, (0,), {
        "sin and cos halves swapped": torch.cat((r32[:, 24:48], r32[:, :24], r32[:, 48:]), dim=1),
        "xyz at column 2F + 1": tail}))
    # timestep_embed
    t = torch.tensor([0.0, 0.5, 1.0, 500.0, 999.0])
    r64, r32 = R.timestep_embed(t, 128), R.timestep_embed(t, 128, torch.float32)
    cases.append(("timestep_embed", "five t", r64, r32, None, (1,), {
        "sin and cos halves swapped": torch.cat((r32[:, 128:], r32[:, :128]), dim=1),
        "k / (half - 1)": torch.cat([f(t[:, None] * torch.exp(-math.log(10000.0) * torch.arange(128.0) / 127)[None]) for f in (torch.sin, torch.cos)], dim=1)}))
    # DDIM
    n = 1000
    x, pred = R.randn(70, n), R.randn(71, 2 * n)
    for cname, sa_t, sb_t, sa_p, sb_p in R.ddim_coefficients():
        for g in (1.0, 7.5, 0.0):
            for ptype in (0, 1):
                co = (sa_t, sb_t, sa_p, sb_p)
                r64, r32 = R.ddim_step(x, pred, n, ptype, g, *co), R.ddim_step(x, pred, n, ptype, g, *co, dt=torch.float32)
                u, c = pred[:n], pred[n:]
                m = c + g * (c - u)
                bad_g = sa_p * (sa_t * x - sb_t * m) + sb_p * (sa_t * m + sb_t * x) if ptype == 0 else sa_p * ((x - sb_t * m) / sa_t) + sb_p * m
                m = u + g * (c - u)
                exch = sa_p * (sa_t * m + sb_t * x) + sb_p * (sa_t * x - sb_t * m) if ptype == 0 else sa_p * m + sb_p * ((x - sb_t * m) / sa_t)
                cases.append((f"ddim {'v' if ptype == 0 else 'eps'}", f"{cname} g {g}", r64, r32, None, None,
                              {"guidance c + g (c - u)": bad_g, "x0 and eps exchanged": exch}))
    # clip_preprocess
    mean = torch.tensor(R.CLIP_MEAN)[None, :, None, None]
    std = torch.tensor(R.CLIP_STD)[None, :, None, None]
    for H, W in ((14, 14), (28, 28), (61, 45), (1, 1)):
        img = R.clip_image(2, H, W, 80)
        r64, r32 = R.clip_preprocess(img, 28), R.clip_preprocess(img, 28, torch.float32)
        late = (F.interpolate(img, (28, 28), mode="bilinear", align_corners=False).clamp(0, 1) - mean) / std
        cases.append(("clip_preprocess", f"{H}x{W}", r64, r32, None, None, {
            "align_corners=True": R.clip_preprocess(img, 28, torch.float32, align_corners=True),
            "resized, clamped to [0, 1], then normalised": late}))
    return cases


GATED = _gated_cases()
GATED_OPS = sorted({c[0] for c in GATED})


def test_gated_operations_are_all_there():
    assert GATED_OPS == sorted(["layernorm", "ln_modulate", "softmax", "gelu", "silu", "geglu", "point_embed", "timestep_embed", "ddim v",
                                "ddim eps", "clip_preprocess"])


@pytest.mark.parametrize("op", GATED_OPS)
def test_float32_reference_inside_gate_and_mutants_outside(op):
    worst_ref, caught = 0.0, {}
    for o, name, r64, r32, tol, dims, mutants in GATED:
        if o != op:
            continue
        worst_ref = max(worst_ref, R.check(r32, r64, r32, tol, dims, f"{op} {name} float32 reference"))
        for mname, out in mutants.items():
            finite, r = R.ratio(out, r64, r32, tol, dims)
            caught[mname] = caught.get(mname, False) or (not finite) or r > 1.0
    assert worst_ref <= 1.0 / R.MARGIN + 1e-12
    assert caught and all(caught.values()), f"{op}: mutants inside the gate on every case: {[k for k, v in caught.items() if not v]}"


def test_softmax_padding_left_unwritten_is_seen():
    """the identity half of the softmax test: columns [n_valid, ld_pad) are zero, beyond ld_pad sentinel"""
    s, nv = R.softmax_scores(1, 4, 20, 32, 40, 0, False, 41)
    assert bool((s[..., 20:32] == 70.0).all()) and bool(R.is_sentinel(s[..., 32:]).all())


def test_gate_is_tight_where_arguments_are_small():
    """groups: the timestep rows t <= 1 and the frequency pi have gates near 1e-6, t = 999 and 128 pi near 1e-4 at most"""
    t = torch.tensor([0.0, 0.5, 1.0, 500.0, 999.0])
    g = R.gate_of(R.timestep_embed(t, 128), R.timestep_embed(t, 128, torch.float32), None, (1,)).view(-1)
    assert float(g[:3].max()) < 1e-6 and float(g.max()) < 1e-3
    pts, basis = R.point_cloud(50, 60), R.point_basis()
    g = R.gate_of(R.point_embed(pts, basis, 64), R.point_embed(pts, basis, 64, torch.float32), None, (0,)).view(-1)
    assert float(g[0]) < 2e-6 and float(g[7]) < 1e-3 and float(g[51:].max()) <= 1.5e-45
