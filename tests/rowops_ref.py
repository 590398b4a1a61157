"""Shared pieces of the row / element-wise / K-V scatter kernel tests (tests/test_rowops_ref_cpu.py, tests/test_gpu_rowops.py,
tests/test_gpu_dit_elementwise.py).  Plain torch on the CPU, no device, no library.

For every operation of csrc/k_rowops.h, csrc/k_dit.h and split_rows_f16_kernel:

  ref64   a float64 restatement of the reference project's formula (the file:line each kernel's comment cites), not of the kernel;
  ref32   for the operations that round: the same formula evaluated elementwise in float32 by torch;
  cases   the inputs both test files use (deterministic, built on the CPU);
  mutants float32 / integer emulations of the operation with ONE plausible bug each.  The CPU test shows every mutant outside the
          gate (or identity) on some case - so the case list can see that bug - and ref32 inside it on every case.

Exact operations (a copy, one fp32 add, a rounding to fp16 / e4m3) are compared bit for bit: `bits_equal`.

Gate of the others, from the references alone (as tests/attn_stress_ref.py):
    err <= max(base, MARGIN x e32),   e32 = |ref32 - ref64|,   MARGIN = 4 (another summation / evaluation order)
    base = atol + rtol |ref64| where the project holds a bound for the operation (layernorm 3e-6 / 3e-6, softmax 1e-7 / 1e-5;
           ln_modulate is a layernorm followed by one multiply-add: layernorm's), else one fp32 ulp of |ref64| plus e32.
|ref64| and e32 are maxima over a GROUP of elements - the whole case, or the slices named by `dims` (a row of the timestep embedding, a
frequency of the point embedding): the error of sin(p) comes from the rounding of p, not from the size of sin(p), so a gate per
element would be a gate on where the float32 reference happened to be lucky.  Groups keep the small-argument slices tight (one
timestep <= 1, the frequency pi: a gate near 1e-6) next to the large-argument ones (t = 999, 128 pi: near 1e-4).  LayerNorm-like
outputs are gated in two groups of rows, the hard ones and the rest (check_rows says why not per row)."""
import math
import os
import sys
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref  # noqa: E402

NAN32, NAN16, NAN8 = 0x7FC00123, 0x7E01, 0x7F      # sentinels (tests/test_gpu_gemm_epilogue.py; the byte: e4m3's NaN)
MARGIN = 4.0
TOL_LAYERNORM = (3e-6, 3e-6)
TOL_SOFTMAX = (1e-7, 1e-5)
INF = float("inf")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(seed, *shape):
    return torch.randn(*shape, generator=gen(seed), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ comparing
def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def bits_equal(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def filled(shape, dtype, device="cpu"):
    """A tensor of `dtype` (float32, float16 or uint8) holding the sentinel of its width."""
    ib, v = {torch.float32: (torch.int32, NAN32), torch.float16: (torch.int16, NAN16), torch.uint8: (torch.uint8, NAN8)}[dtype]
    return torch.full(shape, v, dtype=ib, device=device).view(dtype)


def is_sentinel(t):
    """bool tensor: which elements still hold the sentinel of their width."""
    v = {4: NAN32, 2: NAN16, 1: NAN8}[t.element_size()]
    return bits(t) == v


def ulp32(x):
    """The spacing of float32 at |x| (float64 in, float64 out)."""
    a = x.abs().float()
    return (torch.nextafter(a, torch.tensor(INF)) - a).double()


def _group_max(t, dims):
    if dims is None:
        return t.max()
    return t.amax(dim=dims, keepdim=True)


def gate_of(ref64, ref32, tol=None, dims=None):
    """The gate (a scalar, or broadcastable to ref64 when `dims` names the axes a group spans)."""
    ref64 = ref64.double()
    e32 = _group_max((ref32.double() - ref64).abs(), dims)
    mag = _group_max(ref64.abs(), dims)
    base = tol[0] + tol[1] * mag if tol is not None else ulp32(mag) + e32
    return torch.maximum(base, MARGIN * e32)


def ratio(out, ref64, ref32, tol=None, dims=None):
    """(finite, max err / gate) of an output against the two references."""
    out = out.double().cpu()
    err = (out - ref64.double()).abs().nan_to_num(nan=INF)
    return bool(torch.isfinite(out).all()), float((err / gate_of(ref64, ref32, tol, dims)).max())


def check(out, ref64, ref32, tol=None, dims=None, what=""):
    finite, r = ratio(out, ref64, ref32, tol, dims)
    assert finite, f"{what}: NaN or inf in the output"
    assert r <= 1.0, f"{what}: max err / gate = {r:.3f} (gate from ref64 and the float32 reference alone, {MARGIN:g} x its error)"
    return r


# ------------------------------------------------------------------------------------------------ value sweeps
def half_sweep():
    """fp32 values for the fp16 roundings: fp16 numbers (normal, subnormal, the largest), every midpoint between neighbours (ties to
    an even and to an odd mantissa) and the fp32 numbers just below and above it, +-0, 65504, values that round to infinity (65520 is
    the tie).  No NaN and no infinity (their fp16 conversions are exact but `x - hi` of the split would be NaN)."""
    pos = torch.tensor([0x0001, 0x0002, 0x0003, 0x01FF, 0x03FE, 0x03FF, 0x0400, 0x0401, 0x3BFF, 0x3C00, 0x3C01, 0x3C02, 0x4248, 0x57FF,
                        0x7BFE, 0x7BFF], dtype=torch.int16)
    h = pos.view(torch.float16).float()
    nxt = (pos + 1).view(torch.float16).float()
    nxt[-1] = 65536.0                                   # past 65504: the midpoint 65520 rounds to infinity
    mid = 0.5 * (h + nxt)                               # exact in fp32
    inf = torch.tensor(INF)
    extra = torch.tensor([0.0, 2.0 ** -25, 2.0 ** -26, 1e-10, 65519.996, 65536.0, 1e5, 3e38, 0.1, 1.0 / 3.0, math.pi])
    p = torch.cat((h, mid, torch.nextafter(mid, -inf), torch.nextafter(mid, inf), extra))
    return torch.cat((p, -p))


def e4m3_sweep():
    """tests/kv8_ref.py's sweep (every code, every midpoint and its neighbours, subnormals, +-448 and beyond, +-inf) without its NaNs."""
    s = kv8_ref.torch_sweep()
    return s[~torch.isnan(s)]


def trunc_half(x):
    """fp32 -> fp16 by dropping mantissa bits (round toward zero) - the mutant cast."""
    h = x.half()
    over = h.float().abs() > x.abs()
    hb = h.view(torch.int16)
    return torch.where(over, hb - 1, hb).view(torch.float16)          # one fp16 step toward zero (sign-magnitude: same for both signs)


# ------------------------------------------------------------------------------------------------ exact operations
def gather_rows(table, ids):
    return table[torch.as_tensor(ids, dtype=torch.long)]


def add_pos(emb, pos, pos0):
    """emb [B, S, C] + pos[pos0 : pos0 + S]   (modeling_opt.py:355-357)"""
    return emb + pos[pos0:pos0 + emb.shape[1]][None]


def adaln_gate(table, tada, idx):
    """(scale_shift_table[None] + t_adaln).chunk(6)[idx]   (dit.py:127): table [6, C], tada [B, 6, C] -> [B, C]"""
    return table[idx][None] + tada[:, idx]


def adaln_gate_all(tables, tada):
    """[layers, 2, B, C]: gate_msa (chunk 2) and gate_mlp (chunk 5) of every layer"""
    return torch.stack([torch.stack((adaln_gate(t, tada, 2), adaln_gate(t, tada, 5))) for t in tables])


def clip_assemble(patches, cls, pos):
    """cat([class_embedding, patch_embeds]) + position_embedding: patches [B, NP, C], cls [C], pos [NP + 1, C]"""
    B = patches.shape[0]
    return torch.cat((cls[None, None].expand(B, 1, -1), patches), dim=1) + pos[None]


def clip_im2col(px, P, lda):
    """The patch Conv2d's A operand by unfold: px [B, 3, S, S] -> [B * G * G, lda], column c * P * P + ky * P + kx."""
    cols = F.unfold(px, kernel_size=P, stride=P).transpose(1, 2)              # [B, G * G, 3 P P]
    a = cols.reshape(-1, cols.shape[-1])
    return F.pad(a, (0, lda - a.shape[1]))


def im2col_loop(px, P, lda):
    B, _, S, _ = px.shape
    G = S // P
    a = torch.zeros(B * G * G, lda)
    for b in range(B):
        for gy in range(G):
            for gx in range(G):
                a[(b * G + gy) * G + gx, :3 * P * P] = px[b, :, gy * P:(gy + 1) * P, gx * P:(gx + 1) * P].reshape(-1)
    return a


def split_rows(x):
    hi = x.half()
    return hi, (x - hi.float()).half()


def kv_round(v, f8):
    """(what the cache stores, what the scratch keeps) of fp32 values"""
    if f8:
        b = kv8_ref.torch_kv8(v)
        return b, kv8_ref.kv8_decode(b)
    return v.half(), v.half().float()


def kv_scatter(qkv, B, S, hidden, head_dim, l_cap, kv_bstride, f8, guard):
    """qkv [B * S, 3 * hidden] -> (scratch after, kalloc, valloc): the allocations are flat, `guard` sentinel elements, then B rows of
    kv_bstride elements (the cache row [heads, l_cap, head_dim] first), then `guard` more; everything not written is sentinel."""
    H = hidden // head_dim
    dt = torch.uint8 if f8 else torch.float16
    out = qkv.clone()
    allocs = []
    for which in (1, 2):
        v = qkv[:, which * hidden:(which + 1) * hidden]
        stored, kept = kv_round(v, f8)
        out[:, which * hidden:(which + 1) * hidden] = kept
        a = filled((guard + B * kv_bstride + guard,), dt)
        rows = a[guard:guard + B * kv_bstride].view(B, kv_bstride)[:, :H * l_cap * head_dim].view(B, H, l_cap, head_dim)
        rows[:, :, :S] = stored.view(B, S, H, head_dim).permute(0, 2, 1, 3)
        allocs.append(a)
    return out, allocs[0], allocs[1]


# ------------------------------------------------------------------------------------------------ rounding operations
def _ln(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)                         # biased, eps inside the root (nn.LayerNorm)
    return (x - mu) / torch.sqrt(var + eps)


def layernorm(x, w, b, eps, dt=torch.float64):
    return _ln(x.to(dt), eps) * w.to(dt) + b.to(dt)


def ln_modulate(x, rows_per_batch, table, tvec, shift_idx, scale_idx, eps=1e-6, dt=torch.float64):
    """norm(x) * (1 + scale) + shift, (shift, scale) = (table[None] + tvec).chunk(...)   (dit.py:127-132, 190-193).
    x [rows, C]; table [chunks, C]; tvec [B, chunks, C] (the output layer's t_emb[:, None] broadcast over its 2 chunks)."""
    mod = table[None].to(dt) + tvec.to(dt)
    b = torch.arange(x.shape[0]) // rows_per_batch
    return _ln(x.to(dt), eps) * (1 + mod[b, scale_idx]) + mod[b, shift_idx]


def softmax_rows(s, n_valid, dt=torch.float64):
    """softmax over the first n_valid[r] columns of row r, zeros after: s [..., rows, cols], n_valid [rows]"""
    cols = s.shape[-1]
    vis = torch.arange(cols)[None] < n_valid[:, None]
    x = s.to(dt).masked_fill(~vis, -INF)
    if dt == torch.float64:
        return torch.softmax(x, -1)
    p = torch.exp(x - x.max(-1, keepdim=True).values)
    return p / p.sum(-1, keepdim=True)


def gelu(x, dt=torch.float64):
    """F.gelu (erf form).  float64: through erfc, which keeps its accuracy in the negative tail."""
    x = x.to(dt)
    if dt == torch.float64:
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    return x * 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))


def geglu(u, dt=torch.float64):
    """x, gates = u.chunk(2, -1); x * gelu(gates)   (point.py:68-71)"""
    x, g = u.to(dt).chunk(2, dim=-1)
    return x * gelu(g, dt)


def silu(x, dt=torch.float64):
    x = x.to(dt)
    return x / (1.0 + torch.exp(-x))


def point_basis(n_freq=8):
    """PointEmbed's basis [3, 3 * n_freq]: 2^k pi on the block of its own axis (point.py:43-49)"""
    e = torch.pow(2, torch.arange(n_freq)).float() * math.pi
    z = torch.zeros(n_freq)
    return torch.stack([torch.cat([e, z, z]), torch.cat([z, e, z]), torch.cat([z, z, e])])


def point_embed(pts, basis, ldo, dt=torch.float64):
    """cat([sin(p), cos(p), xyz]), p = einsum('nd,de->ne', pts, basis), zero-padded to ldo   (point.py:53-63)"""
    p = (pts.to(dt)[:, :, None] * basis.to(dt)[None]).sum(1)
    out = torch.cat((p.sin(), p.cos(), pts.to(dt)), dim=1)
    return F.pad(out, (0, ldo - out.shape[1]))


def timestep_embed(t, half, dt=torch.float64):
    """Timesteps(2 * half): [sin(t w_k), cos(t w_k)], w_k = exp(-ln(10000) k / half)   (dit.py:52-66)"""
    k = torch.arange(half, dtype=dt)
    if dt == torch.float64:
        w = torch.exp(-math.log(10000.0) * k / half)
    else:
        w = torch.exp((-math.log(10000.0) * k) / half)                  # the reference's fp32 steps
    a = t.to(dt)[:, None] * w[None]
    return torch.cat((a.sin(), a.cos()), dim=-1)


def ddim_step(x, pred, n, pred_type, g, sa_t, sb_t, sa_p, sb_p, dt=torch.float64):
    """models_dit.py:222-227 + DDIMScheduler.step (eta 0): pred [2 n] = uncond | cond; the coefficients are the fp32 numbers the
    sampler passes.  pred_type 0: v-prediction, 1: epsilon."""
    x, u, c = x.to(dt), pred[:n].to(dt), pred[n:].to(dt)
    co = [torch.tensor(v, dtype=torch.float32).to(dt) for v in (g, sa_t, sb_t, sa_p, sb_p)]
    g, sa_t, sb_t, sa_p, sb_p = co
    m = u + g * (c - u)
    if pred_type == 0:
        x0, eps = sa_t * x - sb_t * m, sa_t * m + sb_t * x
    else:
        x0, eps = (x - sb_t * m) / sa_t, m
    return sa_p * x0 + sb_p * eps


def ddim_coefficients():
    """[(name, sa_t, sb_t, sa_p, sb_p)] at the first, a middle and the last step of the 6- and the 50-step schedule (the scheduler
    restatement of oracle/arae_oracle.py that tests/test_oracle_golden.py pins); roots taken in fp32 as the sampler takes them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.join(root, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(root, "oracle"))
    import arae_oracle as O
    out = []
    for steps in (6, 50):
        ts, ac, final = O.ddim_schedule(steps)
        ratio = 1000 // steps
        for i in (0, steps // 2, steps - 1):
            t = ts[i]
            a_t, a_p = ac[t], (ac[t - ratio] if t - ratio >= 0 else final)
            out.append((f"{steps}steps_t{t}", float(a_t.sqrt()), float((1 - a_t).sqrt()), float(a_p.sqrt()), float((1 - a_p).sqrt())))
    return out


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_preprocess(img, OUT, dt=torch.float64, align_corners=False):
    """TF.normalize(mean, std) then F.interpolate(bilinear, align_corners=False)   (models_dit.py:108-109)"""
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32).to(dt)[None, :, None, None]
    std = torch.tensor(CLIP_STD, dtype=torch.float32).to(dt)[None, :, None, None]
    return F.interpolate((img.to(dt) - mean) / std, (OUT, OUT), mode="bilinear", align_corners=align_corners, antialias=False)


# ------------------------------------------------------------------------------------------------ cases
def ew_values(n, seed):
    """n values for gelu / silu / geglu gates: a grid over [-20, 20], +-0, fp32 subnormals, +-88, N(0, 1) for the rest"""
    grid = torch.linspace(-20.0, 20.0, 4001)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 88.0, -88.0, 87.5, -87.5])
    v = torch.cat((grid, special))
    assert n >= v.numel()
    return torch.cat((v, randn(seed, n - v.numel())))


def layernorm_rows(rows, cols, seed):
    """x [rows, cols] and the row lists (const, hard): N(0, 1) rows with the hard ones at rows 1 .. 3 k (k = 32 of each kind from 200
    rows up, else 1; none below 5 rows): mean 1000 with unit spread; spread 1e-3 around 0.3; one column at 1e4.  Two constant rows
    (0.5 and -3) follow: their output is b bit for bit."""
    x = randn(seed, rows, cols)
    const, hard = [], []
    if rows >= 5:
        k = 32 if rows >= 200 else 1
        for i in range(k):
            x[1 + 3 * i] = 1000.0 + x[1 + 3 * i]
            x[2 + 3 * i] = 0.3 + 1e-3 * x[2 + 3 * i]
            x[3 + 3 * i, (cols // 3 + 7 * i) % cols] = 1e4
        hard = list(range(1, 3 * k + 1))
        x[3 * k + 1] = 0.5
        x[rows - 1] = -3.0
        const = [3 * k + 1, rows - 1]
    return x, const, hard


def check_rows(out, ref64, ref32, hard, tol, what):
    """The gate of a LayerNorm-like output [rows, cols] in two groups, each gated as one case: the hard rows and the others.  (Not per
    row: a row's error is dominated by ONE rounding, that of its mean - a mean off by one fp32 ulp moves the whole row by
    ulp(mean) x rstd - so the float32 reference's error on a single row is a sample of one, and a gate from it a gate on its luck.)
    -> the larger err / gate"""
    sel = torch.zeros(out.shape[0], dtype=torch.bool)
    sel[hard] = True
    r = 0.0
    for name, m in (("plain rows", ~sel), ("hard rows", sel)):
        if bool(m.any()):
            r = max(r, check(out[m], ref64[m], ref32[m], tol, None, f"{what}, {name}"))
    return r


def ln_mod_case(rows, rows_per_batch, layout, seed, C=1024):
    """layout "layer": table [6, C], tvec = t_adaln [B, 6, C], (shift, scale) indices (0, 1) and (3, 4); "out": table [2, C],
    tvec = t_emb [B, C] shared by both chunks (t_cstride 0), indices (0, 1).  Table and tvec sit in allocations whose other rows
    are NaN: `table_alloc` [chunks + 2, C] (rows 1 .. chunks live), `tvec_alloc` [B + 2, chunks or 1, C] (rows 1 .. B live)."""
    B = rows // rows_per_batch
    chunks = 6 if layout == "layer" else 2
    x, _, hard = layernorm_rows(rows, C, seed)
    table_alloc = torch.full((chunks + 2, C), float("nan"))
    table_alloc[1:chunks + 1] = 0.5 * randn(seed + 1, chunks, C)
    tv_chunks = chunks if layout == "layer" else 1
    tvec_alloc = torch.full((B + 2, tv_chunks, C), float("nan"))
    tvec_alloc[1:B + 1] = 0.5 * randn(seed + 2, B, tv_chunks, C)
    table, tv = table_alloc[1:chunks + 1], tvec_alloc[1:B + 1]
    tvec = tv if layout == "layer" else tv.expand(B, 2, C)
    return NS(x=x, hard=hard, rows=rows, rpb=rows_per_batch, B=B, C=C, table=table, tvec=tvec, table_alloc=table_alloc, tvec_alloc=tvec_alloc,
              t_bstride=tv_chunks * C, t_cstride=C if layout == "layer" else 0,
              idx=[(0, 1), (3, 4)] if layout == "layer" else [(0, 1)])


def point_cloud(M, seed):
    """points in [-1, 1] with exactly 0 and +-1 among them"""
    p = torch.rand(M, 3, generator=gen(seed)) * 2 - 1
    edge = torch.tensor([[0.0, 0.0, 0.0], [1.0, -1.0, 0.0], [-1.0, 1.0, 1.0], [0.0, 1.0, -1.0]])
    p[:min(M, 4)] = edge[:min(M, 4)]
    return p


def clip_image(B, H, W, seed):
    """images with values a little outside [0, 1] as well (a clamp anywhere on the way would show)"""
    return torch.rand(B, 3, H, W, generator=gen(seed)) * 1.4 - 0.2


SOFTMAX_ROW_PROFILES = ("offset_hi", "offset_lo", "spike_last", "rising")      # the hidden columns hold the masked spike


def softmax_scores(batch, rows, cols, ld_pad, ld, causal_off, causal, seed):
    """[batch, rows, ld] scores: tests/attn_stress_ref.py's row profiles over the valid columns, +60 in the causally hidden ones, +70
    in the padding [cols, ld_pad), sentinels beyond ld_pad.  n_valid [rows]."""
    import attn_stress_ref as A
    g = gen(seed)
    n_valid = torch.tensor([min(cols, r + 1 + causal_off) if causal else cols for r in range(rows)])
    s = filled((batch, rows, ld), torch.float32)
    for b in range(batch):
        for r in range(rows):
            n = int(n_valid[r])
            s[b, r, :n] = A.profile(SOFTMAX_ROW_PROFILES[(r + b) % 4], n, g).float()
            s[b, r, n:cols] = 60.0
            s[b, r, cols:ld_pad] = 70.0
    return s, n_valid
