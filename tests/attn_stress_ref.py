"""Shared pieces of the attention stress tests (tests/test_attn_stress_cpu.py, tests/test_gpu_attn_stress.py).  Plain torch, no device,
no library.

Every other attention test draws q, K and V from N(0, 1): the scores then have unit variance, no exp ever under- or overflows, and a
kernel that forgot to subtract the maximum would pass.  Here the SCORES are prescribed:

  profile      target scores (after / sqrt(D))           aimed at
  offset_hi    90 + N(0, 1)                               max subtraction: exp overflows without it
  offset_lo    -110 + N(0, 1)                             the same from below: every weight 0, the row 0 / 0
  rising       linspace(-60, 60, n)                       every chunk / tile / pass meets a new maximum; earlier mass is rescaled to nothing
  falling      linspace(60, -60, n)                       the first chunk holds all mass; later partials' l underflows against it
  spike_first  key 0 at +50, the rest -50                 the output is that key's V row
  spike_last   key n - 1 at +50, the rest -50             the same in the ragged tail
  two_spikes   keys 0 and n - 1 at +40, the rest -40      two partials / waves / tiles of equal weight far apart
  flat_tail    key 0 at +10, the rest 0                   an attention sink: the tail's mass n e^-10 is comparable to the spike's
  dead_chunks  +-60 + N(0, 1), sign flips every 128 keys  whole chunks or waves whose mass is exactly 0 in fp32 next to live ones
  zero_q       q = 0                                      all scores exactly 0: the output is the mean of the valid V rows
  masked_spike key j* at +60, the rest -60 + N(0, 1)      (causal forms) the largest score is masked for the first half of the queries

Constructors.  Decode: q ~ N(0, 1), k_j = s_j sqrt(D) q / |q|^2 + 0.05 N(0, 1), v ~ N(0, 1), rounded to the cache type; flash: rank one
plus noise, q_i = a_i u, k_j = b_j sqrt(D) u / |u|^2 + 0.05 N(0, 1), a cycling over {1, -1, 0.25, 0}.  The references are computed on
the STORED values, so a profile need not be hit exactly; everything is finite.

References: ref64 (float64 softmax attention) and plain32 (the same in float32 by elementwise multiply-and-sum, no library GEMM).

Gate: out has no NaN / inf and max|out - ref64| <= max(atol + rtol max|ref64|, 4 max|plain32 - ref64|), atol / rtol those of the same
kernel's N(0, 1) parity test.  The second term is what fp32 itself costs on these inputs (a score near 100 carries an absolute error
near 100 x 2^-24 x a few, and exp turns it into a relative error of the weight), times 4 for a different summation order.  The gate
never looks at the kernel.

The module also holds an fp32 emulation of the chunked online softmax the kernels implement (emulate) with its mutants: the CPU test
shows that the emulation is inside the gate, that every mutant is outside it on some profile, and that `no_max` is invisible to
N(0, 1) scores."""
import math
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref  # noqa: E402

PROFILES = ("offset_hi", "offset_lo", "rising", "falling", "spike_first", "spike_last", "two_spikes", "flat_tail", "dead_chunks", "zero_q")
FLASH_PROFILES = PROFILES[:-1]          # a = 0 is the flash form of zero_q
DEAD_PERIOD = 128
Q_CYCLE = (1.0, -1.0, 0.25, 0.0)
NOISE = 0.05

# atol, rtol of each kernel's N(0, 1) parity test (tests/test_gpu_kernels.py, test_gpu_kv8.py, test_gpu_attn_shared*.py)
TOL_DECODE = (2e-6, 1e-5)
TOL_OUTPROJ3 = (2e-5, 1e-5)
TOL_SHARED = (2e-6, 1e-5)
TOL_FLASH32 = (5e-6, 2e-5)
TOL_FLASH16S = (3e-6, 1e-5)
TOL_FLASH16 = (4e-3, 4e-3)
TOL_SOFTMAX = (1e-7, 1e-5)
MARGIN = 4.0                            # over the fp32 reference's own error: a different summation order


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ profiles
def spike_keys(name, n, n_queries=None):
    """The keys a spike profile puts its large score on ([] for the others).  masked_spike: j* = (M - N) + N // 2 with M = n keys and
    N = n_queries (default n) - masked for queries i < N // 2 under the causal rule j <= i + (M - N)."""
    if name == "spike_first":
        return [0]
    if name == "spike_last":
        return [n - 1]
    if name == "two_spikes":
        return sorted({0, n - 1})
    if name == "flat_tail":
        return [0]
    if name == "masked_spike":
        N = n if n_queries is None else n_queries
        return [(n - N) + N // 2]
    return []


def profile(name, n, g, n_queries=None):
    """Target scores s[0 .. n) of a profile, float64 (zero_q: zeros - the constructor zeroes q instead)."""
    j = torch.arange(n)
    if name == "offset_hi":
        return 90.0 + randn(g, n)
    if name == "offset_lo":
        return -110.0 + randn(g, n)
    if name == "rising":
        return torch.linspace(-60.0, 60.0, n, dtype=torch.float64)
    if name == "falling":
        return torch.linspace(60.0, -60.0, n, dtype=torch.float64)
    if name in ("spike_first", "spike_last", "two_spikes", "flat_tail", "masked_spike"):
        hi, lo = {"spike_first": (50.0, -50.0), "spike_last": (50.0, -50.0), "two_spikes": (40.0, -40.0), "flat_tail": (10.0, 0.0),
                  "masked_spike": (60.0, -60.0)}[name]
        s = torch.full((n,), lo, dtype=torch.float64)
        if name == "masked_spike":
            s = s + randn(g, n)
        s[spike_keys(name, n, n_queries)] = hi
        return s
    if name == "dead_chunks":
        sign = 1.0 - 2.0 * ((j // DEAD_PERIOD) % 2).double()
        return 60.0 * sign + randn(g, n)
    if name == "zero_q":
        return torch.zeros(n, dtype=torch.float64)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ cache types
def to_cache(x, cache):
    """fp32 values -> the cache's storage: "f32" as they are, "f16" .half(), "kv8" the e4m3 bytes of kv8_ref.torch_kv8."""
    x = x.float()
    if cache == "f32":
        return x
    if cache == "f16":
        return x.half()
    if cache == "kv8":
        return kv8_ref.torch_kv8(x)
    raise ValueError(cache)


def from_cache(c):
    """The values a cache tensor stores, float32."""
    return kv8_ref.kv8_decode(c) if c.dtype == torch.uint8 else c.float()


def poison(c, start, odd=False):
    """The unused tail c[..., start:, :] as the parity tests poison it: NaN, or the NaN bytes 0x7F / 0xFF."""
    if c.dtype == torch.uint8:
        c[..., start:, :] = 0xFF if odd else 0x7F
    else:
        c[..., start:, :] = float("nan")


# ------------------------------------------------------------------------------------------------ references
def ref64(q, k, v, visible=None):
    """float64 softmax(q k^T / sqrt(D)) v.  q [..., N, D], k / v [..., M, D], visible bool [..., N, M] or None -> [..., N, D] float64."""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if visible is not None:
        s = s.masked_fill(~visible, float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def plain32(q, k, v, visible=None, max_elems=1 << 25):
    """The same in float32, by elementwise multiply and sum (no GEMM, so no reduced-precision matmul path can enter); the leading
    dimensions are walked in slices of at most max_elems products."""
    q, k, v = q.float(), k.float(), v.float()
    lead = q.shape[:-2]
    N, D, M = q.shape[-2], q.shape[-1], k.shape[-2]
    qf, kf, vf = q.reshape(-1, N, D), k.reshape(-1, M, D), v.reshape(-1, M, D)
    vis = None if visible is None else visible.expand(*lead, N, M).reshape(-1, N, M)
    out = torch.empty_like(qf)
    step = max(1, max_elems // (N * M * D))
    c = torch.tensor(math.sqrt(D), dtype=torch.float32)
    for i in range(0, qf.shape[0], step):
        sl = slice(i, i + step)
        s = (qf[sl, :, None, :] * kf[sl, None, :, :]).sum(-1) / c
        if vis is not None:
            s = s.masked_fill(~vis[sl], float("-inf"))
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        o = (p[..., None] * vf[sl, None, :, :]).sum(-2)
        out[sl] = o / p.sum(-1, keepdim=True)
    return out.reshape(*lead, N, D)


# ------------------------------------------------------------------------------------------------ the gate
def gate_of(ref, p32, atol, rtol):
    ref = ref.double().cpu()
    return max(atol + rtol * float(ref.abs().max()), MARGIN * float((p32.double().cpu() - ref).abs().max()))


def ratio(out, ref, p32, atol, rtol):
    """(finite, err / gate) of an output against the two references; the gate is computed from the references alone."""
    out = out.double().cpu()
    finite = bool(torch.isfinite(out).all())
    err = float((out - ref.double().cpu()).abs().nan_to_num(nan=float("inf")).max())
    return finite, err / gate_of(ref, p32, atol, rtol)


def check(out, ref, p32, atol, rtol, what=""):
    """Asserts the gate and returns err / gate."""
    finite, r = ratio(out, ref, p32, atol, rtol)
    assert finite, f"{what}: NaN or inf in the output"
    assert r <= 1.0, f"{what}: max|out - ref64| = {r * gate_of(ref, p32, atol, rtol):.3e} is {r:.2f} x the gate " \
                     f"{gate_of(ref, p32, atol, rtol):.3e} (atol {atol:g}, rtol {rtol:g}, {MARGIN:g} x plain32's own error " \
                     f"{float((p32.double().cpu() - ref.double().cpu()).abs().max()):.3e})"
    return r


def fp32_score_bound(q, k, v):
    """The rigorous worst case of an fp32 kernel on one query: with delta = (D + 2) 2^-24 max_j sum_i |q_i k_ji| / sqrt(D) every weight
    is off by at most a factor e^(+-delta), so an output element moves by at most (e^(2 delta) - 1)(max_j v_jd - min_j v_jd).
    q [D], k / v [n, D] (stored values) -> float."""
    q, k, v = q.double(), k.double(), v.double()
    D = q.shape[-1]
    delta = (D + 2) * 2.0 ** -24 * float((q.abs() * k.abs()).sum(-1).max()) / math.sqrt(D)
    return math.expm1(2 * delta) * float((v.max(0).values - v.min(0).values).max())


def p16_bound(q, k, v, visible=None):
    """What rounding P to fp16 costs at most (the fp16-P flash kernels): sum_j max(2^-11 p_j, 2^-25)(|v_jd| + |o_d|) / l with p
    relative to the row maximum, in float64 -> [..., N, D]."""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if visible is not None:
        s = s.masked_fill(~visible, float("-inf"))
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    l = p.sum(-1, keepdim=True)
    o = (p @ v) / l
    e = torch.maximum(p * 2.0 ** -11, torch.full_like(p, 2.0 ** -25))
    if visible is not None:
        e = e * visible
    return (e @ v.abs() + e.sum(-1, keepdim=True) * o.abs()) / l


# ------------------------------------------------------------------------------------------------ decode constructor
def keys_for(s, q, g):
    """k_j = s_j sqrt(D) q / |q|^2 + NOISE N(0, 1) for q [H, D], s [H, n] -> [H, n, D] float64 (q = 0: plain N(0, 1) keys)."""
    H, D = q.shape
    n = s.shape[1]
    q = q.double()
    noise = randn(g, H, n, D)
    q2 = (q * q).sum(-1, keepdim=True)
    if float(q2.min()) == 0.0:
        return noise
    return s[:, :, None] * math.sqrt(D) * (q / q2)[:, None, :] + NOISE * noise


def decode_row(name, n, H, D, cache, g, q=None, scale=1.0):
    """One batch row: (q [H, D] fp32, k, v [H, n, D] in the cache's storage).  q given: the keys are built for it; scale multiplies the
    target scores."""
    if q is None:
        q = randn(g, H, D).float()
        if name == "zero_q":
            q = torch.zeros(H, D)
    s = torch.stack([profile(name, n, g) for _ in range(H)]) * scale
    k = keys_for(s, q, g)
    v = randn(g, H, n, D)
    return q, to_cache(k, cache), to_cache(v, cache)


def row_expect(name, v_stored):
    """What a zero_q or spike_first / spike_last row must give, from the stored V rows [H, n, D]: float64 [H, D] or None."""
    v = v_stored.double()
    if name == "zero_q":
        return v.mean(1)
    if name == "spike_first":
        return v[:, 0]
    if name == "spike_last":
        return v[:, -1]
    return None


def decode_case(names, lens, H, D, cache, seed=0):
    """A decode batch with profile names[b] over lens[b] keys in row b: q [B, H * D] fp32, caches [B, H, Lcap, D] with the unused tail
    poisoned, ref64 / plain32 [B, H * D] on the stored values, expect[b] (row_expect)."""
    g = gen(seed)
    B = len(names)
    Lcap = (max(lens) + 63) // 64 * 64
    dt = {"f32": torch.float32, "f16": torch.float16, "kv8": torch.uint8}[cache]
    kc, vc = torch.zeros(B, H, Lcap, D, dtype=dt), torch.zeros(B, H, Lcap, D, dtype=dt)
    qs, r64, p32, expect = [], [], [], []
    for b, (name, n) in enumerate(zip(names, lens)):
        q, k, v = decode_row(name, n, H, D, cache, g)
        kc[b, :, :n], vc[b, :, :n] = k, v
        ks, vs = from_cache(k), from_cache(v)
        assert bool(torch.isfinite(ks).all()) and bool(torch.isfinite(vs).all())
        r64.append(ref64(q[:, None, :], ks, vs).reshape(H * D))
        p32.append(plain32(q[:, None, :], ks, vs).reshape(H * D))
        expect.append(None if row_expect(name, vs) is None else row_expect(name, vs).reshape(H * D))
        qs.append(q.reshape(H * D))
        poison(kc[b], n)
        poison(vc[b], n, odd=bool(b % 2))
    return SimpleNamespace(q=torch.stack(qs), kc=kc, vc=vc, lens=list(lens), names=list(names), ref64=torch.stack(r64), plain32=torch.stack(p32),
                           expect=expect, H=H, D=D, Lcap=Lcap)


# ------------------------------------------------------------------------------------------------ flash constructor
def causal_visible(N, M):
    """bool [N, M]: key j is visible to query i iff j <= i + (M - N)."""
    return torch.arange(M)[None, :] <= torch.arange(N)[:, None] + (M - N)


def flash_case(names, B, H, N, M, D, causal, seed=0, rounding="none"):
    """Packed q [B, N, H * D], k / v [B, M, H * D] fp32 with profile names[(b * H + h) % len(names)] over the keys of slot (b, h) and
    a = Q_CYCLE[i % 4] over the queries; rounding: "none", "kv16" (k, v fp16-valued) or "qkv16" (q too).  ref64 / plain32 [B, H, N, D],
    visible (bool [N, M] or None), a [N], slot_names[b][h]."""
    g = gen(seed)
    a = torch.tensor(Q_CYCLE, dtype=torch.float64)[torch.arange(N) % 4]
    q = torch.zeros(B, H, N, D, dtype=torch.float64)
    k, v = torch.zeros(B, H, M, D, dtype=torch.float64), torch.zeros(B, H, M, D, dtype=torch.float64)
    slot_names = [[names[(b * H + h) % len(names)] for h in range(H)] for b in range(B)]
    for b in range(B):
        for h in range(H):
            u = randn(g, D)
            q[b, h] = a[:, None] * u
            s = profile(slot_names[b][h], M, g, n_queries=N)
            k[b, h] = s[:, None] * math.sqrt(D) * (u / (u * u).sum()) + NOISE * randn(g, M, D)
            v[b, h] = randn(g, M, D)
    q, k, v = q.float(), k.float(), v.float()
    if rounding in ("kv16", "qkv16"):
        k, v = k.half().float(), v.half().float()
    if rounding == "qkv16":
        q = q.half().float()
    assert bool(torch.isfinite(k).all()) and bool(torch.isfinite(q).all())
    visible = causal_visible(N, M) if causal else None
    pack = lambda t: t.transpose(1, 2).reshape(B, t.shape[2], H * D).contiguous()
    return SimpleNamespace(q=pack(q), k=pack(k), v=pack(v), qh=q, kh=k, vh=v, ref64=ref64(q, k, v, visible), plain32=plain32(q, k, v, visible),
                           visible=visible, a=a, slot_names=slot_names, B=B, H=H, N=N, M=M, D=D, causal=causal)


def unpack(o, H):
    """packed [B, N, H * D] -> [B, H, N, D]"""
    B, N, HD = o.shape
    return o.reshape(B, N, H, HD // H).transpose(1, 2)


def flash_uniform_rows(c):
    """The a = 0 queries of a flash case: (row index tensor, float64 mean of each one's visible V rows [B, H, rows, D])."""
    rows = (c.a == 0).nonzero().flatten()
    vis = torch.ones(c.N, c.M, dtype=torch.bool) if c.visible is None else c.visible
    w = vis[rows].double()
    return rows, (w / w.sum(-1, keepdim=True)) @ c.vh.double()


# ------------------------------------------------------------------------------------------------ softmax rows
SOFTMAX_PROFILES = ("offset_hi", "offset_lo", "spike_last", "masked_spike")


def softmax_case(rows, cols, ld, causal, seed=0):
    """Score rows [rows, ld] fp32 for the in-place row softmax: row i holds SOFTMAX_PROFILES[i % 4] over its valid columns (i + 1 when
    causal, else cols); masked_spike rows hold -60 + N(0, 1) there and +60 in EVERY column the kernel must ignore (the causal upper
    triangle), and every row holds +70 in the padding columns [cols, ld).  ref64 / plain32 [rows, cols] with zeros where masked."""
    g = gen(seed)
    s = torch.zeros(rows, ld, dtype=torch.float64)
    valid = torch.zeros(rows, cols, dtype=torch.bool)
    for i in range(rows):
        n = min(i + 1, cols) if causal else cols
        name = SOFTMAX_PROFILES[i % 4]
        valid[i, :n] = True
        if name == "masked_spike":
            s[i, :n] = -60.0 + randn(g, n)
            s[i, n:cols] = 60.0
        else:
            s[i, :n] = profile(name, n, g)
            s[i, n:cols] = randn(g, cols - n)
        s[i, cols:] = 70.0
    s = s.float()
    x = s[:, :cols].double().masked_fill(~valid, float("-inf"))
    r64 = torch.softmax(x, dim=-1)
    x32 = s[:, :cols].masked_fill(~valid, float("-inf"))
    p = torch.exp(x32 - x32.max(dim=-1, keepdim=True).values)
    return SimpleNamespace(s=s, valid=valid, ref64=r64, plain32=p / p.sum(-1, keepdim=True))


# ------------------------------------------------------------------------------------------------ the emulation and its mutants
MUTANTS = ("no_max", "merge_w1", "drop_last", "double_count", "skip_rescale", "mask_after_max", "empty_nan")
NEG_INF = float("-inf")
EMU_WAVES, EMU_BLOCK, EMU_PASS = 4, 32, 64


def _f(x):
    return torch.tensor(x, dtype=torch.float32)


def emulate(q, k, v, chunk=128, mutant=None, visible=None):
    """fp32 emulation of the chunked online softmax for one query: q [D], k / v [n, D] (stored values, fp32), visible bool [n] or None.

    The keys are cut into chunks of `chunk`; a chunk's 32-key blocks are dealt to four waves (block i to wave i % 4), a wave walks its
    blocks with a running maximum and the alpha = exp(m_run - m_new) rescale, the four waves of a chunk are merged into one partial
    {m, l, o} with weights exp(m_wave - M) (0 for a wave that saw no key), and the partials are merged in passes of 64 with a running
    M_run.  One more chunk than the keys need is walked - it holds no key, as a chunk of a 15-key row cut into 16 or a grid sized by
    the cache's capacity does - so the guards for m = -inf are on the path of every call.

    mutant: None or one of MUTANTS -
      no_max          no max subtraction anywhere (every m is 0)
      merge_w1        merge weights forced to 1
      drop_last       the last key is dropped
      double_count    key n // 2 is counted twice in l
      skip_rescale    alpha = 1 when a block brings a new maximum
      mask_after_max  the maximum is taken over masked keys too (the mask only zeroes the weights)
      empty_nan       an empty partial is merged as exp(-inf - (-inf))"""
    assert mutant is None or mutant in MUTANTS
    q, k, v = q.float(), k.float(), v.float()
    n, D = k.shape
    s_all = (k * q[None, :]).sum(-1) / _f(math.sqrt(D))
    vis = torch.ones(n, dtype=torch.bool) if visible is None else visible.clone()
    if mutant == "drop_last":
        vis[int(vis.nonzero()[-1])] = False
    twice = n // 2
    no_max = mutant == "no_max"
    parts = []                                                 # (m, l, o[D]) per chunk
    for c0 in range(0, (n + chunk - 1) // chunk * chunk + chunk, chunk):
        waves = []
        for w in range(EMU_WAVES):
            m_run, l_run, o_run = _f(NEG_INF), _f(0.0), torch.zeros(D)
            for b0 in range(c0 + w * EMU_BLOCK, min(c0 + chunk, n), EMU_WAVES * EMU_BLOCK):
                b1 = min(b0 + EMU_BLOCK, c0 + chunk, n)
                ok = vis[b0:b1]
                s = s_all[b0:b1]
                sm = s if mutant == "mask_after_max" else s.masked_fill(~ok, NEG_INF)
                m_new = torch.maximum(m_run, sm.max())
                if no_max:
                    m_new = _f(0.0) if bool(ok.any()) else m_run
                if m_new == NEG_INF:
                    continue                                   # nothing visible yet
                alpha = _f(0.0) if m_run == NEG_INF else torch.exp(m_run - m_new)
                if mutant == "skip_rescale" and m_run != NEG_INF and m_new > m_run:
                    alpha = _f(1.0)
                p = torch.where(ok, torch.exp(s - m_new), _f(0.0))
                psum = p.sum()
                if b0 <= twice < b1 and mutant == "double_count":
                    psum = psum + p[twice - b0]
                l_run = l_run * alpha + psum
                o_run = o_run * alpha + (p[:, None] * v[b0:b1]).sum(0)
                m_run = m_new
            waves.append((m_run, l_run, o_run))
        M = torch.stack([m for m, _, _ in waves]).max()
        l_c, o_c = _f(0.0), torch.zeros(D)
        for m_w, l_w, o_w in waves:
            if mutant == "empty_nan":
                wgt = torch.exp(m_w - M)                       # exp(-inf - (-inf)) = NaN in a chunk without keys
            elif mutant == "merge_w1":
                wgt = _f(1.0)
            else:
                wgt = _f(0.0) if m_w == NEG_INF else torch.exp(m_w - M)
            l_c = l_c + l_w * wgt
            o_c = o_c + o_w * wgt
        parts.append((M, l_c, o_c))
    M_run, l_run, o_run = _f(NEG_INF), _f(0.0), torch.zeros(D)
    for p0 in range(0, len(parts), EMU_PASS):
        ms = torch.stack([m for m, _, _ in parts[p0:p0 + EMU_PASS]])
        ls = torch.stack([l for _, l, _ in parts[p0:p0 + EMU_PASS]])
        os_ = torch.stack([o for _, _, o in parts[p0:p0 + EMU_PASS]])
        M_new = torch.maximum(M_run, ms.max())
        if mutant == "empty_nan":
            wgt = torch.exp(ms - M_new)
            alpha = torch.exp(M_run - M_new) if p0 else _f(0.0)
        elif mutant == "merge_w1":
            wgt, alpha = torch.ones_like(ms), _f(1.0)
        else:
            wgt = torch.where(ms == NEG_INF, _f(0.0), torch.exp(ms - M_new))
            alpha = _f(0.0) if M_run == NEG_INF else torch.exp(M_run - M_new)
        l_run = l_run * alpha + (ls * wgt).sum()
        o_run = o_run * alpha + (os_ * wgt[:, None]).sum(0)
        M_run = M_new
    return o_run / l_run
