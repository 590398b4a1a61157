"""The rows route of the prefill with a past (csrc/k_attn_extend.h: attn_extend_kernel + attn_extend_merge_kernel) alone, through its unit
entry ``er_k_attn_extend``: n_new queries per row behind past_len cached positions, query t over keys [0, past_len + t] of its own row.

Reference: ``attn_stress_ref.ref64`` on the DEQUANTISED stored values with the visible mask "key <= past_len + t"; gate:
``attn_stress_ref.check`` with ``TOL_SHARED`` - the gate the shared-prefix kernels are held to, whose margin is over the fp32 reference's
own error (``plain32``) and never looks at the kernel.  Every case runs on the fp32, the fp16 and the e4m3 byte cache and prints its worst
err / gate ratio.  The cache handed to the entry is a window of a larger allocation: the rows in front of and behind it and every position
>= past_len + n_new hold NaN, and the output sits between sentinel guards.

Shapes: 3 heads (the head only indexes; an odd count keeps the slices unequal) of 96, the smallest at which the code can go wrong -
past_len around the 128-key chunk and far behind it, n_new 1, 2, 3 and 32 and the route threshold of csrc/er_extend_plan.h with its
predecessor, totals exactly on, one short of and one past a chunk boundary."""
import ctypes as C
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_stress_ref as asr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, D = 3, 96
CACHES = ("f32", "f16", "kv8")
GUARD = 1024
SENTINEL = -777.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def threshold():
    src = open(os.path.join(ROOT, "edgerunner_amd", "csrc", "er_extend_plan.h")).read()
    return int(re.search(r"constexpr int EXTEND_ROWS_MAX_NEW = (\d+);", src).group(1))


THR = threshold()


def build(B, past, n_new, cache, seed, names=None, head_dim=D):
    """q [B, n_new, H * head_dim] fp32, stored K / V [B, H, total, head_dim] in the cache's type, ref64 / plain32 [B, H, n_new, head_dim] on the
    stored values.  names None: N(0, 1) draws; else the rank-one construction of attn_stress_ref.flash_case with profile
    names[(b * H + h) % len(names)] over the keys of slot (b, h) and a cycling over {1, -1, 0.25, 0} over the queries."""
    g = asr.gen(seed)
    total = past + n_new
    if names is None:
        q, k, v = asr.randn(g, B, H, n_new, head_dim), asr.randn(g, B, H, total, head_dim), asr.randn(g, B, H, total, head_dim)
    else:
        a = torch.tensor(asr.Q_CYCLE, dtype=torch.float64)[torch.arange(n_new) % 4]
        q = torch.zeros(B, H, n_new, head_dim, dtype=torch.float64)
        k, v = torch.zeros(B, H, total, head_dim, dtype=torch.float64), torch.zeros(B, H, total, head_dim, dtype=torch.float64)
        for b in range(B):
            for h in range(H):
                u = asr.randn(g, head_dim)
                q[b, h] = a[:, None] * u
                s = asr.profile(names[(b * H + h) % len(names)], total, g, n_queries=n_new)
                k[b, h] = s[:, None] * math.sqrt(head_dim) * (u / (u * u).sum()) + asr.NOISE * asr.randn(g, total, head_dim)
                v[b, h] = asr.randn(g, total, head_dim)
    q = q.float()
    kc, vc = asr.to_cache(k, cache), asr.to_cache(v, cache)
    ks, vs = asr.from_cache(kc), asr.from_cache(vc)
    assert bool(torch.isfinite(ks).all()) and bool(torch.isfinite(vs).all())
    visible = asr.causal_visible(n_new, total)                      # key j visible to query t iff j <= t + past
    assert bool((visible == (torch.arange(total)[None, :] <= past + torch.arange(n_new)[:, None])).all())
    packed = q.transpose(1, 2).reshape(B, n_new, H * head_dim).contiguous()
    return packed, kc, vc, asr.ref64(q, ks, vs, visible), asr.plain32(q, ks, vs, visible)


def run(packed, kc, vc, past, n_new, lcap_extra=37):
    """The entry on a window of a larger, poisoned allocation -> (out [B, H, n_new, D] on the host, guards intact)."""
    from edgerunner_amd import kernels
    B, Hh, total, hd = kc.shape
    Lcap = total + lcap_extra
    big_k = torch.zeros(B + 2, Hh, Lcap, hd, dtype=kc.dtype)
    big_v = torch.zeros(B + 2, Hh, Lcap, hd, dtype=kc.dtype)
    asr.poison(big_k, 0)                                            # everything, the neighbouring rows included ...
    asr.poison(big_v, 0, odd=True)
    big_k[1:B + 1, :, :total] = kc                                  # ... but positions [0, past + n_new) of the call's own rows
    big_v[1:B + 1, :, :total] = vc
    big_k, big_v = big_k.to(DEV), big_v.to(DEV)
    n_out = B * n_new * Hh * hd
    buf = torch.full((GUARD + n_out + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = kernels.attn_extend(packed.to(DEV), big_k[1:B + 1], big_v[1:B + 1], past, out=buf[GUARD:GUARD + n_out])
    torch.cuda.synchronize()
    host = buf.cpu()
    intact = bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + n_out:] == SENTINEL).all())
    return out.view(B, n_new, Hh, hd).transpose(1, 2).cpu(), intact


def check_case(B, past, n_new, cache, seed, names=None, what=""):
    packed, kc, vc, r64, p32 = build(B, past, n_new, cache, seed, names)
    out, intact = run(packed, kc, vc, past, n_new)
    assert intact, f"{what}: the guards around the output were written"
    r = asr.check(out, r64, p32, *asr.TOL_SHARED, what=what)
    print(f"{what}: err / gate = {r:.3f}")
    return r


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("past", [1, 127, 128, 129, 2048, 2085])
def test_extend_parity(past, cache):
    """past_len below, at and above the chunk, odd (the fp16 pair mapping reads pairs from even keys) and not a multiple of 4 (the byte
    cache's quads); n_new 1, 2, 3, 32 and the route threshold with its predecessor."""
    worst = 0.0
    for n_new in sorted({1, 2, 3, 32, max(1, THR - 1), THR}):
        worst = max(worst, check_case(1, past, n_new, cache, 100 + past + n_new, what=f"past {past} n_new {n_new} {cache}"))
    print(f"past {past} {cache}: worst err / gate = {worst:.3f}")


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("total", [255, 256, 257])
def test_extend_chunk_boundary(total, cache):
    """past_len + n_new one short of, exactly on and one past a 128-key boundary, the new positions straddling the boundary."""
    for n_new in (3, 5):
        check_case(1, total - n_new, n_new, cache, 300 + total + n_new, what=f"total {total} n_new {n_new} {cache}")


@pytest.mark.parametrize("cache", CACHES)
def test_extend_batch_rows_differ(cache):
    """B = 5 rows of different content against their own references, and row 2 alone gives the same bits as row 2 of the batch."""
    past, n_new = 131, 6
    packed, kc, vc, r64, p32 = build(5, past, n_new, cache, 7)
    out, intact = run(packed, kc, vc, past, n_new)
    assert intact
    print(f"B = 5 {cache}: err / gate = {asr.check(out, r64, p32, *asr.TOL_SHARED, what=f'B 5 {cache}'):.3f}")
    alone, intact = run(packed[2:3], kc[2:3], vc[2:3], past, n_new)
    assert intact and torch.equal(alone[0], out[2])


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("name", ["offset_hi", "dead_chunks"])
def test_extend_hard_profiles(name, cache):
    """Scores near +90 (exp overflows without the max subtraction) and chunks whose mass is exactly 0 next to live ones, over more than
    two chunks, with queries of scale 1, -1, 0.25 and 0."""
    for past, n_new in ((300, 4), (259, 9)):
        check_case(2, past, n_new, cache, 500 + past, names=[name, "rising"], what=f"{name} past {past} n_new {n_new} {cache}")


@pytest.mark.parametrize("cache", ["f32", "f16"])
def test_extend_head_dim_64(cache):
    """head_dim 64 where the lane mapping has it (fp32 and fp16: the row mapping)."""
    past, n_new = 129, 3
    packed, kc, vc, r64, p32 = build(2, past, n_new, cache, 11, head_dim=64)
    out, intact = run(packed, kc, vc, past, n_new)
    assert intact
    print(f"head_dim 64 {cache}: err / gate = {asr.check(out, r64, p32, *asr.TOL_SHARED, what=f'D 64 {cache}'):.3f}")


def test_extend_refusals_write_nothing():
    from edgerunner_amd import native
    lib = native.load_library()
    Lcap = 64
    q = torch.zeros(1, 2, H * D, device=DEV)
    out = torch.full((1, 2, H * D), SENTINEL, device=DEV)
    caches = {0: torch.zeros(1, H, Lcap, D, device=DEV), 1: torch.zeros(1, H, Lcap, D, dtype=torch.float16, device=DEV),
              2: torch.zeros(1, H, Lcap, D, dtype=torch.uint8, device=DEV)}

    def call(past, n_new, kv_half=0, head_dim=D, B=1, l_cap=Lcap, qq=q):
        c = caches.get(kv_half, caches[0])
        return lib.er_k_attn_extend(native.ptr(qq), native.ptr(c), native.ptr(c), past, n_new, native.ptr(out), B, H, l_cap, head_dim, kv_half, None)

    assert call(0, 2) == -1 and call(-3, 2) == -1                   # ER_ERR_INVALID: no past
    assert call(10, 0) == -1 and call(10, 70000) == -1              # n_new outside [1, 65535]
    assert call(10, 2, kv_half=3) == -1 and call(10, 2, B=0) == -1
    assert call(10, 2, qq=None) == -1
    assert call(63, 2) == -4 and call(2 ** 31 - 1, 2) == -4         # ER_ERR_CAPACITY: past_len + n_new > l_cap, without overflow
    assert call(10, 2, kv_half=2, head_dim=64) == -5 and call(10, 2, head_dim=128) == -5      # ER_ERR_UNSUPPORTED
    assert b"er_k_attn_extend" in lib.er_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(62, 2) == 0                                          # the last two positions of the cache are fine
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == SENTINEL).any())
