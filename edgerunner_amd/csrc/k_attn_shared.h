// Decode attention for batch rows that share a cached prefix (er_set_prefix_groups): a GROUP is a set of rows of one reserved batch whose
// first P cache positions hold bit-identical K/V in every layer; its leader is its lowest row.  The streaming kernel of k_attn_decode.h
// reads every row's whole key range, so the shared prefix crosses HBM once per row and step.  Here it crosses once per group:
//
//   1. attn_prefix_kernel, grid (H, ceil(P / 128), groups): a workgroup loads ITS 128 prefix keys of the LEADER's K and V once - into
//      registers, with the lane mapping and the load order of attn_wave_pass - and then walks the rows of its group: q of the row, scores,
//      the waves' own softmax, the weighted V sum, the four-wave merge, one chunk-local partial {m, l, o[D]} per (row, head, chunk).  What
//      a row gets is attn_decode2_kernel's partial of that chunk, statement for statement: it depends on the row's q and the chunk's bits,
//      not on the size of the group, the row's place in it or the other groups (the chunk size and the grid's first two dimensions follow
//      from P alone; a group is never split or padded, so there is no row tile that two groups could meet in).
//   2. attn_suffix_merge_kernel, grid (H, B): the streaming kernel's shape over keys [P, len) of the row's OWN cache, then the row's prefix
//      partials folded in with attn_combine2_kernel's pass, and the normalised row written exactly where attn_stream_kernel writes it:
//      out[b][h D ..] and, when asked, the tiled hi | lo image of out_proj.
//
// The prefix pass runs on the VALU over the lane mapping of the other decode attention kernels, not on the matrix cores, although its
// work is rows x keys x D: that keeps a row's bits those of the split kernel whatever shares its group, at the price that a row costs
// about 2 us of VALU work per chunk (divisions, exponentials, fp16 unpacking and the cross-lane folds as much as the products).  Measured
// (DESIGN.md section 6): with 32 rows of one cloud the pass is 58 us (fp32 cache) / 68 us (fp16) per layer, far above what its bytes
// need; the fp32 step gains 1.34x, the fp16 step LOSES 10 %.  Four rows side by side per round (more independent chains per SIMD) was
// tried and measured: fp32 53 us, fp16 86 us, singletons 3x slower (spare slots recompute) - the pass is bound by VALU issue, not by
// latency.  S^T = K Q^T / O^T = V^T P^T on the fp32 MFMAs (flash_attn_f32_kernel's scheme, hi/lo-split for the fp16 cache) is the next step.
//
// A follower's own cache entries [0, P) are never read: a masked key's load is clamped into [P, len), and a row without a suffix
// (len == P) skips the walk.
#pragma once
#include "k_attn_decode.h"

namespace er {

constexpr int ATTN_SHARED_CHUNK = 128;        // prefix keys per workgroup: fp32 4 wave-steps x 4 waves x 8 keys, fp16 2 x 4 x 16
inline int attn_shared_chunks(int prefix_len) { return (prefix_len + ATTN_SHARED_CHUNK - 1) / ATTN_SHARED_CHUNK; }

struct AttnSharedArgs {
    AttnDecArgs a;           // q, caches, lengths, out, out_xt as for the streaming kernel; part = [B][H][S][D + 2] with S = chunks of the prefix
    const int* grp_rows;     // the rows of every group, group after group, leader first
    const int* grp_off;      // [groups + 1]: group g is grp_rows[grp_off[g] .. grp_off[g + 1])
    int prefix_len;          // P >= 1
};

// ---- 1. the prefix pass
template <typename KT, int D, int NS>
__global__ __launch_bounds__(ER_WG) void attn_prefix_kernel(AttnSharedArgs s) {
    using M = KMap<KT, D>;
    constexpr int NV = M::NV, EPL = M::EPL, NK = M::NK, KPW = M::KPW;
    static_assert(ER_NWAVES * KPW * NS == ATTN_SHARED_CHUNK, "a workgroup's wave-steps cover one chunk");
    // two sets: row r + 1 stores its wave partials while the slowest wave still merges row r (one barrier per row)
    __shared__ __attribute__((aligned(16))) float ored[2][ER_NWAVES * 4 * D];
    __shared__ float wm[2][ER_NWAVES], wl[2][ER_NWAVES];
    const AttnDecArgs& a = s.a;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const M m(lane);
    const int h = blockIdx.x, c = blockIdx.y, g = blockIdx.z;      // heads fastest: XCD = h % 8 (see attn_decode_kernel)
    // small operands first: the group's rows and the first row's q, then the K/V stream
    const int r0 = s.grp_off[g], r1 = s.grp_off[g + 1];
    const int leader = s.grp_rows[r0];
    float qv[NV][EPL];
    m.load_q(a.q + (long long)leader * a.hidden + h * D, qv);
    const int k0 = c * ATTN_SHARED_CHUNK, k1 = min(s.prefix_len, k0 + ATTN_SHARED_CHUNK);      // k0 < P: the grid has ceil(P / 128) chunks
    const long long head_off = (long long)leader * a.kv_bstride + (long long)h * a.l_cap * D;
    const KT* kb = reinterpret_cast<const KT*>(a.kcache) + head_off;
    const KT* vb = reinterpret_cast<const KT*>(a.vcache) + head_off;
    f32x4 kreg[NS][NV], vreg[NS][NV];
    bool valid[NS][NK];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        int row[NK];
#pragma unroll
        for (int n = 0; n < NK; ++n) {
            const int kk = k0 + (i * ER_NWAVES + wid) * KPW + m.key0() + n;
            valid[i][n] = kk < k1;
            row[n] = valid[i][n] ? kk : k0;          // a masked key reads row k0, which the chunk always holds
        }
        m.load(kb, row, kreg[i]);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int kk = k0 + (i * ER_NWAVES + wid) * KPW + m.key0();
        int row[NK];
#pragma unroll
        for (int n = 0; n < NK; ++n) row[n] = valid[i][n] ? kk + n : k0;
        m.load(vb, row, vreg[i]);
    }
    __builtin_amdgcn_sched_barrier(0);        // every K and V load is issued before the first score is computed

    for (int r = r0; r < r1; ++r) {
        const int b = s.grp_rows[r], set = (r - r0) & 1;
        // the next row's q travels while this row is reduced (the last row re-reads its own)
        float qn[NV][EPL];
        m.load_q(a.q + (long long)s.grp_rows[min(r + 1, r1 - 1)] * a.hidden + h * D, qn);
        float sc[NS][NK];
        float mloc = -INFINITY;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            float d[NK];
            m.dots(kreg[i], qv, d);
#pragma unroll
            for (int n = 0; n < NK; ++n) {
                sc[i][n] = valid[i][n] ? d[n] / a.sqrt_d : -INFINITY;
                mloc = fmaxf(mloc, sc[i][n]);
            }
        }
        const float mw = wave_max(mloc);          // -inf when the wave holds no valid key (the ragged last chunk)
        float o[NV][EPL];
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; ++e) o[j][e] = 0.f;
        float lloc = 0.f;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            float pw[NK];
#pragma unroll
            for (int n = 0; n < NK; ++n) pw[n] = valid[i][n] ? expf(sc[i][n] - mw) : 0.f;
            if (m.counts()) lloc += M::wsum(pw);      // each key counted once
            m.accum(vreg[i], pw, o);
        }
        const float l = wave_sum(lloc);
        attn_fold_store<D>(m, o, ored[set], wid, lane);
        if (lane == 0) { wm[set][wid] = mw; wl[set][wid] = l; }
        __syncthreads();
        if (tid < D) {
            float ov, lv, mx;                         // mx is finite: the chunk holds at least one key
            attn_merge4<D>(ored[set], wm[set], wl[set], tid, ov, lv, mx);
            float* pout = a.part + (((long long)b * a.H + h) * a.S + c) * (D + 2);
            pout[2 + tid] = ov;
            if (tid == 0) { pout[0] = mx; pout[1] = lv; }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; ++e) qv[j][e] = qn[j][e];
    }
}

// ---- 2. suffix + merge.  attn_stream_load / attn_stream_reduce of k_attn_decode.h with a lower end: keys [lo, len), a masked key's load
// clamped INTO that range (below lo lies what a follower never reads; len > lo, the caller checks)
template <typename KT, int D, int STEPS>
__device__ __forceinline__ void attn_range_load(AttnTile<KT, D, STEPS>& t, const KMap<KT, D>& m, const KT* kb, const KT* vb, int kbase, int lo, int len, int wid) {
    using M = KMap<KT, D>;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
        int row[M::NK];
#pragma unroll
        for (int n = 0; n < M::NK; ++n) row[n] = max(lo, min(kbase + (i * ER_NWAVES + wid) * M::KPW + m.key0() + n, len - 1));
        m.load(kb, row, t.k[i]);
    }
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
        int row[M::NK];
#pragma unroll
        for (int n = 0; n < M::NK; ++n) row[n] = max(lo, min(kbase + (i * ER_NWAVES + wid) * M::KPW + m.key0() + n, len - 1));
        m.load(vb, row, t.v[i]);
    }
}

template <typename KT, int D, int STEPS>
__device__ __forceinline__ void attn_range_reduce(const AttnTile<KT, D, STEPS>& t, const KMap<KT, D>& m, const float (&qv)[KMap<KT, D>::NV][KMap<KT, D>::EPL],
                                                  int kbase, int lo, int len, int wid, float sqrt_d, float& m_run, float& l_lane,
                                                  float (&o)[KMap<KT, D>::NV][KMap<KT, D>::EPL]) {
    using M = KMap<KT, D>;
    constexpr int NV = M::NV, EPL = M::EPL, NK = M::NK;
    float sc[STEPS][NK];
    float mloc = -INFINITY;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
        const int kk = kbase + (i * ER_NWAVES + wid) * M::KPW + m.key0();
        float d[NK];
        m.dots(t.k[i], qv, d);
#pragma unroll
        for (int n = 0; n < NK; ++n) {
            sc[i][n] = (kk + n >= lo && kk + n < len) ? d[n] / sqrt_d : -INFINITY;
            mloc = fmaxf(mloc, sc[i][n]);
        }
    }
    const float m_new = fmaxf(m_run, wave_max(mloc));
    if (m_new == -INFINITY) return;                      // wave-uniform: this wave has not seen a valid key yet
    const float alpha = expf(m_run - m_new);             // exp(-inf) = 0 on the first tile with keys
    float pw[STEPS][NK];
    float ladd = 0.f;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) {
#pragma unroll
        for (int n = 0; n < NK; ++n) pw[i][n] = expf(sc[i][n] - m_new);     // 0 for masked keys
        ladd += M::wsum(pw[i]);
    }
    l_lane = fmaf(l_lane, alpha, m.counts() ? ladd : 0.f);
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[j][e] *= alpha;
#pragma unroll
    for (int i = 0; i < STEPS; ++i) m.accum(t.v[i], pw[i], o);
    m_run = m_new;
}

template <typename KT, int D, int STEPS>
__global__ __launch_bounds__(ER_WG) void attn_suffix_merge_kernel(AttnSharedArgs s) {
    using M = KMap<KT, D>;
    constexpr int NV = M::NV, EPL = M::EPL, W = D + 2;
    constexpr int TILE = ER_NWAVES * STEPS * M::KPW;     // keys per workgroup iteration
    __shared__ __attribute__((aligned(16))) float ored[ER_NWAVES * 4 * D];
    __shared__ float wm[ER_NWAVES], wl[ER_NWAVES];
    __shared__ float half1[128];
    const AttnDecArgs& a = s.a;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const M m(lane);
    const int h = blockIdx.x, b = blockIdx.y;
    const int len = attn_len(a, b), P = s.prefix_len;
    const long long head_off = (long long)b * a.kv_bstride + (long long)h * a.l_cap * D;
    const KT* kb = reinterpret_cast<const KT*>(a.kcache) + head_off;
    const KT* vb = reinterpret_cast<const KT*>(a.vcache) + head_off;
    float qv[NV][EPL];
    m.load_q(a.q + (long long)b * a.hidden + h * D, qv);
    float o[NV][EPL];
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[j][e] = 0.f;
    float m_run = -INFINITY, l_lane = 0.f;

    if (len > P) {                                        // workgroup-uniform; without a suffix the row is its prefix partials alone
        // the pair mapping reads two rows of an EVEN key as three whole lines: an odd P starts its first tile one key early and masks it
        const int kstart = M::NK == 2 ? (P & ~1) : P;
        const int nt = (len - kstart + TILE - 1) / TILE;  // >= 1
        AttnTile<KT, D, STEPS> ta, tb;
        attn_range_load<KT, D, STEPS>(ta, m, kb, vb, kstart, P, len, wid);
        for (int t = 0; t < nt; t += 2) {
            attn_range_load<KT, D, STEPS>(tb, m, kb, vb, kstart + (t + 1) * TILE, P, len, wid);
            __builtin_amdgcn_sched_barrier(0);
            attn_range_reduce<KT, D, STEPS>(ta, m, qv, kstart + t * TILE, P, len, wid, a.sqrt_d, m_run, l_lane, o);
            __builtin_amdgcn_sched_barrier(0);
            attn_range_load<KT, D, STEPS>(ta, m, kb, vb, kstart + (t + 2) * TILE, P, len, wid);
            __builtin_amdgcn_sched_barrier(0);
            if (t + 1 < nt) attn_range_reduce<KT, D, STEPS>(tb, m, qv, kstart + (t + 1) * TILE, P, len, wid, a.sqrt_d, m_run, l_lane, o);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const float l = wave_sum(l_lane);
    attn_fold_store<D>(m, o, ored, wid, lane);            // zeros from a wave (or a row) without suffix keys
    if (lane == 0) { wm[wid] = m_run; wl[wid] = l; }
    __syncthreads();

    // the suffix as ONE more partial {mx, lv, ov} in front of the row's prefix partials, merged as attn_combine2_kernel merges: thread
    // (c, half) owns column c of every second partial of a pass, every thread carries the running maximum and sum.  The order of the
    // partials and of the passes follows from P alone.
    const int c = tid & 127, half = tid >> 7;
    const int cc = min(c, D - 1);
    float ov, lv, mx;                                     // mx = -inf, lv = 0, ov = 0 without a suffix
    attn_merge4<D>(ored, wm, wl, cc, ov, lv, mx);
    float M_run = mx, l_run = lv, o_run = half == 0 ? ov : 0.f;
    const int n_act = a.S;                                // ceil(P / 128) >= 1 partials, every one of them holds a key
    const float* pb = a.part + ((long long)b * a.H + h) * n_act * W;
    int base = 0;
    while (base < n_act) {
        const int rem = n_act - base;
        if (rem <= 16) { combine_pass<D, 8>(pb, base, n_act, cc, half, lane, M_run, l_run, o_run); base += 16; }
        else if (rem <= 32) { combine_pass<D, 16>(pb, base, n_act, cc, half, lane, M_run, l_run, o_run); base += 32; }
        else if (rem <= 48) { combine_pass<D, 24>(pb, base, n_act, cc, half, lane, M_run, l_run, o_run); base += 48; }
        else { combine_pass<D, 32>(pb, base, n_act, cc, half, lane, M_run, l_run, o_run); base += 64; }
    }
    if (half == 1) half1[c] = o_run;
    __syncthreads();
    if (half == 0 && c < D) {
        const float r = (o_run + half1[c]) / l_run;
        a.out[(long long)b * a.hidden + h * D + c] = r;
        if (a.out_xt) {        // as attn_stream_kernel: halves (k & 3) [hi] and 4 + (k & 3) [lo] of entry (k >> 2, b)
            const int k = h * D + c;
            _Float16* e = reinterpret_cast<_Float16*>(a.out_xt) + xt_entry(a.hidden, b, k >> 2) * 8 + (k & 3);
            const _Float16 hi = (_Float16)r;
            e[0] = hi;
            e[4] = (_Float16)(r - (float)hi);
        }
    }
}

// the two launches of a layer (launch_kind_t kinds 1 and 2); s.a.S must be attn_shared_chunks(s.prefix_len)
template <int D>
inline hipError_t launch_attn_prefix_d(const AttnSharedArgs& s, bool kv_half, int groups, hipStream_t st) {
    if (s.prefix_len < 1 || s.prefix_len > s.a.l_cap || s.a.S != attn_shared_chunks(s.prefix_len) || groups < 1 || groups > 65535) return hipErrorInvalidValue;
    const dim3 grid(s.a.H, s.a.S, groups), blk(ER_WG);
    if (!kv_half) hipLaunchKernelGGL((attn_prefix_kernel<float, D, 4>), grid, blk, 0, st, s);
    else hipLaunchKernelGGL((attn_prefix_kernel<_Float16, D, 2>), grid, blk, 0, st, s);
    return hipGetLastError();
}
template <int D>
inline hipError_t launch_attn_suffix_merge_d(const AttnSharedArgs& s, bool kv_half, int B, hipStream_t st) {
    if (s.a.S != attn_shared_chunks(s.prefix_len)) return hipErrorInvalidValue;
    const dim3 grid(s.a.H, B), blk(ER_WG);
    if (!kv_half) hipLaunchKernelGGL((attn_suffix_merge_kernel<float, D, 2>), grid, blk, 0, st, s);
    else hipLaunchKernelGGL((attn_suffix_merge_kernel<_Float16, D, 2>), grid, blk, 0, st, s);
    return hipGetLastError();
}

// ---- the prefill's check of a grouping: every follower's K/V [0, P) of every layer against its leader's, bit for bit.  Grid
// (H, 2 * layers, followers); the first mismatch in (row, layer) order is left in *first as row * layers + layer (atomicMin on a word that
// starts at INT_MAX).  A head's prefix is P * D elements = a multiple of 16 bytes at a 16-byte aligned offset (D = 96, Lcap % 32 == 0).
struct PrefixCheckArgs {
    const char *kc, *vc;         // [layers][B][H][Lcap][D]
    const int* followers;        // rows with leader[b] != b
    const int* leader;           // [B]
    long long head_bytes, row_bytes, layer_bytes;      // Lcap * D, H * Lcap * D, B * H * Lcap * D elements in bytes
    long long prefix_vecs;       // P * D * element size / 16
    int layers;
    int* first;
};
__global__ __launch_bounds__(ER_WG) void prefix_check_kernel(PrefixCheckArgs p) {
    const int h = blockIdx.x, layer = blockIdx.y >> 1, b = p.followers[blockIdx.z];
    const char* base = ((blockIdx.y & 1) ? p.vc : p.kc) + layer * p.layer_bytes + h * p.head_bytes;
    const uint4* mine = reinterpret_cast<const uint4*>(base + b * p.row_bytes);
    const uint4* lead = reinterpret_cast<const uint4*>(base + p.leader[b] * p.row_bytes);
    bool diff = false;
    for (long long i = threadIdx.x; i < p.prefix_vecs; i += ER_WG) {
        const uint4 x = mine[i], y = lead[i];
        diff |= x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
    }
    if (diff) atomicMin(p.first, b * p.layers + layer);
}
inline hipError_t launch_prefix_check(const PrefixCheckArgs& p, int heads, int followers, hipStream_t st) {
    if (followers < 1) return hipSuccess;
    hipLaunchKernelGGL(prefix_check_kernel, dim3(heads, 2 * p.layers, followers), dim3(ER_WG), 0, st, p);
    return hipGetLastError();
}

}  // namespace er
