// Attention of a prefill with a past (er_prefill_extend): n_new queries per row at positions [past_len, past_len + n_new), query t sees
// the row's cached keys [0, past_len) and the new keys up to itself, i.e. keys <= past_len + t.  The new positions' K/V are in the cache
// already (the QKV epilogue / kv_scatter wrote them), so both routes read ONE key range [0, past_len + n_new).
//
//   rows route (small n_new: another face count is 2 positions, a short resume a handful):
//   1. attn_extend_kernel, grid (H, ceil((past_len + n_new) / 128), B): a workgroup loads ITS 128 keys of the row's own K and V once - into
//      registers, with the lane mapping (KMap) and the load order of attn_wave_pass - and then walks the queries that see the chunk, the
//      next q prefetched: scores, the waves' own softmax, the weighted V sum, the four-wave merge (attn_merge4), one chunk-local partial
//      {m, l, o[D]} per (row, query, head, chunk).  This is attn_prefix_kernel's walk with the roles turned: there one leader's keys serve
//      the rows of a group, here one row's keys serve its own new queries, and the mask moves with the query.  A chunk wholly above a
//      query's last key is skipped for that query (the walk starts at the first query that sees key k0); a straddling chunk masks by
//      selection - a key past past_len + n_new - 1 is never read, its load is clamped to row k0, which the chunk always holds.
//   2. attn_extend_merge_kernel, grid (H, n_new, B): attn_combine2_kernel's pass (combine_pass) over the (past_len + t) / 128 + 1 partials
//      of query t, the normalised row written to out[(b * n_new + t) * ldo + h * D ..] - the [B * n_new][H * D] rows out_proj's Linear reads.
//
//   flash route (large n_new): the prefill's own flash kernels with N = n_new, M = past_len + n_new, causal_off = past_len.  The exact
//   mode's kernel reads the fp32 cache in place; fast and kv8 mode read fp32 scratch, which kv_gather_kernel - the inverse of
//   kv_scatter - fills from the fp16 / e4m3 cache (every such value is exact in fp32).
//
// Which route a call takes is extend_attn_rows (er_extend_plan.h), measured in profiles/prefill_extend_bench.json.
#pragma once
#include "er_w8.h"
#include "k_attn_decode.h"

namespace er {

constexpr int ATTN_EXTEND_CHUNK = 128;        // keys per workgroup: fp32 4 wave-steps x 4 waves x 8 keys, fp16 2 x 4 x 16, bytes 1 x 4 x 32
inline int attn_extend_chunks(int total_len) { return (total_len + ATTN_EXTEND_CHUNK - 1) / ATTN_EXTEND_CHUNK; }
inline size_t attn_extend_part_floats(int B, int n_new, int H, int total_len, int D) {
    return (size_t)B * n_new * H * attn_extend_chunks(total_len) * (D + 2);
}

struct AttnExtendArgs {
    const float* q;          // query (b, t) of head h at q[(b * n_new + t) * ldq + h * D]
    const void* kcache;      // [B][H][Lcap][D], fp32, fp16 or e4m3 bytes (the kernel's KT); positions [0, past_len + n_new) are read
    const void* vcache;
    float* part;             // [B][n_new][H][S][D + 2] = {m, l, o[0..D)}, S = attn_extend_chunks(past_len + n_new)
    float* out;              // merge: row (b, t) at out[(b * n_new + t) * ldo]
    int ldq, ldo;
    int H, l_cap, S, past_len, n_new;
    long long kv_bstride;
    float sqrt_d;            // sqrt(D): scores are divided by it, as the reference does
};

template <typename KT, int D, int NS>
__global__ __launch_bounds__(ER_WG) void attn_extend_kernel(AttnExtendArgs a) {
    using M = KMap<KT, D>;
    constexpr int NV = M::NV, EPL = M::EPL, NK = M::NK, KPW = M::KPW;
    static_assert(ER_NWAVES * KPW * NS == ATTN_EXTEND_CHUNK, "a workgroup's wave-steps cover one chunk");
    // two sets: query t + 1 stores its wave partials while the slowest wave still merges query t (one barrier per query)
    __shared__ __attribute__((aligned(16))) float ored[2][ER_NWAVES * 4 * D];
    __shared__ float wm[2][ER_NWAVES], wl[2][ER_NWAVES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const M m(lane);
    const int h = blockIdx.x, c = blockIdx.y, b = blockIdx.z;      // heads fastest: XCD = h % 8 (see attn_decode_kernel)
    const int total = a.past_len + a.n_new;
    const int k0 = c * ATTN_EXTEND_CHUNK, k1 = min(total, k0 + ATTN_EXTEND_CHUNK);      // k0 < total: the grid has ceil(total / 128) chunks
    // the first query that sees key k0; every later one sees it too, so each walked query finds a key here and its partial's m is finite
    const int t0 = max(0, k0 - a.past_len);
    // small operands first: the first query's q, then the K/V stream
    const float* qrow = a.q + (long long)b * a.n_new * a.ldq + h * D;
    float qv[NV][EPL];
    m.load_q(qrow + (long long)t0 * a.ldq, qv);
    const long long head_off = (long long)b * a.kv_bstride + (long long)h * a.l_cap * D;
    const KT* kb = reinterpret_cast<const KT*>(a.kcache) + head_off;
    const KT* vb = reinterpret_cast<const KT*>(a.vcache) + head_off;
    f32x4 kreg[NS][NV], vreg[NS][NV];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        int row[NK];
#pragma unroll
        for (int n = 0; n < NK; ++n) {
            const int kk = k0 + (i * ER_NWAVES + wid) * KPW + m.key0() + n;
            row[n] = kk < k1 ? kk : k0;              // a key the call does not own reads row k0, which the chunk always holds
        }
        m.load(kb, row, kreg[i]);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        int row[NK];
#pragma unroll
        for (int n = 0; n < NK; ++n) {
            const int kk = k0 + (i * ER_NWAVES + wid) * KPW + m.key0() + n;
            row[n] = kk < k1 ? kk : k0;
        }
        m.load(vb, row, vreg[i]);
    }
    __builtin_amdgcn_sched_barrier(0);        // every K and V load is issued before the first score is computed

    for (int t = t0; t < a.n_new; ++t) {
        const int set = (t - t0) & 1;
        const int last = a.past_len + t;          // the query's own position: its last visible key (< total, so a visible key was loaded)
        // the next query's q travels while this one is reduced (the last query re-reads its own)
        float qn[NV][EPL];
        m.load_q(qrow + (long long)min(t + 1, a.n_new - 1) * a.ldq, qn);
        float sc[NS][NK];
        bool vis[NS][NK];
        float mloc = -INFINITY;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            float d[NK];
            m.dots(kreg[i], qv, d);
#pragma unroll
            for (int n = 0; n < NK; ++n) {
                vis[i][n] = k0 + (i * ER_NWAVES + wid) * KPW + m.key0() + n <= last;
                sc[i][n] = vis[i][n] ? d[n] / a.sqrt_d : -INFINITY;
                mloc = fmaxf(mloc, sc[i][n]);
            }
        }
        const float mw = wave_max(mloc);          // -inf when the wave holds no visible key
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
            for (int n = 0; n < NK; ++n) pw[n] = vis[i][n] ? expf(sc[i][n] - mw) : 0.f;
            if (m.counts()) lloc += M::wsum(pw);      // each key counted once
            m.accum(vreg[i], pw, o);
        }
        const float l = wave_sum(lloc);
        attn_fold_store<D>(m, o, ored[set], wid, lane);
        if (lane == 0) { wm[set][wid] = mw; wl[set][wid] = l; }
        __syncthreads();
        if (tid < D) {
            float ov, lv, mx;                         // mx is finite: key k0 is visible to every walked query
            attn_merge4<D>(ored[set], wm[set], wl[set], tid, ov, lv, mx);
            float* pout = a.part + ((((long long)b * a.n_new + t) * a.H + h) * a.S + c) * (D + 2);
            pout[2 + tid] = ov;
            if (tid == 0) { pout[0] = mx; pout[1] = lv; }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; ++e) qv[j][e] = qn[j][e];
    }
}

// query t's partials are chunks [0, (past_len + t) / 128]: exactly those attn_extend_kernel wrote for it
template <int D>
__global__ __launch_bounds__(ER_WG) void attn_extend_merge_kernel(AttnExtendArgs a) {
    constexpr int W = D + 2;
    __shared__ float half1[128];
    const int h = blockIdx.x, t = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int n_act = (a.past_len + t) / ATTN_EXTEND_CHUNK + 1;
    const long long qrow = (long long)b * a.n_new + t;
    const float* pb = a.part + (qrow * a.H + h) * a.S * W;
    const int c = tid & 127, half = tid >> 7;          // half is wave-uniform (waves 0,1 -> 0; waves 2,3 -> 1)
    const int cc = min(c, D - 1);
    float M_run = -INFINITY, l_run = 0.f, o_run = 0.f;
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
    if (half == 0 && c < D) a.out[qrow * a.ldo + h * D + c] = (o_run + half1[c]) / l_run;
}

// head_dim 96: all three cache types; head_dim 64: fp32 and fp16 (the byte cache's quad mapping is built for 96-byte rows)
inline bool attn_extend_supported(int D, int kv_half) { return D == 96 || (D == 64 && kv_half != 2); }

// the two launches of a layer.  kv_half: 0 = fp32, 1 = fp16, 2 = e4m3 bytes; a.S must be attn_extend_chunks(past_len + n_new)
inline hipError_t launch_attn_extend(const AttnExtendArgs& a, int D, int kv_half, int B, hipStream_t st) {
    const int total = a.past_len + a.n_new;
    if (a.past_len < 1 || a.n_new < 1 || a.n_new > 65535 || total > a.l_cap || a.S != attn_extend_chunks(total) || a.S > 65535 || B < 1 || B > 65535 ||
        kv_half < 0 || kv_half > 2 || !attn_extend_supported(D, kv_half))
        return hipErrorInvalidValue;
    const dim3 grid(a.H, a.S, B), mgrid(a.H, a.n_new, B), blk(ER_WG);
    if (D == 96) {
        if (kv_half == 0) hipLaunchKernelGGL((attn_extend_kernel<float, 96, 4>), grid, blk, 0, st, a);
        else if (kv_half == 1) hipLaunchKernelGGL((attn_extend_kernel<_Float16, 96, 2>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((attn_extend_kernel<kv8_t, 96, 1>), grid, blk, 0, st, a);
    } else {
        if (kv_half == 0) hipLaunchKernelGGL((attn_extend_kernel<float, 64, 4>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((attn_extend_kernel<_Float16, 64, 2>), grid, blk, 0, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (D == 96) hipLaunchKernelGGL((attn_extend_merge_kernel<96>), mgrid, blk, 0, st, a);
    else hipLaunchKernelGGL((attn_extend_merge_kernel<64>), mgrid, blk, 0, st, a);
    return hipGetLastError();
}

// ---- the flash route's gather in fast / kv8 mode: cache positions [0, T) of every row and head as fp32 rows kx[b * T + s][2 * hidden]
// (K in columns [0, hidden), V behind them: heads side by side, as the fused projection lays them out).  kv_scatter's grid and
// indexing turned round: a token row per blockIdx.y (strided), four consecutive columns per thread (head_dim % 4 == 0).
template <typename CT>
__global__ __launch_bounds__(ER_WG) void kv_gather_kernel(const CT* kcache, const CT* vcache, float* kx, int M, int T, int hidden, int head_dim,
                                                          int l_cap, long long kv_bstride) {
    const int c2 = (blockIdx.x * ER_WG + threadIdx.x) * 4;
    if (c2 >= 2 * hidden) return;
    const int which = c2 >= hidden ? 1 : 0, c = c2 - which * hidden;       // 0 = K, 1 = V
    const int h = c / head_dim, d = c - h * head_dim;
    const CT* cache = which == 0 ? kcache : vcache;
    for (int m = blockIdx.y; m < M; m += gridDim.y) {
        const int b = m / T, s = m - b * T;
        const CT* src = cache + (long long)b * kv_bstride + ((long long)h * l_cap + s) * head_dim + d;
        f32x4 v;
        if constexpr (sizeof(CT) == 2) {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            const h4 hv = *reinterpret_cast<const h4*>(src);
            v = (f32x4){(float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]};
        } else {
            const unsigned w = *reinterpret_cast<const unsigned*>(src);
            v = (f32x4){w8_decode((unsigned char)(w & 0xff)), w8_decode((unsigned char)((w >> 8) & 0xff)), w8_decode((unsigned char)((w >> 16) & 0xff)),
                        w8_decode((unsigned char)(w >> 24))};
        }
        *reinterpret_cast<f32x4*>(kx + (long long)m * 2 * hidden + c2) = v;
    }
}
// f8: the byte cache of kv8 mode, else the fp16 cache of fast mode
inline hipError_t launch_kv_gather(const void* kcache, const void* vcache, float* kx, bool f8, int M, int T, int hidden, int head_dim, int l_cap,
                                   long long kv_bstride, hipStream_t st) {
    if (M < 1 || T < 1 || T > l_cap || head_dim % 4 || hidden % head_dim) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((2 * hidden / 4 + ER_WG - 1) / ER_WG), (unsigned)(M < 65535 ? M : 65535));
    if (f8) hipLaunchKernelGGL(kv_gather_kernel<unsigned char>, grid, dim3(ER_WG), 0, st, (const unsigned char*)kcache, (const unsigned char*)vcache, kx, M, T,
                               hidden, head_dim, l_cap, kv_bstride);
    else hipLaunchKernelGGL(kv_gather_kernel<_Float16>, grid, dim3(ER_WG), 0, st, (const _Float16*)kcache, (const _Float16*)vcache, kx, M, T, hidden,
                            head_dim, l_cap, kv_bstride);
    return hipGetLastError();
}

}  // namespace er
