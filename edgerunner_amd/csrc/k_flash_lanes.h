// What the four fused attention kernels (k_flash_attn.h, k_flash_attn_f32.h, k_flash_attn_f16s.h) have in common, written once.
//
// All four compute both products TRANSPOSED on the 32 x 32 matrix-core shapes, S^T = K Q^T and O^T = V^T P^T, so that everything a query
// needs stays in one lane column (q = lane & 31): the row max / sum take one xor-32 exchange and the O^T rescale factor is lane-local.  A
// 64-key tile is two 32-key blocks; fa_row() is the accumulator register -> row map of both products.  Here live that map, the two online
// softmax steps over a landed key tile (base 2 on the hardware exponential for the fp16-P kernels, exact expf and a correctly rounded
// division for the prefill / point-encoder kernels), the register / LDS staging of a key tile, the causal key bounds, the normalised row
// store and the launchers' compile-time dispatch.  Nothing in this file issues a vector-memory operation except fa_fetch_tile, fa_q8 and
// fa_store_rows, which flash_attn_hh_kernel (hand-counted vmcnt waits) does not use.
#pragma once
#include <type_traits>
#include "er_common.h"
#include "er_gemm_map.h"

namespace er {

constexpr int FA_KT = 64, FA_QW = 32;       // keys per tile, queries per wave
typedef _Float16 fa_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 fa_h4 __attribute__((ext_vector_type(4)));
typedef float fa_acc __attribute__((ext_vector_type(16)));      // one 32 x 32 fp32 accumulator: 16 registers per lane

// Row of a 32 x 32 accumulator that register r of lane half `half` (= lane >> 5) holds; the column is lane & 31 = the query.
//   S^T / P^T block kb of a tile: the KEY kbase + 32 kb + fa_row(r, half)
//   O^T block db:                 the HEAD DIM 32 db + fa_row(r, half)
// (registers 4g .. 4g+3 are four consecutive rows starting at 8g + 4 half)
__host__ __device__ __forceinline__ constexpr int fa_row(int r, int half) { return mfma32_row(r, half); }

__device__ __forceinline__ void fa_zero(fa_acc& x) {
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = 0.f;
}
template <int NB>
__device__ __forceinline__ void fa_zero(fa_acc (&x)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) fa_zero(x[b]);
}

// ---- the online softmax of query lane & 31 over this lane half's 32 keys of the tile in st; st leaves as the probabilities
// Base 2 on the hardware exponential (v_exp_f32): p = 2^((s - m) scale log2 e), sl2 = scale * log2 e.  The probabilities are rounded to fp16
// before P.V, far coarser than the 1-ulp difference to expf; the accurate expf cost ~10 instructions x 32 scores per lane and tile and made
// the kernel VALU-bound at 9 % of the matrix rate (profiles/r03_dit_fp16_kernel_stats_*.csv).
__device__ __forceinline__ void fa_softmax_exp2(fa_acc (&st)[2], fa_acc (&ot)[2], float& m_run, float& l_run, int kbase, int M, int half,
                                                float sl2) {
    float mloc = -INFINITY;
    if (kbase + FA_KT <= M) {                    // wave-uniform: only the last tile can hold keys beyond M
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) mloc = fmaxf(fmaxf(mloc, st[kb][r]), st[kb][r + 1]);      // RAW scores (v_max3_f32); scaled below
    } else {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kbase + kb * 32 + fa_row(r, half);
                const float s = key < M ? st[kb][r] : -INFINITY;
                st[kb][r] = s;
                mloc = fmaxf(mloc, s);
            }
    }
    // log2 units: exp(x * scale) = exp2(x * sl2).  The maximum is taken over the raw scores (sl2 > 0) and every probability is ONE
    // fma + exp2: exp2(fma(s, sl2, -m)) - round 3 spent a multiply and a subtract per score here, and this VALU loop, not the 16
    // MFMAs of a key tile, bounds the kernel at head_dim 64.  (Packed v_pk_fma_f32 / v_pk_add_f32 forms of the same loop and
    // a zero C operand instead of clearing the score registers measured no different on the same box: profiles/r04_dit_softmax_ab.log)
    mloc = xor_max<32>(mloc) * sl2;
    const float m_new = fmaxf(m_run, mloc);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);          // m_run = -inf on the first tile -> 0
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(st[kb][r], sl2, -m_new));  // masked keys: exp2(-inf) = 0
            st[kb][r] = p;
            psum += p;
        }
    l_run = l_run * alpha + psum;
    if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0ull) {      // wave-uniform: no query of this wave met a new maximum -> alpha = 1
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[db][r] *= alpha;
    }
    m_run = m_new;
}

// Exact: scores DIVIDED by c as the reference does (attention.py:52), expf.  CAUSAL: key j is visible to query qi iff j <= qi + causal_off.
// x / c in three instructions instead of hipcc's ten-instruction division: q0 = x * y, r = fma(-q0, c, x), q = fma(r, y, q0) with y = 1 / c
// is the correctly rounded quotient for every |x| in [1e-30, 1e30] - checked over all 2^32 inputs for c = sqrtf(96) and 8, and c times a
// power of two rounds the same (scripts/probes/div_const_probe.hip, profiles/r04_div_const_probe.log); 32 divisions per lane and key tile
// were a third of this loop's VALU work.
template <bool CAUSAL, int NDB>
__device__ __forceinline__ void fa_softmax_exact(fa_acc (&st)[2], fa_acc (&ot)[NDB], float& m_run, float& l_run, int kbase, int M, int qi,
                                                 int causal_off, int half, float c, float inv_c) {
    float mloc = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kbase + kb * 32 + fa_row(r, half);
            bool ok = key < M;
            if (CAUSAL) ok = ok && key <= qi + causal_off;
            const float q0 = st[kb][r] * inv_c;
            const float s = ok ? fmaf(fmaf(-q0, c, st[kb][r]), inv_c, q0) : -INFINITY;
            st[kb][r] = s;
            mloc = fmaxf(mloc, s);
        }
    mloc = xor_max<32>(mloc);
    const float m_new = fmaxf(m_run, mloc);
    // m_new stays -inf only for a query that has not seen any key yet (padding rows q >= N of a causal tile)
    const float alpha = (m_new == -INFINITY) ? 1.0f : expf(m_run - m_new);   // m_run = -inf -> exp(-inf) = 0
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = (st[kb][r] == -INFINITY) ? 0.f : expf(st[kb][r] - m_new);
            st[kb][r] = p;
            psum += p;
        }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[db][r] *= alpha;
}

// ---- key-tile staging
// slot u of thread tid in a tile of 64 key rows x F4 float4: key row and float4 column
struct FaSlot { int key, c4; };
template <int F4, int THREADS>
__device__ __forceinline__ FaSlot fa_slot(int tid, int u) {
    const int idx = tid + THREADS * u, key = idx / F4;
    return {key, idx - key * F4};
}

// global -> registers: this thread's NST float4 of the K and V rows of the key tile at kbase (rows clamped to M - 1).  The exact kernels
// issue it a whole tile ahead: the loads of tile t + 1 are in flight while tile t is multiplied.
template <int F4, int THREADS, int NST>
__device__ __forceinline__ void fa_fetch_tile(const float* K, const float* V, int ldk, int ldv, int kbase, int M, int tid, f32x4 (&kst)[NST],
                                              f32x4 (&vst)[NST]) {
    static_assert(NST * THREADS == FA_KT * F4, "staging loop shape");
#pragma unroll
    for (int u = 0; u < NST; ++u) {
        const auto [key, c4] = fa_slot<F4, THREADS>(tid, u);
        const int gk = min(kbase + key, M - 1);
        kst[u] = *reinterpret_cast<const f32x4*>(K + (long long)gk * ldk + 4 * c4);
        vst[u] = *reinterpret_cast<const f32x4*>(V + (long long)gk * ldv + 4 * c4);
    }
}

// registers -> the fp16 LDS image Ks[key][d] (row stride KLD halves), Vt[d][key] (row stride VLD): one float4 of K and of V
template <int KLD, int VLD>
__device__ __forceinline__ void fa_stage_h16(_Float16* Ks, _Float16* Vt, int key, int c4, const f32x4& kv, const f32x4& vv) {
    *reinterpret_cast<fa_h4*>(&Ks[key * KLD + 4 * c4]) = (fa_h4){(_Float16)kv.x, (_Float16)kv.y, (_Float16)kv.z, (_Float16)kv.w};
    Vt[(4 * c4 + 0) * VLD + key] = (_Float16)vv.x;          // four 2-byte transposing stores
    Vt[(4 * c4 + 1) * VLD + key] = (_Float16)vv.y;
    Vt[(4 * c4 + 2) * VLD + key] = (_Float16)vv.z;
    Vt[(4 * c4 + 3) * VLD + key] = (_Float16)vv.w;
}

// A operand of one 16-key step of O^T += V^T P^T from that image: row d of Vt, keys kcol + {0..3} and kcol + 8 + {0..3} with
// kcol = 32 kb + 16 step + 4 half - the keys whose probabilities are registers 8 step .. 8 step + 7 of this lane (fa_row)
template <int VLD>
__device__ __forceinline__ fa_h8 fa_vt_frag(const _Float16* Vt, int d, int kcol) {
    const _Float16* vr = &Vt[d * VLD + kcol];
    const fa_h4 v0 = *reinterpret_cast<const fa_h4*>(vr);
    const fa_h4 v1 = *reinterpret_cast<const fa_h4*>(vr + 8);
    return (fa_h8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
}

// B operand of that step: the eight probabilities, rounded to fp16 (no data movement: P^T is S^T's registers)
__device__ __forceinline__ fa_h8 fa_p8(const fa_acc& p, int stp) {
    return (fa_h8){(_Float16)p[8 * stp + 0], (_Float16)p[8 * stp + 1], (_Float16)p[8 * stp + 2], (_Float16)p[8 * stp + 3],
                   (_Float16)p[8 * stp + 4], (_Float16)p[8 * stp + 5], (_Float16)p[8 * stp + 6], (_Float16)p[8 * stp + 7]};
}

// B operand of S^T on the fp16 matrix cores, step ks: dims 16 ks + 8 half + {0..7} of the fp32 query row qr
__device__ __forceinline__ void fa_q8(const float* qr, int ks, int half, float (&x)[8]) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(qr + ks * 16 + half * 8);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(qr + ks * 16 + half * 8 + 4);
    x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w;
    x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
}

// ---- prologue and epilogue
// Key tiles a workgroup of NWV waves walks for query tile qt, and the last key this WAVE (queries q0 .. q0 + 31) can see: beyond it the
// wave has nothing to do.  CAUSAL: key j is visible to query i iff j <= i + causal_off.
struct FaKeyBounds { int ntiles, wave_last_key; };
template <bool CAUSAL, int NWV>
__device__ __forceinline__ FaKeyBounds fa_key_bounds(int N, int M, int causal_off, int qt, int q0) {
    const int wg_last_q = min(N - 1, qt * (NWV * FA_QW) + NWV * FA_QW - 1);
    const int kmax = CAUSAL ? min(M, wg_last_q + causal_off + 1) : M;
    return {(kmax + FA_KT - 1) / FA_KT, CAUSAL ? (q0 + FA_QW - 1 + causal_off) : (M - 1)};
}

// orow[d] = O^T[d][q] / l_tot for the output row of query lane & 31
template <int NDB, typename T>
__device__ __forceinline__ void fa_store_rows(T* orow, const fa_acc (&ot)[NDB], float l_tot, int half) {
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) orow[db * 32 + fa_row(r, half)] = (T)(ot[db][r] / l_tot);
}

// ---- launch
// waves per workgroup of the prefill kernels: two while four-wave workgroups (128 queries) would leave fewer than three per CU
inline int fa_auto_waves(int N, int H, int B) {
    const long long wg4 = (long long)((N + 4 * FA_QW - 1) / (4 * FA_QW)) * H * B;
    return wg4 < 768 ? 2 : 4;
}

template <typename F>
inline void fa_with_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
// f(D, causal, NWV) with the three as integral constants, for a head_dim among Ds and two or four waves; false for any other head_dim
template <int... Ds, typename F>
inline bool fa_dispatch(int D, bool causal, int nwv, F&& f) {
    auto on_d = [&](auto d) {
        fa_with_bool(causal, [&](auto c) {
            fa_with_bool(nwv == 4, [&](auto w4) { f(d, c, std::integral_constant<int, decltype(w4)::value ? 4 : 2>{}); });
        });
        return true;
    };
    return ((D == Ds && on_d(std::integral_constant<int, Ds>{})) || ...);
}

}  // namespace er
