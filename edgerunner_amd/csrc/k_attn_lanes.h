// How the lanes of a wave cover the keys of the decode KV cache, and the one pass every wave of the split kernels runs over its keys.
//
// KMap<KT, D> is the lane mapping: which 16 bytes of which key row a lane loads, how a wave-step's q.k products come out of those registers,
// how a wave-step of V is accumulated and how the wave's accumulators are folded into rows of 16 lanes and stored to LDS.  It has three
// forms - the ROW mapping (fp32 caches, and fp16 caches whose rows are whole 128-byte lines), the PAIR mapping (fp16 cache, D = 96) and
// the QUAD mapping (e4m3 byte cache, D = 96) - and the kernels of k_attn_decode.h are written once over it.  attn_wave_pass is "load NS
// wave-steps of K and V, score, soften, accumulate, fold" of the per-wave-softmax kernels; attn_merge4 merges the four waves of a
// 256-thread workgroup.
#pragma once
#include "er_common.h"
#include "er_kv8_map.h"

// timeline hooks of scripts/probes/attn_timeline_probe.hip (expand to nothing in the library build)
#ifndef ER_TP
#define ER_TP(i)
#endif

namespace er {

// 16 bytes of a key row as EPL floats
template <typename KT> struct KVec;
template <> struct KVec<float> { static constexpr int EPL = 4, LPK = 8; };      // 8 lanes x NV float4 per key row
template <> struct KVec<_Float16> { static constexpr int EPL = 8, LPK = 4; };   // 4 lanes x NV (8 x fp16) per key row

template <typename KT>
__device__ __forceinline__ void kv_unpack(const f32x4& raw, float (&f)[KVec<KT>::EPL]) {
    if constexpr (sizeof(KT) == 4) {
        f[0] = raw.x; f[1] = raw.y; f[2] = raw.z; f[3] = raw.w;
    } else {
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        const h8 h = __builtin_bit_cast(h8, raw);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (float)h[i];
    }
}

// ---- fp16 cache: lanes mapped over PAIRS of key rows (round 5).
//
// A row of the fp16 cache is 96 halves = 192 bytes = one and a half 128-byte lines.  The first fp16 mapping gave a row to 4 lanes x
// 3 loads, so load j of a wave read the j-th 64-byte THIRD of 16 rows: sixteen half-used lines per wave-instruction, every line
// requested by two instructions - 12 % below the rate of whole-line requests at the same bytes (5.8 vs 5.15 us for 25 MB, 6.3 vs
// 7.2 TB/s incremental: scripts/probes/attn_load_pattern_probe.hip, profiles/r05_attn_load_pattern_probe.log; the fp32 cache's
// 384-byte rows already are whole lines and measure like a contiguous stream).  Two consecutive rows starting at an EVEN key are
// 384 bytes = three whole lines, so 8 lanes x 3 loads take a pair (A, B): lane p of the group reads the p-th 16 bytes of line j.
// In units of 8-half chunks ("parts" 0..11 of a row):
//     load 0: row A part p          load 1: p < 4 ? row A part 8 + p : row B part p - 4          load 2: row B part 4 + p
// Scores: a = t0 + (p < 4 ? t1 : 0), b = (p < 4 ? 0 : t1) + t2 summed over the 8 lanes; weights: pA on load 0, pA / pB on load 1,
// pB on load 2.  Every part is accumulated by two (lane, load) slots 4 lanes apart; hpair_fold() adds them with row_ror:4.
struct HPair {
    int p; bool lo; int part1;
    __device__ __forceinline__ explicit HPair(int lane) : p(lane & 7), lo((lane & 7) < 4), part1((lane & 7) < 4 ? 8 + (lane & 7) : (lane & 7) - 4) {}
};

__device__ __forceinline__ void hpair_load_q(const float* qp, const HPair& hp, float (&qv)[3][8]) {
    const int part[3] = {hp.p, hp.part1, 4 + hp.p};
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int e = 0; e < 8; e += 4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(qp + part[j] * 8 + e);
            qv[j][e] = t.x; qv[j][e + 1] = t.y; qv[j][e + 2] = t.z; qv[j][e + 3] = t.w;
        }
}
// rA / rB: the rows this lane reads for key A / key B of its pair (a masked key reads a valid row: its weight is 0)
__device__ __forceinline__ void hpair_load(const _Float16* base, int rA, int rB, const HPair& hp, f32x4 (&r)[3]) {
    r[0] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (long long)rA * 96 + hp.p * 8));
    r[1] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (long long)(hp.lo ? rA : rB) * 96 + hp.part1 * 8));
    r[2] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (long long)rB * 96 + (4 + hp.p) * 8));
}
__device__ __forceinline__ float hpair_dot8(const f32x4& raw, const float (&q)[8]) {
    float f[8];
    kv_unpack<_Float16>(raw, f);
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(q[e], f[e], acc);
    return acc;
}
__device__ __forceinline__ void hpair_scores(const f32x4 (&k)[3], const float (&qv)[3][8], const HPair& hp, float& sA, float& sB) {
    const float t0 = hpair_dot8(k[0], qv[0]), t1 = hpair_dot8(k[1], qv[1]), t2 = hpair_dot8(k[2], qv[2]);
    sA = lane_group_sum<8>(t0 + (hp.lo ? t1 : 0.f));
    sB = lane_group_sum<8>((hp.lo ? 0.f : t1) + t2);
}
__device__ __forceinline__ void hpair_accum(const f32x4 (&v)[3], float pA, float pB, const HPair& hp, float (&o)[3][8]) {
    const float w[3] = {pA, hp.lo ? pA : pB, pB};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float f[8];
        kv_unpack<_Float16>(v[j], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[j][e] = fmaf(w[j], f[e], o[j][e]);
    }
}
// o[j][e] already summed over the two lane groups of the row of 16 (o += row_ror<8>(o)): main = part p (all 8 lanes), hi = part 8 + p
// (lanes p < 4 only)
__device__ __forceinline__ void hpair_fold(const float (&o)[3][8], const HPair& hp, float (&main)[8], float (&hi)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        main[e] = o[0][e] + row_ror<4>(hp.lo ? o[2][e] : o[1][e]);     // a lane hands its receiver (4 lanes below) what THAT lane lacks
        hi[e] = o[1][e] + row_ror<4>(o[2][e]);
    }
}

// ---- the lane mapping.  A wave-step is one round of loads of a wave: KPW keys, GL lanes per group of keys, NK keys per lane (their
// scores and weights travel as float[NK]), NV 16-byte loads per lane and cache (f32x4[NV]; q and o registers are float[NV][EPL]).
//
// ROW mapping: LPK lanes cover one key row with NV 16-byte loads each (full 128-byte lines per wave-instruction), lane group g of a
// wave-step holds its key g; lane p of the group owns dims (j * LPK + p) * EPL .. + EPL of load j.
template <typename KT, int D, bool PAIR = (sizeof(KT) == 2 && D == 96)>
struct KMap {
    static constexpr int EPL = KVec<KT>::EPL, LPK = KVec<KT>::LPK;
    static constexpr int NV = D / (EPL * LPK);
    static constexpr int KPW = 64 / LPK, NK = 1, GL = LPK;
    static_assert(D % (EPL * LPK) == 0, "head_dim must tile into 16-byte loads");
    int p, g;
    __device__ __forceinline__ explicit KMap(int lane) : p(lane & (LPK - 1)), g(lane / LPK) {}
    // the first of this lane's NK consecutive keys, counted from the first key of the wave-step
    __device__ __forceinline__ int key0() const { return g; }
    // true in one lane per key: the lane that adds the key's weight to the softmax denominator
    __device__ __forceinline__ bool counts() const { return p == 0; }
    __device__ __forceinline__ void load_q(const float* qp, float (&qv)[NV][EPL]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; e += 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(qp + (j * LPK + p) * EPL + e);
                qv[j][e] = t.x; qv[j][e + 1] = t.y; qv[j][e + 2] = t.z; qv[j][e + 3] = t.w;
            }
    }
    // this lane's 16-byte pieces of the K (or V) rows row[] (the caller has already replaced out-of-range rows by a row it may read);
    // the lane's offset leads the address so that it stays out of the per-row arithmetic
    __device__ __forceinline__ void load(const KT* base, const int (&row)[NK], f32x4 (&r)[NV]) const {
        const f32x4* src = reinterpret_cast<const f32x4*>(base) + p + (long long)row[0] * (NV * LPK);
#pragma unroll
        for (int j = 0; j < NV; ++j) r[j] = __builtin_nontemporal_load(src + j * LPK);
    }
    // q.k / sqrt(D) of the lane's keys (every lane of a key's lane group ends up holding its score), -inf where !valid.
    // S is float or const float&: same bits, different code.  By value hipcc divides in every lane and selects; by reference the divisor
    // is read only where the key is valid and the division stays under that branch - the form attn_decode3_kernel was tuned in.
    __device__ __forceinline__ void dots(const f32x4 (&k)[NV], const float (&qv)[NV][EPL], float (&s)[NK]) const {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float kf[EPL];
            kv_unpack<KT>(k[j], kf);
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc = fmaf(qv[j][e], kf[e], acc);
        }
        s[0] = lane_group_sum<LPK>(acc);
    }
    static __device__ __forceinline__ float wsum(const float (&w)[NK]) { return w[0]; }
    // o += sum over the lane's keys of w * V
    __device__ __forceinline__ void accum(const f32x4 (&v)[NV], const float (&w)[NK], float (&o)[NV][EPL]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            float vf[EPL];
            kv_unpack<KT>(v[j], vf);
#pragma unroll
            for (int e = 0; e < EPL; ++e) o[j][e] = fmaf(w[0], vf[e], o[j][e]);
        }
    }
    // key groups sit LPK lanes apart: add them inside each row of 16 lanes with DPP rotations (VALU, no LDS crossbar); the four rows of
    // a wave are left to the LDS merge (round 2a did all of it with 36 / 96 ds_bpermutes per lane)
    __device__ __forceinline__ void fold_rows(float (&o)[NV][EPL]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                o[j][e] += row_ror<8>(o[j][e]);
                if (LPK == 4) o[j][e] += row_ror<4>(o[j][e]);
            }
    }
    // o summed over the key groups: the D floats dst[0 .. D) from the GL lanes of a group (active: this lane is one of them)
    __device__ __forceinline__ void store(const float (&o)[NV][EPL], float* dst, bool active) const {
        if (active) {
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int e = 0; e < EPL; ++e) dst[(j * LPK + p) * EPL + e] = o[j][e];
        }
    }
};

// PAIR mapping (see HPair above): 8 lanes x 3 loads take the two rows of an even key and its successor.
template <typename KT, int D>
struct KMap<KT, D, true> {
    static_assert(sizeof(KT) == 2 && D == 96, "pair mapping: 96 halves per row");
    static constexpr int EPL = 8, NV = 3;
    static constexpr int KPW = 16, NK = 2, GL = 8;
    HPair hp; int g;
    __device__ __forceinline__ explicit KMap(int lane) : hp(lane), g(lane >> 3) {}
    __device__ __forceinline__ int key0() const { return 2 * g; }
    __device__ __forceinline__ bool counts() const { return hp.p == 0; }
    __device__ __forceinline__ void load_q(const float* qp, float (&qv)[NV][EPL]) const { hpair_load_q(qp, hp, qv); }
    __device__ __forceinline__ void load(const KT* base, const int (&row)[NK], f32x4 (&r)[NV]) const { hpair_load(base, row[0], row[1], hp, r); }
    __device__ __forceinline__ void dots(const f32x4 (&k)[NV], const float (&qv)[NV][EPL], float (&s)[NK]) const { hpair_scores(k, qv, hp, s[0], s[1]); }
    static __device__ __forceinline__ float wsum(const float (&w)[NK]) { return w[0] + w[1]; }
    __device__ __forceinline__ void accum(const f32x4 (&v)[NV], const float (&w)[NK], float (&o)[NV][EPL]) const { hpair_accum(v, w[0], w[1], hp, o); }
    __device__ __forceinline__ void fold_rows(float (&o)[NV][EPL]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; ++e) o[j][e] += row_ror<8>(o[j][e]);
    }
    // every part sits in two (lane, load) slots 4 lanes apart: all lanes fold, the GL lanes of a group store
    __device__ __forceinline__ void store(const float (&o)[NV][EPL], float* dst, bool active) const {
        float om[8], oh[8];
        hpair_fold(o, hp, om, oh);
        if (active) {
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[hp.p * 8 + e] = om[e];
            if (hp.lo) {
#pragma unroll
                for (int e = 0; e < 8; ++e) dst[(8 + hp.p) * 8 + e] = oh[e];
            }
        }
    }
};

// ---- byte cache (kv8 mode, one e4m3fn byte per element, D = 96): lanes mapped over QUADS of key rows.
//
// A byte row is 96 bytes, three quarters of a line; four consecutive rows from a key that is a multiple of 4 are three whole lines, so
// 8 lanes x 3 loads take a quad the way the PAIR mapping takes two fp16 rows: lane p of load j reads the p-th 16 bytes of line j, which is
// piece (8 j + p) % 6 of row (8 j + p) / 6.  The index arithmetic - slot -> (row, piece), which slots make up a score, how the fold adds
// the four slots of a piece - is er_kv8_map.h, enumerated on the host by tests/host/kv8_map_check.cpp.  Every slot takes the row index
// of its own row (a masked key reads a valid row and gets weight 0; 0 x NaN is never formed, so the unused tail may hold anything).
typedef unsigned char kv8_t;

// 16 e4m3 bytes (element k of the load in byte k) as floats: two packed conversions per dword, as k_gemv.h dot_w8
__device__ __forceinline__ void kv8_unpack(const f32x4& raw, float (&f)[16]) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const int w[4] = {__float_as_int(raw.x), __float_as_int(raw.y), __float_as_int(raw.z), __float_as_int(raw.w)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false), b = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
        f[4 * i] = a.x; f[4 * i + 1] = a.y; f[4 * i + 2] = b.x; f[4 * i + 3] = b.y;
    }
}

// v of lane (l + K) mod 8 of the lane's group of 8, for a value that both groups of a row of 16 lanes hold alike (after fold_rows):
// row_ror:N hands lane l the value of lane (l - N) mod 16
template <int K>
__device__ __forceinline__ float quad_from_above(float v) { return row_ror<8 - K>(v); }

template <int D>
struct KMap<kv8_t, D, false> {
    static_assert(D == kv8::D, "quad mapping: 96 bytes per row");
    static constexpr int EPL = kv8::EPL, NV = kv8::NV;
    static constexpr int KPW = kv8::KPW, NK = kv8::ROWS, GL = kv8::GL;
    int p, g;
    bool lo[NV];       // load j holds row j (else row j + 1) in this lane
    int piece[NV];     // and this piece of it
    __device__ __forceinline__ explicit KMap(int lane) : p(lane & 7), g(lane >> 3) {
#pragma unroll
        for (int j = 0; j < NV; ++j) { lo[j] = p < kv8::load_split(j); piece[j] = kv8::load_piece(j, p); }
    }
    __device__ __forceinline__ int key0() const { return NK * g; }
    __device__ __forceinline__ bool counts() const { return p == 0; }
    __device__ __forceinline__ void load_q(const float* qp, float (&qv)[NV][EPL]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; e += 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(qp + piece[j] * EPL + e);
                qv[j][e] = t.x; qv[j][e + 1] = t.y; qv[j][e + 2] = t.z; qv[j][e + 3] = t.w;
            }
    }
    __device__ __forceinline__ void load(const kv8_t* base, const int (&row)[NK], f32x4 (&r)[NV]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j)
            r[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (long long)(lo[j] ? row[j] : row[j + 1]) * D + piece[j] * EPL));
    }
    static __device__ __forceinline__ float dot16(const f32x4& raw, const float (&q)[EPL]) {
        float f[EPL];
        kv8_unpack(raw, f);
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc = fmaf(q[e], f[e], acc);
        return acc;
    }
    __device__ __forceinline__ void dots(const f32x4 (&k)[NV], const float (&qv)[NV][EPL], float (&s)[NK]) const {
        const float t[NV] = {dot16(k[0], qv[0]), dot16(k[1], qv[1]), dot16(k[2], qv[2])};
#pragma unroll
        for (int r = 0; r < NK; ++r) {         // row r: what kv8::score_takes names of the loads that can hold it (r - 1 and r)
            float acc = 0.f;
            bool first = true;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                if (!kv8::score_load(r, j)) continue;
                const float term = kv8::score_takes(r, j, p) ? t[j] : 0.f;
                acc = first ? term : acc + term;
                first = false;
            }
            s[r] = lane_group_sum<8>(acc);
        }
    }
    // the accumulator kv8::fold_load(I, p) names for fold term I of this lane: one of two registers, picked by a select (no indexing)
    template <int I>
    __device__ __forceinline__ float fold_term(const float (&o)[NV][EPL], int e) const {
        constexpr int A = kv8::fold_load(I, 0), B = kv8::fold_load(I, GL - 1);
        static_assert(kv8::fold_load_two_valued(I), "a fold term sends one of two accumulators");
        if constexpr (A == B) return o[A][e];
        else return kv8::fold_load(I, p) == A ? o[A][e] : o[B][e];
    }
    static __device__ __forceinline__ float wsum(const float (&w)[NK]) { return (w[0] + w[1]) + (w[2] + w[3]); }
    __device__ __forceinline__ void accum(const f32x4 (&v)[NV], const float (&w)[NK], float (&o)[NV][EPL]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float wj = lo[j] ? w[j] : w[j + 1];
            float f[EPL];
            kv8_unpack(v[j], f);
#pragma unroll
            for (int e = 0; e < EPL; ++e) o[j][e] = fmaf(wj, f[e], o[j][e]);
        }
    }
    __device__ __forceinline__ void fold_rows(float (&o)[NV][EPL]) const {
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < EPL; ++e) o[j][e] += row_ror<8>(o[j][e]);
    }
    // every piece sits in four (lane, load) slots 2 lanes apart: all lanes fold - term i is the accumulator kv8::fold_load(i, sender)
    // of the lane kv8::fold_shift(i) above - and the lanes kv8::fold_stores names store their piece (active: the row's first group)
    __device__ __forceinline__ void store(const float (&o)[NV][EPL], float* dst, bool active) const {
        static_assert(kv8::FOLD_TERMS == 4 && kv8::fold_shift(0) == 0, "the fold is written out for its four terms");
        float om[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            const float s1 = quad_from_above<kv8::fold_shift(1)>(fold_term<1>(o, e));
            const float s2 = quad_from_above<kv8::fold_shift(2)>(fold_term<2>(o, e));
            const float s3 = quad_from_above<kv8::fold_shift(3)>(fold_term<3>(o, e));
            om[e] = (fold_term<0>(o, e) + s1) + (s2 + s3);
        }
        if (active && kv8::fold_stores(p)) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) dst[kv8::store_piece(p) * EPL + e] = om[e];
        }
    }
};

// the wave's accumulators as four rows of D floats (one per row of 16 lanes) at ored[(wid * 4 + row) * LD]
template <int LD, typename M>
__device__ __forceinline__ void attn_fold_store(const M& m, float (&o)[M::NV][M::EPL], float* ored, int wid, int lane) {
    m.fold_rows(o);
    m.store(o, ored + (wid * 4 + (lane >> 4)) * LD, (lane & 15) < M::GL);
}

// ---- the wave pass of the per-wave-softmax kernels (attn_decode2_kernel, attn_decode3_kernel).  A workgroup of NW waves owns keys
// [k0, k1); wave-step i of wave wid covers the KPW keys from k0 + (i * NW + wid) * KPW.  Every K load, then every V load (K returns
// first, V lands while the scores are reduced), all of them issued before the first score is computed; the wave's own softmax (max and
// sum through shuffles only); the weighted V sum folded to rows of 16 lanes at ored[(wid * 4 + row) * LD] and the wave's {m, l} in
// wm[wid] / wl[wid] (m = -inf when the wave holds no valid key: the ragged tail of a chunk).  The caller's barrier comes next.
// A key past k1 is masked (weight 0) and reads row k0 instead, which the chunk always holds.  `a` is the kernel's argument struct (for
// sqrt_d, read where a score is valid).
//
// The statements are in the order, and the score mask in the written-out form, that the kernels were tuned in: hipcc decides early
// whether `valid ? d / sqrt_d : -inf` becomes a branch or a select, and a loop over the lane's keys, a helper around the division or
// one more function between a kernel and this pass each moves an instantiation by a register or a few dozen instructions
// (the bits are the same in every form).
template <typename KT, int D, int NS, int NW, int LD, typename A>
__device__ __forceinline__ void attn_wave_pass(const A& a, const KT* kb, const KT* vb, const float (&qv)[KMap<KT, D>::NV][KMap<KT, D>::EPL],
                                               int k0, int k1, float* ored, float* wm, float* wl) {
    using M = KMap<KT, D>;
    constexpr int NV = M::NV, EPL = M::EPL, NK = M::NK, KPW = M::KPW;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const M m(lane);
    f32x4 kreg[NS][NV], vreg[NS][NV];
    bool valid[NS][NK];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        int row[NK];
#pragma unroll
        for (int n = 0; n < NK; ++n) {
            const int kk = k0 + (i * NW + wid) * KPW + m.key0() + n;
            valid[i][n] = kk < k1;
            row[n] = valid[i][n] ? kk : k0;
        }
        m.load(kb, row, kreg[i]);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int kk = k0 + (i * NW + wid) * KPW + m.key0();
        int row[NK];
#pragma unroll
        for (int n = 0; n < NK; ++n) row[n] = valid[i][n] ? kk + n : k0;
        m.load(vb, row, vreg[i]);
    }
    __builtin_amdgcn_sched_barrier(0);        // every K and V load is issued before the first score is computed
    ER_TP(2);

    float sc[NS][NK];
    float mloc = -INFINITY;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        float d[NK];
        m.dots(kreg[i], qv, d);
        if constexpr (NK == 2) {                  // written out per key, see above
            sc[i][0] = valid[i][0] ? d[0] / a.sqrt_d : -INFINITY;
            sc[i][1] = valid[i][1] ? d[1] / a.sqrt_d : -INFINITY;
            mloc = fmaxf(mloc, fmaxf(sc[i][0], sc[i][1]));
        } else if constexpr (NK == 4) {           // the quad mapping's four keys, written out the same way
            sc[i][0] = valid[i][0] ? d[0] / a.sqrt_d : -INFINITY;
            sc[i][1] = valid[i][1] ? d[1] / a.sqrt_d : -INFINITY;
            sc[i][2] = valid[i][2] ? d[2] / a.sqrt_d : -INFINITY;
            sc[i][3] = valid[i][3] ? d[3] / a.sqrt_d : -INFINITY;
            mloc = fmaxf(mloc, fmaxf(fmaxf(sc[i][0], sc[i][1]), fmaxf(sc[i][2], sc[i][3])));
        } else {
            sc[i][0] = valid[i][0] ? d[0] / a.sqrt_d : -INFINITY;
            mloc = fmaxf(mloc, sc[i][0]);
        }
    }
    const float mw = wave_max(mloc);          // -inf when the wave holds no valid key
    ER_TP(3);
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
    ER_TP(4);
    attn_fold_store<LD>(m, o, ored, wid, lane);
    if (lane == 0) { wm[wid] = mw; wl[wid] = l; }
}

// ---- the four-wave merge of a 256-thread workgroup: column tid (< D) of the waves' row partials ored[wave][row of 16 lanes][D],
// weighed with exp(m_wave - M).  M is finite: the workgroup holds at least one key.
template <int D>
__device__ __forceinline__ void attn_merge4(const float* ored, const float* wm, const float* wl, int tid, float& ov, float& lv, float& M) {
    M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    ov = 0.f; lv = 0.f;
#pragma unroll
    for (int k = 0; k < ER_NWAVES; ++k) {
        const float w = (wm[k] == -INFINITY) ? 0.f : expf(wm[k] - M);
        const float* src = ored + k * 4 * D + tid;
        ov = fmaf((src[0] + src[D]) + (src[2 * D] + src[3 * D]), w, ov);
        lv = fmaf(wl[k], w, lv);
    }
}

}  // namespace er
