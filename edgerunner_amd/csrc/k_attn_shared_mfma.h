// The prefix pass of the shared-prefix decode attention (k_attn_shared.h) on the fp16 matrix cores, for fp16 caches at head_dim 96:
// attn_prefix_kernel's grid, chunks and partials, with the rows of a group as MFMA columns instead of a loop over rows on the VALU.
//
//   grid (H, ceil(P / 128), groups), 256 threads.  Wave w owns keys k0 + 32 w .. + 31 of the LEADER's chunk and keeps them in registers
//   for the whole workgroup: K as the A operand of S^T = K Q^T straight from global memory (lane (li, half) holds 16 bytes of key li per
//   16-dim step: 6 steps, 24 VGPRs), V^T as the A operand of O^T = V^T P^T through a transposed fp16 LDS image that is read once
//   (fa_vt_frag: 3 blocks of 32 dims x 2 steps of 16 keys, 24 VGPRs).  The group's rows are walked in tiles of 32, one row per column:
//   q x 2^4 and p x 2^10 split into hi + lo fp16 (flash_attn_f16s_kernel's scheme and scales: fp16 x fp16 products are exact in the fp32
//   accumulator and the scales keep the lo parts out of the fp16 subnormals), 12 + 12 v_mfma_f32_32x32x16_f16 per wave and tile, the
//   wave's own softmax per column (one xor-32 exchange: a column is a lane pair), and the four waves' {m, l, o[96]} of every row merged
//   through LDS with attn_merge4's weights into the partial attn_suffix_merge_kernel reads.
//
// Row invariance: a column of either product depends on that column of the B operand alone, the softmax statistics are per column and
// the merge is per (row, dim), so a row's partial bits follow from its q and the chunk's K/V bits - not from the size of its group, its
// place in it, the rows in the other columns of its tile (pad columns take q = 0 and are never stored) or the other groups (a workgroup
// serves one group).  A key >= P loads row k0 of the chunk (always a prefix row of the leader) and gets weight 0 by selection, never by
// a product; a follower's cache is not addressed at all.
//
// 190 VGPRs (two workgroups per CU), 52 224 B of LDS, no scratch (-save-temps).  Measured (DESIGN.md section 6, 24 layers, B = 32, L = 2550):
// with 32 rows of one cloud the pass falls from 68 to about 10 us per layer and the fp16 step gains where the VALU pass lost; with 32
// singletons - one workgroup per (row, head, chunk) again, every one paying the transposition and 24 MFMAs for ONE live column - it is
// slower than the VALU pass (102 against 74 us), which is why the VALU pass stays the default.  Tried and dropped: nontemporal K/V loads (a lane's 16-byte
// pieces of a key row come from six instructions that hit the same lines: singletons 99 -> 141 us), a three-waves-per-SIMD bound
// (168 VGPRs spill).
#pragma once
#include "k_attn_shared.h"
#include "k_flash_attn_f16s.h"

namespace er {

constexpr int ASM_VLD = 32 + 8;         // halves per row of a wave's V^T image [d][key] (fa_vt_frag: VLD / 8 odd)
constexpr int ASM_OLD = 96 + 4;         // floats per row of a wave's merge image [row of the tile][d]

template <int D>
__global__ __launch_bounds__(ER_WG) void attn_prefix_mfma_kernel(AttnSharedArgs s) {
    static_assert(D == 96 && ER_NWAVES * 32 == ATTN_SHARED_CHUNK, "four waves of 32 keys cover one chunk of head_dim 96");
    constexpr int KS = D / 16, NDB = D / 32, W = D + 2;
    constexpr int VT_HALVES = D * ASM_VLD, O_FLOATS = 32 * ASM_OLD;
    static_assert(VT_HALVES * 2 <= O_FLOATS * 4, "the V^T image fits into the merge image it is replaced by");
    // per wave: first the V^T image (read once into registers), then the merge image of every row tile
    __shared__ __attribute__((aligned(16))) float ored[ER_NWAVES][O_FLOATS];
    __shared__ float wm[ER_NWAVES][32], wl[ER_NWAVES][32];
    const AttnDecArgs& a = s.a;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const int h = blockIdx.x, c = blockIdx.y, g = blockIdx.z;      // heads fastest, as attn_prefix_kernel
    // small operands first: the group's rows and the first tile's q, then the K/V stream
    const int r0 = s.grp_off[g], r1 = s.grp_off[g + 1];
    const int leader = s.grp_rows[r0];
    float qv[KS][8];                   // B operand of S^T before its split: row t0 + li, dims 16 ks + 8 half + {0..7}
    bool qlive;                        // a pad column (no row) loads the leader's q and takes q = 0 at the split
    const auto load_q = [&](int t0) {
        qlive = t0 + li < r1;
        const float* qr = a.q + (long long)s.grp_rows[qlive ? t0 + li : r0] * a.hidden + h * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) fa_q8(qr, ks, half, qv[ks]);
    };
    load_q(r0);
    const int k0 = c * ATTN_SHARED_CHUNK, k1 = min(s.prefix_len, k0 + ATTN_SHARED_CHUNK);      // k0 < P
    const int kw0 = k0 + 32 * wid;                                                             // this wave's first key
    const long long head_off = (long long)leader * a.kv_bstride + (long long)h * a.l_cap * D;
    const _Float16* kb = reinterpret_cast<const _Float16*>(a.kcache) + head_off;
    const _Float16* vb = reinterpret_cast<const _Float16*>(a.vcache) + head_off;
    fa_h8 kf[KS];                      // A operand of S^T: key kw0 + li, dims 16 ks + 8 half + {0..7}
    {
        const int gk = kw0 + li < k1 ? kw0 + li : k0;      // a masked key reads row k0, which the chunk always holds
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const fa_h8*>(kb + (long long)gk * D + ks * 16 + half * 8);
    }
    // V: the same lane -> (key, 16 bytes) map, so that a transposing store of a wave goes to 32 consecutive halves of two rows 8 apart
    // (row stride 20 words: the two lane halves land 32 banks apart)
    fa_h8 vst[KS];
    {
        const int gk = kw0 + li < k1 ? kw0 + li : k0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) vst[ks] = *reinterpret_cast<const fa_h8*>(vb + (long long)gk * D + ks * 16 + half * 8);
    }
    _Float16* Vt = reinterpret_cast<_Float16*>(ored[wid]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(ks * 16 + half * 8 + e) * ASM_VLD + li] = vst[ks][e];
    __syncthreads();
    fa_h8 vf[2][NDB];                  // A operand of O^T: dim 32 db + li, the 16-key step's keys of this lane half (fa_vt_frag)
#pragma unroll
    for (int stp = 0; stp < 2; ++stp)
#pragma unroll
        for (int db = 0; db < NDB; ++db) vf[stp][db] = fa_vt_frag<ASM_VLD>(Vt, db * 32 + li, 16 * stp + 4 * half);
    __syncthreads();                   // the image is consumed: the first tile's merge image may replace it

    const float sdiv = a.sqrt_d * FAS_QSCALE;      // sqrt(D) times a power of two: fa_softmax_exact's three-instruction division stays exact
    const float inv_sdiv = 1.0f / sdiv;
    bool valid[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) valid[r] = kw0 + fa_row(r, half) < k1;

    // the four-wave merge of tile t0 with attn_merge4's weights: eight threads per row, twelve dims each
    const auto merge_tile = [&](int t0) {
        const int row = tid >> 3, d0 = tid & 7;
        if (t0 + row >= r1) return;
        const float m0 = wm[0][row], m1 = wm[1][row], m2 = wm[2][row], m3 = wm[3][row];
        const float mx = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));      // finite: the chunk holds at least one key
        float wgt[ER_NWAVES];
        wgt[0] = (m0 == -INFINITY) ? 0.f : expf(m0 - mx);
        wgt[1] = (m1 == -INFINITY) ? 0.f : expf(m1 - mx);
        wgt[2] = (m2 == -INFINITY) ? 0.f : expf(m2 - mx);
        wgt[3] = (m3 == -INFINITY) ? 0.f : expf(m3 - mx);
        const int b = s.grp_rows[t0 + row];
        float* pout = a.part + (((long long)b * a.H + h) * a.S + c) * W;
#pragma unroll
        for (int j = 0; j < D / 8; ++j) {
            const int d = d0 + 8 * j;
            float ov = 0.f;
#pragma unroll
            for (int k = 0; k < ER_NWAVES; ++k) ov = fmaf(ored[k][row * ASM_OLD + d], wgt[k], ov);
            pout[2 + d] = ov;
        }
        if (d0 == 0) {
            float lv = 0.f;
#pragma unroll
            for (int k = 0; k < ER_NWAVES; ++k) lv = fmaf(wl[k][row], wgt[k], lv);
            pout[0] = mx;
            pout[1] = lv;
        }
    };

    for (int t0 = r0;; t0 += 32) {
        // S^T = K Q^T: lane (li, half) holds keys kw0 + fa_row(r, half) of row t0 + li
        fa_acc st;
        fa_zero(st);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            fa_h8 qh, ql;              // hi + lo fp16 parts of 2^4 q, split step by step: q stays 48 registers, not 48 + 48
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = qlive ? qv[ks][e] * FAS_QSCALE : 0.f;
                const _Float16 hi = (_Float16)x;
                qh[e] = hi;
                ql[e] = (_Float16)(x - (float)hi);
            }
            st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], ql, st, 0, 0, 0);      // small parts first
            st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qh, st, 0, 0, 0);
        }
        // the wave's softmax of the row: scores divided by sqrt(D) (correctly rounded, k_flash_lanes.h), weights expf(s - m)
        float mloc = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float q0 = st[r] * inv_sdiv;
            const float sc = valid[r] ? fmaf(fmaf(-q0, sdiv, st[r]), inv_sdiv, q0) : -INFINITY;
            st[r] = sc;
            mloc = fmaxf(mloc, sc);
        }
        const float mw = xor_max<32>(mloc);      // -inf when the wave holds no valid key (the ragged last chunk)
        float lloc = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = valid[r] ? expf(st[r] - mw) : 0.f;
            st[r] = p;
            lloc += p;
        }
        const float l = xor_sum<32>(lloc);
        // O^T = V^T P^T: P^T is S^T's registers (8 per 16-key step), as hi + lo parts of 2^10 p
        fa_acc ot[NDB];
        fa_zero(ot);
#pragma unroll
        for (int stp = 0; stp < 2; ++stp) {
            fa_h8 ph, pl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = st[8 * stp + e] * FAS_PSCALE;
                const _Float16 hi = (_Float16)x;
                ph[e] = hi;
                pl[e] = (_Float16)(x - (float)hi);
            }
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                ot[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[stp][db], pl, ot[db], 0, 0, 0);
                ot[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[stp][db], ph, ot[db], 0, 0, 0);
            }
        }
        // the wave's part of every row: ored[wid][row][d] (registers 4 g .. 4 g + 3 are dims 32 db + 8 g + 4 half + {0..3})
        float* orow = ored[wid] + li * ASM_OLD;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 v;
                v.x = ot[db][4 * gq + 0] * (1.0f / FAS_PSCALE);
                v.y = ot[db][4 * gq + 1] * (1.0f / FAS_PSCALE);
                v.z = ot[db][4 * gq + 2] * (1.0f / FAS_PSCALE);
                v.w = ot[db][4 * gq + 3] * (1.0f / FAS_PSCALE);
                *reinterpret_cast<f32x4*>(orow + db * 32 + 8 * gq + 4 * half) = v;
            }
        if (half == 0) { wm[wid][li] = mw; wl[wid][li] = l; }
        if (t0 + 32 >= r1) {                    // workgroup-uniform: the group's last tile
            __syncthreads();
            merge_tile(t0);
            break;
        }
        __builtin_amdgcn_sched_barrier(0);      // behind the stores of O^T: its registers are free for the next q
        load_q(t0 + 32);                        // the next tile's q travels while this tile is merged
        __syncthreads();
        merge_tile(t0);
        __syncthreads();                        // the next tile's merge image replaces this one
    }
}

// kind 1 of a plan with shared_mfma; the suffix / merge launch (launch_attn_suffix_merge_d, kv_half) follows unchanged
template <int D>
inline hipError_t launch_attn_prefix_mfma_d(const AttnSharedArgs& s, int groups, hipStream_t st) {
    if (s.prefix_len < 1 || s.prefix_len > s.a.l_cap || s.a.S != attn_shared_chunks(s.prefix_len) || groups < 1 || groups > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((attn_prefix_mfma_kernel<D>), dim3(s.a.H, s.a.S, groups), dim3(ER_WG), 0, st, s);
    return hipGetLastError();
}

}  // namespace er
