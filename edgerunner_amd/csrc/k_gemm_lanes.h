// What the GEMM kernels (k_gemm.h, k_gemm_stream.h) have in common on the device, written once: the accumulator block of a wave and
// its zeroing, the MFMA step over it (fp16 and fp32 inputs), and - for the kernels whose operands arrive by LDS-DMA in the swizzled
// 128-byte row image of er_gemm_map.h - the per-lane source offset of a piece and the fragment reads.  The bit-equality the kernels
// promise each other (f32 == f32d, f16 == hh == hh256 == stream, f16s == hh split) rests on these steps being the same ones.
// Nothing here issues a vector-memory operation: the LDS-DMA kernels count their vmcnt waits by hand.
#pragma once
#include "er_common.h"
#include "er_gemm_map.h"

namespace er {

typedef float f32x16 __attribute__((ext_vector_type(16)));      // one 32 x 32 fp32 accumulator: 16 registers per lane (rows: mfma32_row)
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

template <int TM, int TN>
__device__ __forceinline__ void gm_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// acc[i][j] += a[i] . b[j]^T over one k-substep: 16 k values on v_mfma_f32_32x32x16_f16 (lane half h holds k = 8 h .. 8 h + 7 of both
// operands), 2 on v_mfma_f32_32x32x2_f32 (lane half h holds k = h).  i outer, j inner: the order every kernel issues them in.
template <int TM, int TN>
__device__ __forceinline__ void gm_mfma_f16(f32x16 (&acc)[TM][TN], const h16x8 (&a)[TM], const h16x8 (&b)[TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
}
template <int TM, int TN>
__device__ __forceinline__ void gm_mfma_f32(f32x16 (&acc)[TM][TN], const float (&a)[TM], const float (&b)[TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
}

// ---- LDS-DMA operands.  A piece is 8 tile rows of 128 bytes = one global_load_lds_dwordx4 of a wave: lane -> (row lane / 8 of the
// piece, LDS slot lane % 8).  Offset (in T elements) of the 16 bytes lane `lane` brings in for tile row r (8 piece + lane / 8) of an
// operand whose tile starts at row row0: the row clamped to `last` (rows beyond the matrix are dropped by the epilogue), and the chunk
// the swizzle puts at that slot.
template <typename T>
__device__ __forceinline__ long long gm_dma_src(int row0, int r, int last, int ld, int lane) {
    return (long long)min(row0 + r, last) * ld + swz_chunk_off<(int)sizeof(T)>(r, lane & 7);
}

// f[b] = the fragment at element offset `off` (swz_frag_off) of row 32 b below rowp, a row of the image being 128 bytes of T
template <typename V, int NB, typename T>
__device__ __forceinline__ void gm_frags(V (&f)[NB], const T* rowp, int off) {
#pragma unroll
    for (int b = 0; b < NB; ++b) f[b] = *reinterpret_cast<const V*>(rowp + 32 * b * (128 / (int)sizeof(T)) + off);
}

}   // namespace er
