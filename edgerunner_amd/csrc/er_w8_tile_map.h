// The tiled copy of an fp8-mode byte matrix, as the matrix-core batched projections stream it (k_gemv_mfma.h, WT = w8_t): where weight
// (n, k) of the row-major block [N][K] lives, written once for the kernel that tiles (tile_weights_kernel), the kernel that streams
// (gemv_mfma_kernel) and the host check that enumerates both (tests/host/w8_tile_check.cpp; er_gemm_map.h is the precedent).
//
// The fp16 tiled copy is [N/16][K/32] tiles of 64 pieces x 16 bytes, piece number = the lane that consumes it: lane (li = lane & 15,
// kq = lane >> 4) holds the eight weights k = 32 kt + 8 kq .. + 7 of row 16 nt + li.  A byte piece is 8 bytes, so the byte copy PAIRS
// the two 16-row tiles a workgroup reads: [N/32][K/32] tiles of 64 pieces x 16 bytes, the piece of lane (li, kq) holding the same eight
// k of row 32 np + li in its low 8 bytes (row tile t = 0) and of row 32 np + 16 + li in its high 8 bytes (t = 1).  A wave-load is one
// contiguous KiB as before and a lane issues 3 loads for its 96-wide K-slice instead of 6.  N is padded to a multiple of 32 with zero
// rows; the row scales follow the tiles as fp32, padded with 1: ONE block and one pointer, like the row-major byte block (k_gemv.h
// w8_scales).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ER_W8T_FN __host__ __device__ __forceinline__
#else
#define ER_W8T_FN inline
#endif

namespace er {

constexpr int W8T_ROWS = 32, W8T_K = 32, W8T_PIECE = 16;      // rows and k per tile; bytes per piece

ER_W8T_FN long long w8t_rows(int N) { return ((long long)N + W8T_ROWS - 1) / W8T_ROWS * W8T_ROWS; }      // rows with the padding
ER_W8T_FN long long w8t_pieces(int N, int K) { return w8t_rows(N) / W8T_ROWS * (K / W8T_K) * 64; }
ER_W8T_FN size_t w8t_block_bytes(int N, int K) { return (size_t)w8t_rows(N) * K + (size_t)w8t_rows(N) * sizeof(float); }
ER_W8T_FN const float* w8t_scales(const void* w, int N, int K) {
    return reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(w) + w8t_rows(N) * K);
}

// the piece lane `lane` of a wave loads for the rows 32 np .. + 31 and the k 32 kt .. + 31 (index in pieces of 16 bytes)
ER_W8T_FN long long w8t_piece(int K, int np, int kt, int lane) { return ((long long)np * (K / W8T_K) + kt) * 64 + lane; }

// what piece p holds: bytes 0..7 = row n_lo, bytes 8..15 = row n_lo + 16, both k0 .. k0 + 7 (rows >= N are padding)
ER_W8T_FN void w8t_piece_source(int K, long long p, int* n_lo, int* k0) {
    const int lane = (int)(p & 63), KT = K / W8T_K;
    const long long tile = p >> 6;
    const int np = (int)(tile / KT), kt = (int)(tile - (long long)np * KT);
    *n_lo = np * W8T_ROWS + (lane & 15);
    *k0 = kt * W8T_K + (lane >> 4) * 8;
}

// byte offset of weight (n, k) in the tiled copy: the inverse of w8t_piece_source, stated on its own
ER_W8T_FN long long w8t_offset(int K, int n, int k) {
    const int np = n >> 5, t = (n >> 4) & 1, li = n & 15, kt = k >> 5, kq = (k >> 3) & 3, j = k & 7;
    return w8t_piece(K, np, kt, kq * 16 + li) * W8T_PIECE + t * 8 + j;
}

}   // namespace er
