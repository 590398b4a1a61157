// The tiled copy of an fp4-mode matrix (MXFP4: er_w4.h), as the matrix-core batched projections stream it (k_gemv_mfma.h, WT = w4_t):
// index arithmetic only, pure constexpr C++ with no device call (er_w8_tile_map.h / er_w4_map.h are the precedents).  The kernel that
// tiles (er_weights.h w4_tile_kernel) and the kernel that streams (gemv_mfma_kernel) are written over these functions and
// tests/host/w4_tile_check.cpp enumerates them on the host.
//
// The unit of work of gemv_mfma_kernel is a workgroup's 32-row tile (two 16-row A tiles, t = 0 / 1) x one wave's 96-wide K-slice.  Lane
// (li = lane & 15, kq = lane >> 4) needs for the steps c = 0, 1, 2 the eight weights k = 96 s + 32 c + 8 kq .. + 7 of the rows
// 32 np + 16 t + li - a PIECE of 4 bytes per (step, row tile), 24 bytes per lane - and the six e8m0 scales of 2 rows x 3 blocks of 32 (a
// step is exactly one scale block, so a piece never straddles one).  One UNIT per (np, s), 1664 bytes = 13 lines of 128:
//     [unit * 1664 +        16 lane + 4 (2 c + t) + byte]   steps c = 0, 1: one 16-byte load per lane, 1 KiB contiguous across the wave
//     [unit * 1664 + 1024 +  8 lane + 4 t + byte]           step c = 2: one 8-byte load per lane, 512 bytes contiguous
//     [unit * 1664 + 1536 +  8 li + 4 t + c]                the scale of block 3 s + c of row 32 np + 16 t + li; c = 3 is padding (0).
//                                                           The four kq lanes of a row share one 8-byte load
//     unit (np, s) = np * (K / 96) + s
// byte `byte` of a piece holds the elements 2 byte (low nibble) and 2 byte + 1 (high nibble) of the piece's eight: the canonical packing.
// N is padded to a multiple of 32 with zero nibbles and the scale byte 127 (2^0); K must be a multiple of 96.  Against 6144 bytes per
// unit for the fp16 tiled copy and 3072 (+ row scales) for the byte copy.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace er {
namespace w4t {

constexpr int ROWS = 32, KW = 96, BLOCK = 32;      // rows and k per unit; elements per scale block
constexpr int STEPS = KW / BLOCK;                  // 3 steps (= scale blocks) per lane and unit
constexpr int PIECE = 4;                           // bytes of a lane's eight weights of one (step, row tile)
constexpr int A_LANE = 16, B_LANE = 8, S_ROW = 8;  // bytes per lane of the two nibble loads; bytes per li of the scale load
constexpr int A_BYTES = 64 * A_LANE, B_BYTES = 64 * B_LANE, S_BYTES = 16 * S_ROW;      // 1024, 512, 128
constexpr int B_BASE = A_BYTES, S_BASE = A_BYTES + B_BYTES;                            // 1024, 1536
constexpr int UNIT_BYTES = S_BASE + S_BYTES;                                           // 1664 = 13 * 128
constexpr int PAD_SCALE = 127;                     // the e8m0 byte of 2^0: what a padded row's scales hold

constexpr bool shape_ok(long long n, long long k) { return n > 0 && k > 0 && k % KW == 0; }
constexpr long long rows(long long n) { return (n + ROWS - 1) / ROWS * ROWS; }      // rows with the padding
constexpr long long units(long long n, long long k) { return rows(n) / ROWS * (k / KW); }
constexpr long long block_bytes(long long n, long long k) { return units(n, k) * UNIT_BYTES; }

constexpr long long unit(int K, long long np, int s) { return np * (K / KW) + s; }
// what lane `lane` of the wave that owns unit u loads: 16 + 8 bytes of nibbles and the 8 scale bytes of its two rows
constexpr long long lane_a_offset(long long u, int lane) { return u * UNIT_BYTES + (long long)lane * A_LANE; }
constexpr long long lane_b_offset(long long u, int lane) { return u * UNIT_BYTES + B_BASE + (long long)lane * B_LANE; }
constexpr long long lane_scale_offset(long long u, int lane) { return u * UNIT_BYTES + S_BASE + (long long)(lane & 15) * S_ROW; }

// byte offset of the byte that holds weight (n, k) - low nibble for an even k, high nibble for an odd one
constexpr long long offset(int K, long long n, long long k) {
    const int t = (int)(n >> 4) & 1, li = (int)(n & 15), s = (int)(k / KW), r = (int)(k % KW), c = r / BLOCK, kq = (r % BLOCK) / 8, byte = (r % 8) / 2;
    const long long u = unit(K, n >> 5, s);
    const int lane = kq * 16 + li;
    return c < 2 ? lane_a_offset(u, lane) + PIECE * (2 * c + t) + byte : lane_b_offset(u, lane) + PIECE * t + byte;
}
// byte offset of the e8m0 scale of block `block` (elements 32 block .. + 31) of row n
constexpr long long scale_offset(int K, long long n, long long block) {
    const int t = (int)(n >> 4) & 1, li = (int)(n & 15);
    return lane_scale_offset(unit(K, n >> 5, (int)(block / STEPS)), li) + PIECE * t + (int)(block % STEPS);
}

// the inverse: what the byte at `off` of the block holds.  WEIGHT: elements k, k + 1 of row n; SCALE: block k of row n (k counts blocks);
// PAD: the fourth byte of a row's scale dword.  Rows n >= N are the padding rows (zero nibbles, PAD_SCALE).
enum Kind { WEIGHT = 0, SCALE = 1, PAD = 2 };
struct What { int kind; long long n; long long k; };
constexpr What what(int K, long long off) {
    const long long u = off / UNIT_BYTES, np = u / (K / KW);
    const int in = (int)(off % UNIT_BYTES), s = (int)(u % (K / KW));
    if (in >= S_BASE) {
        const int q = in - S_BASE, li = q / S_ROW, t = (q % S_ROW) / PIECE, c = q % PIECE;
        const long long n = np * ROWS + 16 * t + li;
        return c < STEPS ? What{SCALE, n, (long long)s * STEPS + c} : What{PAD, n, 0};
    }
    const bool b = in >= B_BASE;
    const int q = b ? in - B_BASE : in, lane = q / (b ? B_LANE : A_LANE), p = (q % (b ? B_LANE : A_LANE)) / PIECE, byte = q % PIECE;
    const int c = b ? 2 : p / 2, t = p % 2, li = lane & 15, kq = lane >> 4;
    return What{WEIGHT, np * ROWS + 16 * t + li, (long long)s * KW + BLOCK * c + 8 * kq + 2 * byte};
}

}   // namespace w4t
}   // namespace er
