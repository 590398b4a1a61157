// The streamed copy of an MXFP4 matrix (fp4 mode, er_w4.h), as index arithmetic only: where the nibble kernels of k_gemv.h find the
// bytes and the scale of every element.  Pure constexpr C++ with no device call (er_kv8_map.h / er_w8_tile_map.h are the precedents):
// gemv_kernel<w4_t> and w4_interleave_kernel are written over these functions and tests/host/w4_map_check.cpp enumerates them on the host.
//
// The nibble kernels keep fp16's lane -> element map: load j of lane l = elements (64 j + l) * 8 .. + 8 of the wave's 1536-element
// slice.  Eight nibbles are 4 bytes, and dword loads are an under-vectorised read pattern, so the copy interleaves ROW QUADS: for rows
// 4 r .. 4 r + 3, slice s, load j, lane l hold 16 contiguous bytes = the 4-byte pieces of the four rows, in row order.  A wave-load
// is 1 KiB, and the 64 scale bytes of the same (quad, slice, load) - 16 blocks of 32 elements per row - follow it as [block][row]:
// lane l reads the dword of block l / 4 (lanes 4 b .. 4 b + 3 share block b) and has the four rows' scales.  One such UNIT is 1088 bytes:
//     unit (quad r, slice s, load j) = (r * K / 1536 + s) * 3 + j
//     [unit * 1088 + 16 l + 4 row + byte]   byte `byte` (elements 2 byte, 2 byte + 1: low, high nibble) of lane l's piece of row 4 r + row
//     [unit * 1088 + 1024 + 4 b + row]      the e8m0 scale of block b (elements 32 b .. + 31 of the load's 512) of row 4 r + row
// N must be a multiple of 4 and K of 1536.
#pragma once

namespace er {
namespace w4map {

constexpr int SLICE = 1536;                 // elements of a row one wave reduces
constexpr int EPL = 8;                      // elements per lane and load (fp16's)
constexpr int LOADS = SLICE / (64 * EPL);   // 3 loads per lane and slice
constexpr int QUAD = 4;                     // rows interleaved
constexpr int LOAD_ELEMS = 64 * EPL;        // 512 elements of a row per wave-load
constexpr int LANE_BYTES = 16;              // one lane's load: QUAD pieces of EPL / 2 bytes
constexpr int PIECE_BYTES = EPL / 2;        // 4
constexpr int UNIT_NIBBLE_BYTES = 64 * LANE_BYTES;              // 1024
constexpr int BLOCKS_PER_LOAD = LOAD_ELEMS / 32;                // 16 scale blocks per row and wave-load
constexpr int UNIT_SCALE_BYTES = BLOCKS_PER_LOAD * QUAD;        // 64
constexpr int UNIT_BYTES = UNIT_NIBBLE_BYTES + UNIT_SCALE_BYTES; // 1088 = 68 * 16
constexpr int LANES_PER_BLOCK = 32 / EPL;                       // 4 lanes share a scale block

constexpr bool shape_ok(long long n, long long k) { return n > 0 && k > 0 && n % QUAD == 0 && k % SLICE == 0; }
constexpr long long units(long long n, long long k) { return n / QUAD * (k / SLICE) * LOADS; }
constexpr long long stream_bytes(long long n, long long k) { return units(n, k) * UNIT_BYTES; }

constexpr long long unit(long long quad, int k, int slice, int load) { return (quad * (k / SLICE) + slice) * LOADS + load; }
// what a lane loads: 16 bytes of nibbles, and the dword of its block's four scales
constexpr long long lane_offset(long long u, int lane) { return u * UNIT_BYTES + (long long)lane * LANE_BYTES; }
constexpr long long lane_scale_offset(long long u, int lane) { return u * UNIT_BYTES + UNIT_NIBBLE_BYTES + (lane / LANES_PER_BLOCK) * QUAD; }

// element (n, k) of the matrix -> where it lives
struct Where { long long quad; int row, slice, load, lane, byte, nibble; };
constexpr Where where(long long n, long long k) {
    const int in_slice = (int)(k % SLICE), g = in_slice / EPL;      // g: the 8-element group of the slice, = 64 load + lane
    return Where{n / QUAD, (int)(n % QUAD), (int)(k / SLICE), g / 64, g % 64, (in_slice % EPL) / 2, in_slice & 1};
}
constexpr long long byte_offset(const Where& w, int K) { return lane_offset(unit(w.quad, K, w.slice, w.load), w.lane) + w.row * PIECE_BYTES + w.byte; }
constexpr long long scale_offset(const Where& w, int K) { return lane_scale_offset(unit(w.quad, K, w.slice, w.load), w.lane) + w.row; }

}   // namespace w4map
}   // namespace er
