// Index maps of the GEMM kernels (k_gemm.h, k_gemm_stream.h) and of the LDS-DMA attention kernel (k_flash_attn.h), written once: the
// register -> row map of a 32 x 32 MFMA accumulator, the XCD-aware tile order of the LDS-DMA kernels, the streamed kernel's dealing of
// tiles to workgroups, the XOR-swizzled 128-byte row image and the row permutation of the fused GEGLU weight.
// Pure integer arithmetic with no device call (er_gemm_rows.h / er_mlp_map.h are the precedent): the kernels include it, and
// tests/host/gemm_map_check.cpp enumerates it on the host (permutations, bank-conflict freedom, exactly-once dealing).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ER_MAP_FN __host__ __device__ __forceinline__ constexpr
#else
#define ER_MAP_FN inline constexpr
#endif

namespace er {

// ---- C/D fragment of v_mfma_f32_32x32x*: row that accumulator register r (0..15) of lane half `half` (= lane >> 5) holds; the column
// is lane & 31.  Registers 4g .. 4g+3 are four consecutive rows starting at 8g + 4 half.  Independent of the input type.
ER_MAP_FN int mfma32_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

struct TileYX { int ty, tx; };

// ---- XCD-aware tile order of the 1-D grids (gemm_hh_mfma_kernel, gemm_hh256_kernel, gemm_f32d_mfma_kernel): workgroup `block` of nwg
// runs on XCD block % 8, and every XCD receives one contiguous run of row-major tile indices (neighbouring tiles share their A row panel
// in that XCD's L2) instead of every eighth one.  A permutation of [0, nwg) for any nwg; (ty, tx) = the tile at that index, ntx per row.
ER_MAP_FN int xcd_tile_index(unsigned block, int nwg) {
    const int xq = nwg >> 3, xr = nwg & 7, xcd = block & 7, within = block >> 3;      // (block unsigned: blockIdx.x as it comes)
    return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + within;
}
ER_MAP_FN TileYX xcd_tile(unsigned block, int nwg, int ntx) {
    const int lin = xcd_tile_index(block, nwg), ty = lin / ntx;
    return TileYX{ty, lin - ty * ntx};
}

// ---- the streamed kernel (gemm_hh_stream_kernel): workgroup b of G owns the tiles base + slot + j wx, j < mine, of ntiles.  Each XCD
// (b % 8: a speed assumption only) owns a contiguous run of tile indices, dealt round-robin to the wx workgroups of that XCD.
struct GsDeal { int base, slot, wx, mine; };
ER_MAP_FN GsDeal gs_deal(unsigned b, int G, int ntiles) {
    // Fewer workgroups than XCDs (a device of under eight CUs; no launch on a 256-CU chip): one contiguous run per workgroup.  With
    // eight runs the tiles of the XCDs that got no workgroup were nobody's (G = 1, two tiles: tile 1) - found by the host check.
    if (G < 8) {
        const int x = b, tq = ntiles / G, tr = ntiles % G;
        return GsDeal{x < tr ? x * (tq + 1) : tr * (tq + 1) + (x - tr) * tq, 0, 1, tq + (x < tr ? 1 : 0)};
    }
    const int xcd = b & 7, slot = b >> 3;
    const int wx = (G >> 3) + (xcd < (G & 7) ? 1 : 0);
    const int tq = ntiles >> 3, tr = ntiles & 7;
    const int nx = tq + (xcd < tr ? 1 : 0);
    const int base = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
    return GsDeal{base, slot, wx, slot < nx ? (nx - slot + wx - 1) / wx : 0};
}
// Tile order inside the stream: bands of GS_GH tile rows, walked column by column.  The tiles an XCD's 32 workgroups hold at the same
// time are 32 consecutive indices = a GS_GH x 8 block: per k-step the XCD's L2 fetches 4 A slices + 8 B slices (192 KB) for the 1 MB its
// CUs pull, instead of 1 + 32 (528 KB) with row-major order - the row-major first version of this kernel ran 4096^3 at 575 TFLOP/s,
// fabric-bound (profiles/r06_gemm_stream_probe_v1.log, r06_dma_rate_probe.log: a CU pulls 130 GB/s from L2 but 24 GB/s from HBM).
// (Two out-parameters on purpose: with a TileYX returned, the same arithmetic, hipcc placed two more vmcnt waits in the plain
// streamed kernel's epilogue - profiles/gemm_lanes_ab.log.)
constexpr int GS_GH = 4;
ER_MAP_FN void gs_tile_coords(int lin, int ntx, int nty, int& ty, int& tx) {
    const int band = lin / (GS_GH * ntx), r0 = band * GS_GH;
    const int gh = GS_GH < nty - r0 ? GS_GH : nty - r0, in = lin - band * GS_GH * ntx;
    tx = in / gh;
    ty = r0 + in - tx * gh;
}

// ---- the swizzled LDS image of a 128-byte tile row (64 halves or 32 floats of a k-tile): its 8 chunks of 16 bytes, chunk c of row r
// stored at slot c ^ ((r >> 1) & 7).  LDS-DMA writes lane-linearly, so the permutation is applied to the per-lane GLOBAL address (the 8
// lanes of a row still read one 128-byte line); XOR is its own inverse, so the same function names the source chunk of a slot.
// ESZ = bytes per element of the offsets returned: 2 (halves), 4 (floats), 1 (bytes).
ER_MAP_FN int swz_key(int row) { return (row >> 1) & 7; }
ER_MAP_FN int swz_slot(int row, int chunk) { return chunk ^ swz_key(row); }
template <int ESZ>
ER_MAP_FN int swz_chunk_off(int row, int chunk) {
    static_assert(ESZ == 1 || ESZ == 2 || ESZ == 4, "bytes, halves or floats");
    return swz_slot(row, chunk) << (ESZ == 1 ? 4 : ESZ == 2 ? 3 : 2);
}
// Offset inside the row image of the fragment a lane reads in k-substep ks: lane half `half` takes FRAG consecutive elements from
// element (2 ks + half) FRAG of the row - one whole chunk per ds_read_b128 of the fp16 kernels (FRAG = 8 halves or 16 bytes: 16 lanes
// with consecutive rows hit 16 different 16-byte bank groups), one float per ds_read_b32 of the fp32 kernel (FRAG = 1).
template <int ESZ, int FRAG>
ER_MAP_FN int swz_frag_off(int ks, int half, int row) {
    constexpr int EPC = 16 / ESZ;
    static_assert(FRAG == EPC || (FRAG == 1 && EPC == 4), "a whole chunk, or one float");
    if constexpr (FRAG == EPC) return swz_chunk_off<ESZ>(row, 2 * ks + half);
    else return swz_chunk_off<ESZ>(row, (2 * ks + half) >> 2) + ((2 * ks + half) & 3);
}

// ---- row of the ORIGINAL [2F][K] GEGLU weight that sits at row p of the permuted copy (tile = 128 columns = 4 blocks of 32:
// {value j0..j0+31, gate j0..j0+31, value j0+32.., gate j0+32..}); host and device agree through this one function
ER_MAP_FN int gemm_hh_geglu_row(int p, int F) {
    const int tile = p >> 7, local = p & 127, wn = local >> 6, blk = (local >> 5) & 1, l = local & 31;
    const int j = tile * 64 + wn * 32 + l;
    return blk == 0 ? j : F + j;
}

}   // namespace er
