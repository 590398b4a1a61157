// Stand-alone check of the GEMM kernels' index maps (edgerunner_amd/csrc/er_gemm_map.h): the XCD-aware tile order, the streamed kernel's
// dealing of tiles to workgroups and its band order, the swizzled 128-byte row image, the 32 x 32 MFMA C/D map and the GEGLU row
// permutation.  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o gemm_map_check tests/host/gemm_map_check.cpp
// (tests/test_gemm_map_cpu.py does).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../../edgerunner_amd/csrc/er_gemm_map.h"

static int g_a, g_b, g_c;
#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at a=%d b=%d c=%d\n", __FILE__, __LINE__, #cond, g_a, g_b, g_c);            \
            exit(1);                                                                                                             \
        }                                                                                                                        \
    } while (0)

using namespace er;

// the 1-D grids: a permutation of the tiles for every grid size, and XCD x (the blocks = x mod 8) walks ONE contiguous run of indices
static long long check_xcd_order() {
    long long grids = 0;
    std::vector<int> seen;
    for (int nwg = 1; nwg <= 1100; ++nwg) {
        int run_end = 0;      // XCD x's run starts where XCD x - 1's ended
        for (int x = 0; x < 8; ++x)
            for (int b = x, prev = -1; b < nwg; b += 8) {
                g_a = nwg; g_b = b; g_c = -1;
                const int lin = xcd_tile_index(b, nwg);
                CHECK(lin == (prev < 0 ? run_end : prev + 1));
                prev = lin;
                run_end = lin + 1;
            }
        CHECK(run_end == nwg);
        for (int ntx = 1; ntx <= nwg; ++ntx) {
            if (nwg % ntx) continue;
            ++grids;
            const int nty = nwg / ntx;
            seen.assign(nwg, 0);
            for (int b = 0; b < nwg; ++b) {
                g_a = nwg; g_b = b; g_c = ntx;
                const TileYX t = xcd_tile(b, nwg, ntx);
                CHECK(t.ty >= 0 && t.ty < nty && t.tx >= 0 && t.tx < ntx);
                CHECK(t.ty * ntx + t.tx == xcd_tile_index(b, nwg));
                CHECK(seen[t.ty * ntx + t.tx]++ == 0);
            }
        }
    }
    return grids;
}

// the stream: every tile index belongs to exactly one workgroup, and the band order maps the indices one to one onto the tile grid
static long long check_stream_dealing() {
    long long deals = 0, ragged = 0;
    std::vector<int> seen;
    for (int ntiles = 1; ntiles <= 1100; ++ntiles) {
        for (int G = 1; G <= (ntiles < 256 ? ntiles : 256); ++G) {
            g_a = ntiles; g_b = G; g_c = -1;
            ++deals;
            seen.assign(ntiles, 0);
            long long total = 0;
            for (int b = 0; b < G; ++b) {
                const GsDeal d = gs_deal(b, G, ntiles);
                CHECK(d.mine >= 0 && d.wx >= 1);
                total += d.mine;
                for (int j = 0; j < d.mine; ++j) {
                    const int lin = d.base + d.slot + j * d.wx;
                    g_c = lin;
                    CHECK(lin >= 0 && lin < ntiles);
                    CHECK(seen[lin]++ == 0);
                }
            }
            CHECK(total == ntiles);
        }
        for (int ntx = 1; ntx <= ntiles; ++ntx) {
            if (ntiles % ntx) continue;
            const int nty = ntiles / ntx;
            if (nty % GS_GH) ++ragged;
            seen.assign(ntiles, 0);
            for (int lin = 0; lin < ntiles; ++lin) {
                g_a = ntiles; g_b = ntx; g_c = lin;
                int ty = -1, tx = -1;
                gs_tile_coords(lin, ntx, nty, ty, tx);
                CHECK(ty >= 0 && ty < nty && tx >= 0 && tx < ntx);
                CHECK(seen[ty * ntx + tx]++ == 0);
            }
        }
    }
    CHECK(ragged > 0);
    return deals;
}

// fragment reads of a whole chunk per lane (FRAG elements of ESZ bytes = 16 bytes): bank groups the 16 lanes of a group hit
template <int ESZ, int FRAG>
static void check_frag_banks() {
    for (int ks = 0; ks < 4; ++ks)
        for (int blk = 0; blk < 8; ++blk)          // the lane's row is li + 32 x block: up to 256 rows per operand image
            for (int grp = 0; grp < 4; ++grp) {
                unsigned hit = 0;
                for (int l = 16 * grp; l < 16 * grp + 16; ++l) {
                    g_a = ks; g_b = blk; g_c = l;
                    const int row = 32 * blk + (l & 31), half = l >> 5;
                    const int off = swz_frag_off<ESZ, FRAG>(ks, half, l & 31);
                    CHECK((off == swz_frag_off<ESZ, FRAG>(ks, half, row)));          // 32-row blocks share the lane's key (the kernels hoist it)
                    const int byte = row * 128 + off * ESZ;
                    CHECK(byte % 16 == 0 && off * ESZ < 128);
                    // the chunk read is the one the DMA lane of that slot brought in: chunk 2 ks + half of the row
                    CHECK(swz_chunk_off<ESZ>(row, (off * ESZ) >> 4) * ESZ == 16 * (2 * ks + half));
                    hit |= 1u << ((byte >> 4) & 15);                               // 64 banks x 4 bytes = 16 groups of 16 bytes
                }
                CHECK(hit == 0xffffu);
            }
}

static void check_swizzle() {
    for (int row = 0; row < 256; ++row) {
        unsigned slots = 0;
        for (int c = 0; c < 8; ++c) {
            g_a = row; g_b = c; g_c = -1;
            const int s = swz_slot(row, c);
            CHECK(s >= 0 && s < 8);
            CHECK(swz_slot(row, s) == c);                                          // its own inverse: source chunk of a slot
            CHECK(swz_chunk_off<2>(row, c) == 8 * s && swz_chunk_off<4>(row, c) == 4 * s && swz_chunk_off<1>(row, c) == 16 * s);
            slots |= 1u << s;
        }
        CHECK(slots == 0xffu);
    }
    check_frag_banks<2, 8>();       // fp16 kernels, offsets in halves
    check_frag_banks<1, 16>();      // the streamed kernel, offsets in bytes
    // the fp32 kernel reads one float per lane: k = 2 kk + half lies in chunk k / 4 at position k % 4
    for (int kk = 0; kk < 16; ++kk)
        for (int l = 0; l < 64; ++l) {
            g_a = kk; g_b = l; g_c = -1;
            const int row = l & 31, k = 2 * kk + (l >> 5);
            CHECK((swz_frag_off<4, 1>(kk, l >> 5, row)) == 4 * swz_slot(row, k >> 2) + (k & 3));
        }
}

static void check_cd_map() {
    unsigned rows = 0;
    for (int half = 0; half < 2; ++half)
        for (int r = 0; r < 16; ++r) {
            g_a = r; g_b = half; g_c = -1;
            const int row = mfma32_row(r, half);
            CHECK(row >= 0 && row < 32 && !(rows & (1u << row)));
            rows |= 1u << row;
        }
    CHECK(rows == 0xffffffffu);
}

static void check_geglu() {
    for (int F : {64, 128, 4096}) {
        std::vector<int> seen(2 * F, 0);
        for (int p = 0; p < 2 * F; ++p) {
            g_a = F; g_b = p; g_c = -1;
            const int src = gemm_hh_geglu_row(p, F);
            CHECK(src >= 0 && src < 2 * F);
            CHECK(seen[src]++ == 0);
            // blocks of 32: value rows j .. j + 31, then the gate rows of the SAME outputs
            if ((p >> 5) & 1) CHECK(src == F + gemm_hh_geglu_row(p - 32, F));
        }
    }
}

int main() {
    const long long grids = check_xcd_order();
    const long long deals = check_stream_dealing();
    check_swizzle();
    check_cd_map();
    check_geglu();
    printf("gemm_map_check: ok (%lld grids, %lld dealings)\n", grids, deals);
    return 0;
}
