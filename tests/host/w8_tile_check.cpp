// csrc/er_w8_tile_map.h on the host: the tiled byte copy of an fp8-mode matrix, enumerated.  For every shape: the tiling loop of
// tile_weights_kernel<w8_t> (w8t_piece_source) puts every (n, k) of [N][K] into exactly one byte of the block, at w8t_offset(n, k); pad
// rows are zero and pad scales 1; and the piece that lane (li, kq) of wave wid of workgroup (np, y) loads for step c
// (gemv_mfma_kernel: w8t_piece) holds, in bytes 8 t .. 8 t + 7, the weights k = kbase + 32 c .. + 7 of row 32 np + 16 t + li with
// kbase = (y * NWV + wid) * 96 + 8 kq - the slot assignment of the fp16 form - for 16- and 4-wave workgroups.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../edgerunner_amd/csrc/er_w8_tile_map.h"

using namespace er;

static int failures = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            if (++failures <= 10) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                               \
    } while (0)

static unsigned char src_byte(int n, int k) { return (unsigned char)(1 + (n * 131 + k * 7) % 251); }      // never 0: a pad byte is told apart

static void check_shape(int N, int K) {
    const long long rows = w8t_rows(N), wbytes = rows * K;
    CHECK(rows % 32 == 0 && rows >= N && rows - N < 32, "N %d: %lld padded rows", N, rows);
    CHECK(w8t_block_bytes(N, K) == (size_t)(wbytes + rows * 4), "N %d K %d: block bytes", N, K);
    CHECK(w8t_pieces(N, K) * W8T_PIECE == wbytes, "N %d K %d: pieces", N, K);
    std::vector<unsigned char> blk(w8t_block_bytes(N, K), 0xEE);
    std::vector<unsigned char> hits(wbytes, 0);
    // the tiling kernel's loop
    for (long long p = 0; p < w8t_pieces(N, K); ++p) {
        int n, k;
        w8t_piece_source(K, p, &n, &k);
        CHECK(n >= 0 && n + 16 < rows + 16 && n % 32 < 16 && k >= 0 && k + 8 <= K && k % 8 == 0, "piece %lld: source (%d, %d)", p, n, k);
        for (int t = 0; t < 2; ++t)
            for (int j = 0; j < 8; ++j) {
                const int nn = n + 16 * t;
                const long long off = p * W8T_PIECE + 8 * t + j;
                blk[off] = nn < N ? src_byte(nn, k + j) : 0;
                ++hits[off];
                CHECK(w8t_offset(K, nn, k + j) == off, "piece %lld byte %d: w8t_offset(%d, %d) = %lld", p, 8 * t + j, nn, k + j, w8t_offset(K, nn, k + j));
            }
    }
    float* sc = reinterpret_cast<float*>(blk.data() + wbytes);
    CHECK((const void*)w8t_scales(blk.data(), N, K) == (const void*)sc, "N %d K %d: scales pointer", N, K);
    for (long long i = 0; i < rows; ++i) sc[i] = i < N ? 1.0f + (float)i : 1.0f;
    for (long long o = 0; o < wbytes; ++o) CHECK(hits[o] == 1, "N %d K %d: byte %lld written %d times", N, K, o, (int)hits[o]);
    // every (n, k) exactly once, pad rows zero
    std::vector<unsigned char> seen(wbytes, 0);
    for (int n = 0; n < rows; ++n)
        for (int k = 0; k < K; ++k) {
            const long long off = w8t_offset(K, n, k);
            CHECK(off >= 0 && off < wbytes, "(%d, %d): offset %lld outside the block", n, k, off);
            if (off < 0 || off >= wbytes) continue;
            CHECK(!seen[off], "(%d, %d): offset %lld taken twice", n, k, off);
            seen[off] = 1;
            CHECK(blk[off] == (n < N ? src_byte(n, k) : 0), "(%d, %d): byte %d", n, k, (int)blk[off]);
        }
    for (long long i = N; i < rows; ++i) CHECK(sc[i] == 1.0f, "pad scale %lld", i);
    // the streaming kernel's reads: workgroup (np, y), NWV waves of 64 lanes, 3 loads of 16 bytes per lane
    for (int NWV : {16, 4}) {
        if (K % (NWV * 96)) continue;
        std::vector<unsigned char> read(wbytes, 0);
        for (int np = 0; np < rows / 32; ++np)
            for (int y = 0; y < K / (NWV * 96); ++y)
                for (int wid = 0; wid < NWV; ++wid)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int li = lane & 15, kq = lane >> 4, kbase = (y * NWV + wid) * 96 + kq * 8, kt0 = (y * NWV + wid) * 3;
                        for (int c = 0; c < 3; ++c) {
                            const long long piece = w8t_piece(K, np, kt0 + c, lane);
                            CHECK(piece >= 0 && piece < w8t_pieces(N, K), "load outside the block: piece %lld", piece);
                            if (piece < 0 || piece >= w8t_pieces(N, K)) continue;
                            for (int t = 0; t < 2; ++t)
                                for (int j = 0; j < 8; ++j) {
                                    const int n = 32 * np + 16 * t + li, k = kbase + 32 * c + j;
                                    const long long off = piece * W8T_PIECE + 8 * t + j;
                                    CHECK(blk[off] == (n < N ? src_byte(n, k) : 0), "NWV %d wg (%d, %d) wave %d lane %d c %d t %d j %d: slot holds %d", NWV, np, y, wid, lane, c, t, j, (int)blk[off]);
                                    ++read[off];
                                }
                        }
                        for (int t = 0; t < 2; ++t) {      // the two row scales of the lane
                            const int n = 32 * np + 16 * t + li;
                            CHECK(n < rows && w8t_scales(blk.data(), N, K)[n] == (n < N ? 1.0f + (float)n : 1.0f), "scale of row %d", n);
                        }
                    }
        for (long long o = 0; o < wbytes; ++o) CHECK(read[o] == 1, "NWV %d: byte %lld streamed %d times", NWV, o, (int)read[o]);
    }
}

int main() {
    const int shapes[][2] = {{4608, 1536}, {1536, 1536}, {6144, 1536}, {1536, 6144}, {501, 6144}, {1001, 1536}, {1, 1536}, {33, 1536}};
    for (const auto& s : shapes) check_shape(s[0], s[1]);
    if (failures) { printf("w8_tile_check: %d failures\n", failures); return 1; }
    printf("w8_tile_check: ok\n");
    return 0;
}
