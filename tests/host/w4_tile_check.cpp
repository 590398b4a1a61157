// csrc/er_w4_tile_map.h on the host: the tiled nibble copy of an fp4-mode (MXFP4) matrix, enumerated.  For every shape:
//   - offset(n, k) and scale_offset(n, block) are injections into the block (two elements per weight byte: k even low, k odd high);
//   - what() - the inverse the tiling kernel (er_weights.h w4_tile_kernel) is written over - agrees with them, and every byte of the
//     block is a weight byte, a scale byte or the named padding byte of a row's scale dword;
//   - the tiling kernel's loop (one dword per thread, replayed here) fills the block from a canonical block, pad rows zero / scale 127;
//   - the loads of lane (li, kq) of wave `wid` of workgroup (np, y) in gemv_mfma_kernel<w4_t> - 16 + 8 nibble bytes and 8 scale bytes -
//     stay inside the wave's unit, are aligned, and hold for step c and row tile t exactly the eight weights k = kbase + 32 c .. + 7 of
//     row 32 np + 16 t + li with kbase = (y * NWV + wid) * 96 + 8 kq - the slot assignment of the fp16 tiled copy (k_gemv_mfma.h; the same
//     set tests/host/w8_tile_check.cpp holds the byte copy to) - in nibble order, with the scale of block k / 32 of that row; for 16-
//     and 4-wave workgroups, every byte of the block streamed exactly once (scale bytes once per kq lane: four times).
// Then the launch rules of csrc/er_w4_rule.h: "R <proj> <B> <knob> <w4_streams_batched> <w4_streams>" for every projection, B = 0 .. 33
// and knob = -1, 0, 1, and "w4_tile_check: ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../edgerunner_amd/csrc/er_w4_rule.h"
#include "../../edgerunner_amd/csrc/er_w4_tile_map.h"

using namespace er::w4t;

static_assert(UNIT_BYTES == 1664 && UNIT_BYTES % 128 == 0 && STEPS == 3 && A_LANE + B_LANE == 2 * STEPS * PIECE, "unit shape");
static_assert(shape_ok(4608, 1536) && shape_ok(501, 6144) && !shape_ok(32, 1000) && !shape_ok(0, 1536), "shapes");
static_assert(block_bytes(4608, 1536) == 4608LL / 32 * 16 * 1664, "144 row pairs x 16 slices");

static int failures = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            if (++failures <= 10) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                               \
    } while (0)

static unsigned nib_of(long long n, long long k) { return (unsigned)((n * 7 + k * 5 + (k >> 5)) % 15 + 1); }              // never 0: a pad nibble is told apart
static unsigned char scale_of(long long n, long long b) { return (unsigned char)(112 + (n * 3 + b * 11) % 23); }        // e8m0 bytes of e = -15 .. 7

static void check_shape(int N, int K) {
    CHECK(shape_ok(N, K), "shape %d x %d refused", N, K);
    const long long R = rows(N), total = block_bytes(N, K), KB = K / BLOCK;
    CHECK(R % 32 == 0 && R >= N && R - N < 32, "N %d: %lld padded rows", N, R);
    CHECK(total == R / 32 * (K / 96) * 1664, "N %d K %d: block bytes", N, K);
    // the canonical block: nibble bytes row-major, then scale bytes row-major
    std::vector<unsigned char> canon((size_t)N * K / 2 + (size_t)N * KB);
    for (long long n = 0; n < N; ++n) {
        for (long long k = 0; k < K; k += 2) canon[(n * K + k) / 2] = (unsigned char)(nib_of(n, k) | nib_of(n, k + 1) << 4);
        for (long long b = 0; b < KB; ++b) canon[(size_t)N * K / 2 + n * KB + b] = scale_of(n, b);
    }
    // the tiling kernel's loop, dword by dword
    std::vector<unsigned char> blk(total, 0xEE);
    CHECK(total % 4 == 0, "block of %lld bytes", total);
    for (long long i = 0; i < total / 4; ++i) {
        const What w = what(K, i * 4);
        unsigned char v[4] = {0, 0, 0, 0};
        if (w.kind == WEIGHT) {
            CHECK(w.k % 8 == 0 && w.n >= 0 && w.n < R && w.k + 8 <= K, "dword %lld: weight (%lld, %lld)", i, w.n, w.k);
            if (w.n < N) for (int j = 0; j < 4; ++j) v[j] = canon[(w.n * K + w.k) / 2 + j];
        } else {
            CHECK(w.kind == SCALE && w.k % STEPS == 0 && w.n >= 0 && w.n < R && w.k + STEPS <= KB, "dword %lld: scale (%lld, %lld)", i, w.n, w.k);
            for (int j = 0; j < 3; ++j) v[j] = w.n < N ? canon[(size_t)N * K / 2 + w.n * KB + w.k + j] : (unsigned char)PAD_SCALE;
        }
        for (int j = 0; j < 4; ++j) blk[i * 4 + j] = v[j];
    }
    // injections, and the inverse
    std::vector<unsigned char> owner(total, 0);      // 1 / 2: low / high nibble taken, 4: scale
    for (long long n = 0; n < R; ++n) {
        for (long long k = 0; k < K; ++k) {
            const long long off = offset(K, n, k);
            CHECK(off >= 0 && off < total, "(%lld, %lld): offset %lld outside the block", n, k, off);
            if (off < 0 || off >= total) continue;
            const unsigned char bit = (k & 1) ? 2 : 1;
            CHECK(!(owner[off] & bit) && !(owner[off] & 4), "(%lld, %lld): nibble of byte %lld taken twice", n, k, off);
            owner[off] |= bit;
            const What w = what(K, off);
            CHECK(w.kind == WEIGHT && w.n == n && w.k == (k & ~1LL), "(%lld, %lld): what(%lld) = kind %d (%lld, %lld)", n, k, off, w.kind, w.n, w.k);
            const unsigned got = (k & 1) ? blk[off] >> 4 : blk[off] & 15u;
            CHECK(got == (n < N ? nib_of(n, k) : 0u), "(%lld, %lld): nibble %u", n, k, got);
        }
        for (long long b = 0; b < KB; ++b) {
            const long long off = scale_offset(K, n, b);
            CHECK(off >= 0 && off < total, "scale (%lld, %lld): offset %lld outside the block", n, b, off);
            if (off < 0 || off >= total) continue;
            CHECK(owner[off] == 0, "scale (%lld, %lld): byte %lld taken twice", n, b, off);
            owner[off] = 4;
            const What w = what(K, off);
            CHECK(w.kind == SCALE && w.n == n && w.k == b, "scale (%lld, %lld): what(%lld) = kind %d (%lld, %lld)", n, b, off, w.kind, w.n, w.k);
            CHECK(blk[off] == (n < N ? scale_of(n, b) : PAD_SCALE), "scale (%lld, %lld): byte %d", n, b, (int)blk[off]);
        }
    }
    long long pads = 0;
    for (long long o = 0; o < total; ++o) {
        if (owner[o] == 0) {
            const What w = what(K, o);
            CHECK(w.kind == PAD && w.n >= 0 && w.n < R, "byte %lld is neither weight, scale nor padding (kind %d)", o, w.kind);
            ++pads;
        } else {
            CHECK(owner[o] == 3 || owner[o] == 4, "byte %lld holds one nibble only", o);
        }
    }
    CHECK(pads == R * (K / 96), "N %d K %d: %lld padding bytes", N, K, pads);
    // the streaming kernel's reads
    for (int NWV : {16, 4}) {
        if (K % (NWV * 96)) continue;
        std::vector<unsigned char> read(total, 0);
        for (int np = 0; np < R / 32; ++np)
            for (int y = 0; y < K / (NWV * 96); ++y)
                for (int wid = 0; wid < NWV; ++wid)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int li = lane & 15, kq = lane >> 4, s = y * NWV + wid, kbase = s * 96 + kq * 8;
                        const long long u = unit(K, np, s), lo = u * UNIT_BYTES, hi = lo + UNIT_BYTES;
                        const long long oa = lane_a_offset(u, lane), ob = lane_b_offset(u, lane), os = lane_scale_offset(u, lane);
                        CHECK(u >= 0 && u < units(N, K), "unit %lld out of range", u);
                        CHECK(oa % 16 == 0 && ob % 8 == 0 && os % 8 == 0, "unit %lld lane %d: misaligned load", u, lane);
                        CHECK(oa >= lo && oa + A_LANE <= lo + B_BASE && ob >= lo + B_BASE && ob + B_LANE <= lo + S_BASE && os >= lo + S_BASE && os + S_ROW <= hi,
                              "unit %lld lane %d: a load leaves its part of the unit", u, lane);
                        if (u < 0 || u >= units(N, K)) continue;
                        CHECK(oa == lo + 16 * lane && ob == lo + 1024 + 8 * lane, "wave-loads are not contiguous across the lanes");
                        for (int c = 0; c < STEPS; ++c)
                            for (int t = 0; t < 2; ++t) {
                                const long long piece = c < 2 ? oa + PIECE * (2 * c + t) : ob + PIECE * t;      // the kernel: w4a[2 c + t] / w4b[t]
                                const long long n = 32LL * np + 16 * t + li;
                                for (int j = 0; j < 8; ++j) {
                                    const long long k = kbase + 32 * c + j;
                                    CHECK(offset(K, n, k) == piece + j / 2, "NWV %d wg (%d, %d) wave %d lane %d c %d t %d j %d: not in the lane's piece", NWV, np, y, wid, lane, c, t, j);
                                    const unsigned got = (j & 1) ? blk[piece + j / 2] >> 4 : blk[piece + j / 2] & 15u;      // nibble j of the dword
                                    CHECK(got == (n < N ? nib_of(n, k) : 0u), "NWV %d wg (%d, %d) wave %d lane %d c %d t %d j %d: slot holds %u", NWV, np, y, wid, lane, c, t, j, got);
                                    if (!(j & 1)) ++read[piece + j / 2];
                                }
                                // the kernel: byte c of scale dword t
                                CHECK(scale_offset(K, n, (kbase + 32 * c) / 32) == os + PIECE * t + c, "scale of row %lld block %d is not byte %d of the lane's dword %d", n, (kbase + 32 * c) / 32, c, t);
                                CHECK(blk[os + PIECE * t + c] == (n < N ? scale_of(n, 3 * s + c) : PAD_SCALE), "scale byte of row %lld step %d", n, c);
                                ++read[os + PIECE * t + c];
                            }
                    }
        for (long long o = 0; o < total; ++o) CHECK(read[o] == (owner[o] == 3 ? 1 : owner[o] == 4 ? 4 : 0), "NWV %d: byte %lld streamed %d times", NWV, o, (int)read[o]);
    }
    printf("M %d %d %lld %lld\n", N, K, units(N, K), total);
}

int main() {
    const int shapes[][2] = {{4608, 1536}, {6144, 1536}, {1536, 6144}, {1536, 1536}, {501, 6144}, {48, 1536}};
    for (const auto& s : shapes) check_shape(s[0], s[1]);
    for (int proj = er::PROJ_QKV; proj <= er::PROJ_HEAD; ++proj)
        for (int B = 0; B <= 33; ++B)
            for (int knob = -1; knob <= 1; ++knob)
                printf("R %d %d %d %d %d\n", proj, B, knob, er::w4_streams_batched((er::Proj)proj, B, knob) ? 1 : 0, er::w4_streams((er::Proj)proj, B, knob) ? 1 : 0);
    if (failures) { printf("w4_tile_check: %d failures\n", failures); return 1; }
    printf("w4_tile_check: ok\n");
    return 0;
}
