// Host enumeration of csrc/er_w4_map.h (the quad-interleaved streamed copy of an MXFP4 matrix).  For every element of a [N][K] matrix:
//   - exactly one (quad, slice, load, lane, byte, nibble) holds it, and every nibble of the copy holds exactly one element;
//   - its scale is one of the four bytes of the dword the lane reads, the byte of its row, and every scale byte of the copy is the
//     scale of exactly one block;
//   - the element sits where the kernel's lane -> element map expects it: load j of lane l = elements (64 j + l) * 8 .. + 8 of the slice;
//   - no load crosses its unit, and every load is 16-byte aligned (scale dwords 4-byte aligned).
// w4_map_check <n> <k> ...: checks each pair, prints "M <n> <k> <units> <bytes>" per pair, then the launch rule of csrc/er_w4_rule.h as
// "R <proj> <B> <knob> <w4_streams>" for every projection, B = 0 .. 5 and knob = -1, 0, 1, and "w4_map_check: ok".  Built with ASan + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../edgerunner_amd/csrc/er_w4_map.h"
#include "../../edgerunner_amd/csrc/er_w4_rule.h"

using namespace er::w4map;

static_assert(UNIT_BYTES == 1088 && UNIT_BYTES % 16 == 0 && LOADS == 3 && LANE_BYTES == QUAD * PIECE_BYTES, "unit shape");
static_assert(shape_ok(4608, 1536) && shape_ok(6144, 1536) && shape_ok(1536, 6144) && !shape_ok(6, 1536) && !shape_ok(8, 1024), "shapes");
static_assert(stream_bytes(4608, 1536) == 4608LL * 1536 / 2 + 4608LL * 1536 / 32, "a copy has the canonical block's size");

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

static int check(long long n, int k) {
    if (!shape_ok(n, k)) FAIL("shape %lld x %d refused", n, k);
    const long long total = stream_bytes(n, k);
    std::vector<uint8_t> nib_owner(total * 2, 0), scale_owner(total, 0);      // how many elements / blocks claim a nibble / a scale byte
    for (long long r = 0; r < n; ++r)
        for (long long c = 0; c < k; ++c) {
            const Where w = where(r, c);
            if (w.quad != r / 4 || w.row != r % 4 || w.slice * SLICE + (w.load * 64 + w.lane) * EPL + w.byte * 2 + w.nibble != c) FAIL("element (%lld, %lld) is not where the lane map reads it", r, c);
            if (w.lane < 0 || w.lane >= 64 || w.load < 0 || w.load >= LOADS || w.byte < 0 || w.byte >= PIECE_BYTES) FAIL("element (%lld, %lld): slot out of range", r, c);
            const long long u = unit(w.quad, k, w.slice, w.load), lo = lane_offset(u, w.lane), so = lane_scale_offset(u, w.lane);
            if (u < 0 || u >= units(n, k)) FAIL("unit %lld out of range", u);
            if (lo % 16 || so % 4) FAIL("load of unit %lld lane %d is misaligned", u, w.lane);
            if (lo < u * UNIT_BYTES || lo + LANE_BYTES > u * UNIT_BYTES + UNIT_NIBBLE_BYTES) FAIL("nibble load crosses its unit");
            if (so < u * UNIT_BYTES + UNIT_NIBBLE_BYTES || so + QUAD > (u + 1) * UNIT_BYTES) FAIL("scale load crosses its unit");
            const long long b = byte_offset(w, k), s = scale_offset(w, k);
            if (b < lo || b >= lo + LANE_BYTES || b != lo + w.row * PIECE_BYTES + w.byte) FAIL("byte of (%lld, %lld) is outside its lane's load", r, c);
            if (s < so || s >= so + QUAD || s != so + w.row) FAIL("scale of (%lld, %lld) is not the one its lane reads", r, c);
            ++nib_owner[b * 2 + w.nibble];
            // the four lanes of a block read the same dword, and elements of one block of one row share the byte
            const Where first = where(r, c / 32 * 32);
            if (scale_offset(first, k) != s) FAIL("block of (%lld, %lld) has two scales", r, c);
            if (c % 32 == 0) ++scale_owner[s];
        }
    for (long long u = 0; u < units(n, k); ++u)
        for (int i = 0; i < UNIT_BYTES; ++i) {
            const long long o = u * UNIT_BYTES + i;
            if (i < UNIT_NIBBLE_BYTES) {
                if (nib_owner[2 * o] != 1 || nib_owner[2 * o + 1] != 1 || scale_owner[o] != 0) FAIL("nibble byte %lld is held %d + %d times", o, nib_owner[2 * o], nib_owner[2 * o + 1]);
            } else if (scale_owner[o] != 1 || nib_owner[2 * o] || nib_owner[2 * o + 1]) FAIL("scale byte %lld is held %d times", o, scale_owner[o]);
        }
    std::printf("M %lld %d %lld %lld\n", n, k, units(n, k), total);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3 || argc % 2 == 0) FAIL("usage: w4_map_check <n> <k> ...");
    for (int i = 1; i + 1 < argc; i += 2)
        if (check(std::atoll(argv[i]), std::atoi(argv[i + 1]))) return 1;
    for (int proj = er::PROJ_QKV; proj <= er::PROJ_HEAD; ++proj)
        for (int B = 0; B <= 5; ++B)
            for (int knob = -1; knob <= 1; ++knob) std::printf("R %d %d %d %d\n", proj, B, knob, er::w4_streams((er::Proj)proj, B, knob) ? 1 : 0);
    std::printf("w4_map_check: ok\n");
    return 0;
}
