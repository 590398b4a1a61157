// Host enumeration of the byte KV cache (kv8 mode): the QUAD lane mapping of csrc/er_kv8_map.h, the cache encoder kv8_encode of
// csrc/er_w8.h and the plan rules of csrc/er_decode_plan.h.  The mapping is checked here (a failed property prints a line and the
// program returns 1); tests/test_kv8_cpu.py compares the encoder lines with torch's float8_e4m3fn cast and the plan lines with the
// rules of the mode.  Built with ASan + UBSan.
//   E <fp32 bits of v> <kv8_encode(v)>
//   P <batch> <kv8> <decode_version> <attn_kernel> <merge_launch> <plan.kv8> <plan.stream_attn> <plan.v3>
//   S <batch> <plan.shared_attn with prefix groups asked for on a kv8 plan>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../edgerunner_amd/csrc/er_decode_plan.h"
#include "../../edgerunner_amd/csrc/er_kv8_map.h"
#include "../../edgerunner_amd/csrc/er_w8.h"

using namespace er;

static int fail(const char* what, int a, int b) {
    std::printf("kv8_map_check: %s (%d, %d)\n", what, a, b);
    return 1;
}

static int check_map() {
    using namespace kv8;
    static_assert(SLOTS == ROWS * PIECES && NV * GL == SLOTS && PIECES * EPL == D && KPW == 32, "quad shape");
    // every byte of a quad of consecutive rows is loaded exactly once, and no 16-byte load straddles a row
    int loaded[ROWS * D] = {0};
    int slot_of[ROWS][PIECES];
    std::memset(slot_of, -1, sizeof(slot_of));
    for (int j = 0; j < NV; ++j)
        for (int p = 0; p < GL; ++p) {
            const int t = slot(j, p), r = load_row(j, p), c = load_piece(j, p);
            if (r != slot_row(t) || c != slot_piece(t)) return fail("load_row / load_piece disagree with the slot", j, p);
            if (r < 0 || r >= ROWS || c < 0 || c >= PIECES) return fail("slot outside the quad", j, p);
            if (r != j && r != j + 1) return fail("load j holds rows j and j + 1 only", j, p);
            const int byte0 = r * D + load_byte_in_row(j, p);
            if (byte0 != 16 * t) return fail("lane p of load j reads the p-th 16 bytes of line j", j, p);
            if (byte0 / D != (byte0 + EPL - 1) / D) return fail("a load straddles a row", j, p);
            for (int e = 0; e < EPL; ++e) ++loaded[byte0 + e];
            if (slot_of[r][c] != -1) return fail("a (row, piece) has two slots", r, c);
            slot_of[r][c] = t;
        }
    for (int i = 0; i < ROWS * D; ++i)
        if (loaded[i] != 1) return fail("a byte of the quad is not loaded exactly once", i, loaded[i]);
    for (int r = 0; r < ROWS; ++r)
        for (int c = 0; c < PIECES; ++c)
            if (slot_of[r][c] < 0) return fail("a (row, piece) has no slot", r, c);
    // a key's score: the slots score_takes() names are the six pieces of that row, each once, and nothing else
    for (int r = 0; r < ROWS; ++r) {
        int pieces[PIECES] = {0}, n = 0;
        for (int j = 0; j < NV; ++j)
            for (int p = 0; p < GL; ++p)
                if (score_takes(r, j, p)) {
                    if (slot_row(slot(j, p)) != r) return fail("a score takes another row's slot", r, slot(j, p));
                    ++pieces[load_piece(j, p)];
                    ++n;
                }
        for (int j = 0; j < NV; ++j)
            for (int p = 0; p < GL; ++p)
                if (score_takes(r, j, p) && !score_load(r, j)) return fail("score_load leaves out a load that holds the row", r, j);
        if (n != PIECES) return fail("a score does not take six slots", r, n);
        for (int c = 0; c < PIECES; ++c)
            if (pieces[c] != 1) return fail("a score misses a piece", r, c);
    }
    // the fold: a row of 16 lanes is two groups of 8 that hold the same sums after the rotation by 8; receiver lane c < 6 of either
    // group adds, for every term i, the accumulator fold_load(i, sender) of the sender fold_shift(i) lanes above it (mod 8).  Each of
    // the 96 outputs (piece c, element e) is then reached exactly once per row of 16 lanes and group: by lane c, from the four slots
    // of piece c - one per key row.
    if (fold_shift(0) != 0 || fold_load(0, 0) != 0) return fail("term 0 is the lane's own load 0", fold_shift(0), fold_load(0, 0));
    int stored[PIECES] = {0};
    for (int lane16 = 0; lane16 < 16; ++lane16) {      // the 16 lanes of a row: who stores, and which piece
        if (!fold_stores(lane16)) continue;            // the second group and lanes 6 and 7 fold too and store nothing
        const int c = lane16 & (GL - 1);
        if (store_piece(c) < 0 || store_piece(c) >= PIECES) return fail("a lane stores outside the 96 outputs", lane16, store_piece(c));
        if (store_piece(c) != c) return fail("lane c collects piece c, and must store it as that", c, store_piece(c));
        ++stored[store_piece(c)];
        bool row_seen[ROWS] = {false, false, false, false};
        for (int i = 0; i < FOLD_TERMS; ++i) {
            const int sender = (c + fold_shift(i)) % GL, j = fold_load(i, sender);
            if (j < 0 || j >= NV) return fail("fold_load outside the loads", i, sender);
            const int t = slot(j, sender);
            if (slot_piece(t) != c) return fail("the fold hands a lane another piece", c, i);
            if (row_seen[slot_row(t)]) return fail("the fold adds a key row twice", c, i);
            row_seen[slot_row(t)] = true;
        }
        for (int r = 0; r < ROWS; ++r)
            if (!row_seen[r]) return fail("the fold misses a key row", c, r);
    }
    for (int c = 0; c < PIECES; ++c)
        if (stored[c] != 1) return fail("a piece of the output is not stored exactly once per row of 16 lanes", c, stored[c]);
    return 0;
}

static void encode_sweep() {
    std::vector<float> in;
    for (int c = 0; c < 0x7f; ++c) {      // all 127 finite magnitudes (254 codes with the signs), every midpoint and its fp32 neighbours
        const float lo = w8_decode((uint8_t)c);
        in.push_back(lo); in.push_back(-lo);
        if (c == 0x7e) break;
        const float hi = w8_decode((uint8_t)(c + 1)), mid = 0.5f * (lo + hi);
        for (float v : {mid, std::nextafterf(mid, 0.f), std::nextafterf(mid, 1e9f)}) { in.push_back(v); in.push_back(-v); }
    }
    const float inf = std::numeric_limits<float>::infinity();
    for (float v : {448.f, std::nextafterf(448.f, 1e9f), 464.f, 480.f, 1e6f, 3.0e38f, inf, 0.f,
                    1e-38f, 1.1754942e-38f /* the largest fp32 subnormal */, 1e-41f, 1.4e-45f /* the smallest */}) { in.push_back(v); in.push_back(-v); }
    for (float v : in) std::printf("E %u %d\n", (unsigned)w8_f32_bits(v), (int)kv8_encode(v));
    for (uint32_t bits : {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu})      // quiet and signalling NaNs
        std::printf("E %u %d\n", (unsigned)bits, (int)kv8_encode(w8_bits_f32(bits)));
}

static void plan_lines() {
    const DecodeKnobs k;                                  // the defaults: decode_v 3, attn_v_batched auto
    const ReserveKnobs rk{false, false, true};
    const AttnChunking ch{16, 16 * 512, 128};
    for (int B : {1, 4, 5, 15, 16, 33})
        for (int kv8 = 0; kv8 <= 1; ++kv8) {
            const DecodePlan p = make_decode_plan(k, rk, true, B, 4096, 24, 16, 96, 1536, ch, false, kv8 != 0);
            std::printf("P %d %d %d %d %d %d %d %d\n", B, kv8, p.sel.decode_version, p.sel.attn_kernel, p.sel.merge_launch, (int)p.kv8,
                        (int)p.stream_attn, (int)p.v3);
            if (kv8) std::printf("S %d %d\n", B, (int)make_decode_plan(k, rk, true, B, 4096, 24, 16, 96, 1536, ch, true, true).shared_attn);
        }
    DecodeKnobs split = k;                                // ER_ATTN_V_BATCHED=1 asks for the round-1 split kernel, which reads no bytes
    split.attn_v_batched = 1;
    const DecodePlan p = make_decode_plan(split, rk, true, 8, 4096, 24, 16, 96, 1536, ch, false, true);
    std::printf("P %d %d %d %d %d %d %d %d\n", 8, 2, p.sel.decode_version, p.sel.attn_kernel, p.sel.merge_launch, (int)p.kv8, (int)p.stream_attn, (int)p.v3);
}

int main() {
    if (check_map()) return 1;
    encode_sweep();
    plan_lines();
    std::printf("kv8_map_check: ok\n");
    return 0;
}
