// Stand-alone check of which fc2 rows the fused single-row MLP requests (edgerunner_amd/csrc/er_mlp_map.h: mlp_live_count,
// mlp_live_slots, mlp_live_peel, mlp_live_lane, mlp_live_place) for all 4096 live masks of a half-chain, and of the claim that running
// the chain over the compacted slots gives what the 12-step chain with zeros gives.  No device call: build with the host sanitizers
// and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o mlp_live_check tests/host/mlp_live_check.cpp
// (tests/test_mlp_live_cpu.py does).  Exit status 0 = every check held.
//
// The chain: the row kernel runs s = fmaf(w_i, f_i, s) over all 12 places, a dead place with f_i = +0 and a finite w_i; the fused
// kernel of the parent form ran fmaf(+0, +0, s) there; the compacted form runs the live places in the same order, then
// fmaf(+0, +0, s) for the pads of the last block, and nothing for the rest.  A left-out step fmaf(+-0, +0, s) returns s for every
// s but a zero, and for a zero s it returns a zero: the two chains can differ only in the SIGN OF A ZERO result.  The finish tree
// adds chain values pairwise and its last stage starts from +0 ((0 + p0) + p1 ...): a zero of either sign added to a non-zero value
// leaves it unchanged, added to a zero it gives a zero, and +0 + (+-0) = +0, so no bit of the output depends on that sign.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../edgerunner_amd/csrc/er_mlp_map.h"

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at %s\n", __FILE__, __LINE__, #cond, where);   \
            exit(1);                                                                                \
        }                                                                                           \
    } while (0)

using namespace er;

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd_float() {                     // magnitudes over many decades, both signs, now and then a zero of either sign
    const uint32_t r = rnd();
    if (r % 17 == 0) return (r & 32) ? 0.0f : -0.0f;
    const float m = (float)(rnd() & 0xffff) / 65536.f + 0.5f;
    return ((r & 1) ? m : -m) * std::ldexp(1.0f, (int)(r >> 4) % 60 - 45);
}

int main() {
    char where[160] = "";
    static_assert(MLP_HALF == 12 && MLP_LIVE_BLOCK == 4 && MLP_PAD_LANE == 12 && MLP_HALF_MASK == 0xfffu, "two halves of 12 places, blocks of 4");
    static_assert(mlp_live_slots(0u) == 0 && mlp_live_slots(1u) == 4 && mlp_live_slots(0xfu) == 4 && mlp_live_slots(0x1fu) == 8 && mlp_live_slots(0xfffu) == 12, "");
    static_assert(mlp_live_place(0x804u, 0) == 2 && mlp_live_place(0x804u, 1) == 11 && mlp_live_place(0x804u, 2) == -1, "");
    long chains = 0, zero_sign = 0;
    for (unsigned mask = 0; mask < (1u << MLP_HALF); ++mask) {
        snprintf(where, sizeof(where), "mask=0x%03x", mask);
        // the padded count: the next multiple of 4, 0 for the empty mask
        int n = 0;
        for (int i = 0; i < MLP_HALF; ++i) n += (mask >> i) & 1;
        CHECK(mlp_live_count(mask) == n);
        const int slots = mlp_live_slots(mask);
        CHECK(slots % MLP_LIVE_BLOCK == 0 && slots >= n && slots < n + MLP_LIVE_BLOCK && slots <= MLP_HALF);
        CHECK((mask == 0) == (slots == 0));
        // the slots list exactly the set bits, in ascending place order; behind them pads
        unsigned seen = 0;
        int prev = -1;
        for (int u = 0; u < MLP_HALF; ++u) {
            const int p = mlp_live_place(mask, u);
            if (u < n) {
                CHECK(p > prev && p < MLP_HALF && ((mask >> p) & 1));
                seen |= 1u << p;
                prev = p;
            } else {
                CHECK(p == -1);
            }
        }
        CHECK(seen == mask);
        // the kernel's walk: lane i < 12 keeps place i (f, and the row of a live place), the lanes from 12 on f = 0 and the zero row;
        // slot u reads lane mlp_live_lane of the mask peeled u times
        for (int trial = 0; trial < 6; ++trial) {
            float w[MLP_HALF], f[MLP_HALF], lane_f[MLP_PAD_LANE + 1], lane_w[MLP_PAD_LANE + 1];
            int lane_row[MLP_PAD_LANE + 1];
            for (int i = 0; i < MLP_HALF; ++i) {
                w[i] = rnd_float();
                float a = std::fabs(rnd_float());
                if (a == 0.f) a = 1.f;
                f[i] = ((mask >> i) & 1) ? a : 0.f;        // relu output: positive where alive
                lane_f[i] = f[i];
                lane_row[i] = f[i] != 0.f ? i : -1;        // -1: the zero row
                lane_w[i] = f[i] != 0.f ? w[i] : 0.f;
            }
            if (trial == 1 && n > 0) {                     // a product that underflows to -0 on a +0 sum
                const int p = mlp_live_place(mask, 0);
                w[p] = lane_w[p] = -1e-30f;
                f[p] = lane_f[p] = 1e-30f;
            }
            lane_f[MLP_PAD_LANE] = 0.f; lane_row[MLP_PAD_LANE] = -1; lane_w[MLP_PAD_LANE] = 0.f;
            const float starts[4] = {0.f, -0.f, rnd_float(), trial == 1 ? 0.f : rnd_float()};
            for (float s0 : starts) {
                float full = s0, parent = s0, comp = s0;
                for (int i = 0; i < MLP_HALF; ++i) {
                    full = std::fmaf(w[i], f[i], full);                                   // the row kernel
                    parent = std::fmaf(f[i] != 0.f ? w[i] : 0.f, f[i], parent);           // zero row for a dead place
                }
                unsigned m = mask;
                for (int u = 0; u < slots; ++u) {
                    const int lane = mlp_live_lane(m);
                    m = mlp_live_peel(m);
                    CHECK(lane == (u < n ? mlp_live_place(mask, u) : MLP_PAD_LANE));
                    if (u >= n) CHECK(lane_f[lane] == 0.f && bits(lane_f[lane]) == 0u && lane_row[lane] == -1);      // a pad: f = +0, the zero row
                    else CHECK(lane_row[lane] == lane && lane_f[lane] == f[lane]);
                    comp = std::fmaf(lane_w[lane], lane_f[lane], comp);
                }
                CHECK(m == 0u || slots == MLP_HALF);
                ++chains;
                for (float other : {full, parent}) {
                    if (bits(comp) != bits(other)) {
                        CHECK(comp == 0.f && other == 0.f);                               // only the sign of a zero
                        ++zero_sign;
                    }
                    CHECK(bits(0.f + comp) == bits(0.f + other));                         // the finish's last stage starts from +0
                    const float y = rnd_float();
                    if (y != 0.f) CHECK(bits(comp + y) == bits(other + y));               // a tree add with a non-zero partner
                    CHECK((comp + y == 0.f) == (other + y == 0.f));                       // with a zero partner: a zero either way
                }
            }
        }
    }
    CHECK(zero_sign > 0);                      // the -0 case was exercised
    printf("mlp_live_check: ok (4096 masks, %ld chains, %ld differ in the sign of a zero)\n", chains, zero_sign);
    return 0;
}
