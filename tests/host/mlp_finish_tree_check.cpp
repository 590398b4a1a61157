// Stand-alone check of the finish launch's lane mapping and sum tree (edgerunner_amd/csrc/er_mlp_map.h: mlp_fin_chain, mlp_fin_piece,
// mlp_fin_level), for NC = 8, 16, 32 outputs per workgroup.  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o mlp_finish_tree_check tests/host/mlp_finish_tree_check.cpp
// (tests/test_mlp_finish_cpu.py does).  Exit status 0 = every check held.
//
//   1. (load, lane) -> (chain, piece) covers each of a slice's 64 chains x NC / 4 pieces exactly once.
//   2. The level schedule, run the way mlp_finish_kernel runs it (register levels fold load j ^ off into load j, lane levels add lane
//      l ^ off to lane l in every lane), gives in EVERY lane that ends up holding a result the bit pattern of the plain 64-lane
//      butterfly (v[l] + v[l ^ 32], then 16, 8, 4, 2, 1) over the chain index: random vectors whose magnitudes span twelve decades,
//      vectors with +0 / -0 entries, vectors with one huge element.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../edgerunner_amd/csrc/er_mlp_map.h"

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at %s\n", __FILE__, __LINE__, #cond, where);   \
            exit(1);                                                                                \
        }                                                                                           \
    } while (0)

using namespace er;

static char where[160] = "";

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// wave_sum of er_common.h on a host array: six levels, every lane computes v[l] + v[l ^ off]
static float butterfly(const float* v) {
    float a[64], b[64];
    memcpy(a, v, sizeof(a));
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ off];
        memcpy(a, b, sizeof(a));
    }
    for (int l = 1; l < 64; ++l)
        if (bits(a[l]) != bits(a[0])) { fprintf(stderr, "butterfly: lanes disagree\n"); exit(1); }
    return a[0];
}

// the kernel's schedule for ONE output column: r[lane][load] holds the chain value the lane loaded; returns lane 0's r[0] after
// checking that every lane of chain 0 .. (all lanes, in fact: the lane levels are butterflies) agrees with it
static float kernel_tree(int nc, const float* chain_val) {
    const int g = mlp_fin_group(nc);
    std::vector<float> r(64 * g), t(64 * g);
    // only the lanes of one piece take part in a column's sum: piece 0 here (the others run the same schedule on other columns)
    for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < g; ++j) r[lane * g + j] = chain_val[mlp_fin_chain(nc, j, lane)];
    for (int k = 0; k < MLP_FIN_LEVELS; ++k) {
        const MlpFinLevel lv = mlp_fin_level(nc, k);
        if (lv.reg) {
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < lv.off; ++j) r[lane * g + j] = r[lane * g + j] + r[lane * g + (j ^ lv.off)];
        } else {
            for (int lane = 0; lane < 64; ++lane) t[lane * g] = r[lane * g] + r[(lane ^ lv.off) * g];
            for (int lane = 0; lane < 64; ++lane) r[lane * g] = t[lane * g];
        }
    }
    // lanes with the same piece hold the same bits; the kernel takes the lane of chain 0
    for (int lane = 0; lane < 64; ++lane)
        if (mlp_fin_piece(nc, lane) == 0) CHECK(bits(r[lane * g]) == bits(r[0]));
    return r[0];
}

int main() {
    int vectors = 0;
    for (int nc : {8, 16, 32}) {
        const int g = mlp_fin_group(nc), cpl = mlp_fin_chains_per_load(nc);
        snprintf(where, sizeof(where), "nc=%d", nc);
        CHECK(mlp_fin_nc_ok(nc) && g * 4 == nc && g * cpl == 64);
        // 1. the cover
        std::vector<int> seen(64 * g, 0);
        for (int j = 0; j < g; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                snprintf(where, sizeof(where), "nc=%d load=%d lane=%d", nc, j, lane);
                const int c = mlp_fin_chain(nc, j, lane), p = mlp_fin_piece(nc, lane);
                CHECK(c >= 0 && c < 64 && p >= 0 && p < g);
                CHECK(seen[c * g + p] == 0);
                seen[c * g + p] = 1;
                // a wave-load reads g adjacent lanes' pieces of one chain as one contiguous run, chains ascending with the lane
                CHECK(p == lane % g && c == j * cpl + lane / g);
            }
        for (int i = 0; i < 64 * g; ++i) CHECK(seen[i] == 1);
        // the schedule is a permutation of the butterfly's levels: chain xor 32 >> k at level k
        for (int k = 0; k < MLP_FIN_LEVELS; ++k) {
            snprintf(where, sizeof(where), "nc=%d level=%d", nc, k);
            const MlpFinLevel lv = mlp_fin_level(nc, k);
            const int x = 32 >> k;
            if (lv.reg) {
                CHECK(lv.off >= 1 && lv.off < g);
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < g; ++j) CHECK(mlp_fin_chain(nc, j ^ lv.off, lane) == (mlp_fin_chain(nc, j, lane) ^ x));
            } else {
                CHECK(lv.off >= g && lv.off < 64);
                for (int lane = 0; lane < 64; ++lane) {
                    CHECK(mlp_fin_chain(nc, 0, lane ^ lv.off) == (mlp_fin_chain(nc, 0, lane) ^ x));
                    CHECK(mlp_fin_piece(nc, lane ^ lv.off) == mlp_fin_piece(nc, lane));
                }
            }
        }

        // 2. the bits
        std::mt19937 rng(1234 + nc);
        std::uniform_real_distribution<float> mant(-1.0f, 1.0f), expo(-6.0f, 6.0f);
        std::uniform_int_distribution<int> pick(0, 63), coin(0, 3);
        float v[64];
        for (int it = 0; it < 12000; ++it) {
            snprintf(where, sizeof(where), "nc=%d random vector %d", nc, it);
            for (int l = 0; l < 64; ++l) v[l] = mant(rng) * powf(10.0f, expo(rng));
            CHECK(bits(kernel_tree(nc, v)) == bits(butterfly(v)));
            ++vectors;
        }
        for (int it = 0; it < 4000; ++it) {      // signed zeros (a dead chain's sum is +0, -0 must not survive differently) and one huge element
            snprintf(where, sizeof(where), "nc=%d zero / huge vector %d", nc, it);
            for (int l = 0; l < 64; ++l) {
                const int c = coin(rng);
                v[l] = c == 0 ? 0.0f : c == 1 ? -0.0f : mant(rng) * powf(10.0f, expo(rng));
            }
            if (it % 4 == 1) for (int l = 0; l < 64; ++l) v[l] = (l & 1) ? -0.0f : 0.0f;
            if (it % 4 == 2) for (int l = 0; l < 64; ++l) v[l] = -0.0f;
            if (it % 2 == 1) v[pick(rng)] = (it % 4 == 1 ? 1.0f : -1.0f) * 3.0e37f;
            CHECK(bits(kernel_tree(nc, v)) == bits(butterfly(v)));
            ++vectors;
        }
    }
    printf("mlp_finish_tree_check: ok (%d vectors)\n", vectors);
    return 0;
}
