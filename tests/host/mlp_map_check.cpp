// Stand-alone check of the fused single-row MLP's host-side rules: the neuron map of edgerunner_amd/csrc/er_mlp_map.h (which
// workgroup owns which fc1 neurons, in which order) and the plan flag that selects the fused launches (er_decode_plan.h).  No device
// call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o mlp_map_check tests/host/mlp_map_check.cpp
// (tests/test_mlp_sparse_cpu.py does).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../edgerunner_amd/csrc/er_decode_plan.h"
#include "../../edgerunner_amd/csrc/er_mlp_map.h"

#define CHECK(cond)                                                                                 \
    do {                                                                                            \
        if (!(cond)) {                                                                              \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at %s\n", __FILE__, __LINE__, #cond, where);   \
            exit(1);                                                                                \
        }                                                                                           \
    } while (0)

using namespace er;

int main() {
    char where[128] = "";
    static_assert(MLP_WGS == 256 && MLP_CHAIN == 24 && MLP_WGS * MLP_CHAIN == MLP_INTER, "256 chains of 24 neurons");
    for (int epl : {4, 8}) {      // fp32 / fp16 weights: elements per 16-byte load
        const int J = MLP_HIDDEN / (64 * epl);      // 16-byte loads per lane and slice in gemv_kernel
        CHECK(J * epl == MLP_CHAIN);
        // the map is gemv_kernel's index formula: the wave of slice s, lane l, load j, element e multiplies weight column
        // s * 1536 + (j * 64 + l) * epl + e, and a lane's chain takes (j, e) in ascending order
        std::vector<int> owner(MLP_INTER, -1);
        for (int s = 0; s < MLP_SLICES; ++s)
            for (int l = 0; l < 64; ++l) {
                int i = 0, prev = -1;
                for (int j = 0; j < J; ++j)
                    for (int e = 0; e < epl; ++e, ++i) {
                        snprintf(where, sizeof(where), "epl=%d slice=%d lane=%d j=%d e=%d", epl, s, l, j, e);
                        const int k = s * MLP_HIDDEN + (j * 64 + l) * epl + e;
                        CHECK(mlp_neuron(epl, s * 64 + l, i) == k);
                        CHECK(k > prev);                                   // ascending along the chain
                        prev = k;
                        CHECK(k >= 0 && k < MLP_INTER && owner[k] == -1);   // nobody else owns it
                        owner[k] = (s * 64 + l) * MLP_CHAIN + i;
                        const MlpSlot t = mlp_slot(epl, k);
                        CHECK(t.wg == s * 64 + l && t.i == i);
                    }
                CHECK(i == MLP_CHAIN);
            }
        // a bijection on 0 .. 6143, and mlp_slot is its inverse
        for (int k = 0; k < MLP_INTER; ++k) {
            snprintf(where, sizeof(where), "epl=%d k=%d", epl, k);
            CHECK(owner[k] >= 0);
            const MlpSlot t = mlp_slot(epl, k);
            CHECK(t.wg >= 0 && t.wg < MLP_WGS && t.i >= 0 && t.i < MLP_CHAIN);
            CHECK(mlp_neuron(epl, t.wg, t.i) == k);
        }
    }

    // the plan: fused only for one row, not batched, hidden 1536, knob on
    const AttnChunking ch{16, 16 * 512, 128};
    for (int mlp_v : {0, 1})
        for (int B : {1, 2, 3, 4, 5, 16})
            for (int half = 0; half <= 1; ++half)
                for (int force = 0; force <= 1; ++force)
                    for (int hid : {1536, 1024})
                        for (int decode_v : {2, 3}) {
                            snprintf(where, sizeof(where), "mlp_v=%d B=%d half=%d force=%d hid=%d decode_v=%d", mlp_v, B, half, force, hid, decode_v);
                            DecodeKnobs k;
                            k.mlp_v = mlp_v; k.decode_v = decode_v;
                            const ReserveKnobs rk{force != 0, false, true};
                            const int H = 16, D = hid / H;
                            const DecodePlan p = make_decode_plan(k, rk, half != 0, B, 4096, 24, H, D, hid, ch);
                            CHECK(p.mlp_fused == (mlp_v != 0 && B == 1 && !force && hid == 1536));
                            CHECK(!p.mlp_fused || !p.batched);
                            CHECK(p.sel.launches_per_layer == (p.batched ? 0 : 5 + p.sel.merge_launch));      // the fused pair takes the places of fc1 and fc2
                        }
    CHECK(DecodeKnobs{}.mlp_v == 0);
    printf("mlp_map_check: ok\n");
    return 0;
}
