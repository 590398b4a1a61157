// Stand-alone check of the prefix-pass rule of the decode plan (edgerunner_amd/csrc/er_decode_plan.h): over every batch, storage mode,
// head_dim, prefix-pass knob and reserve switch, make_decode_plan sets shared_mfma exactly when prefix groups are set on a batched
// shape with an fp16 cache at head_dim 96 and the knob asks for the matrix-core pass - never with a byte cache (kv8), never without
// groups - and reports it as ER_ATTN_SHARED_MFMA with a merge launch; the shape-only rule (plan_decode) never names a shared kernel,
// and nothing else of the plan moves with the knob.  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o prefix_pass_plan_check tests/host/prefix_pass_plan_check.cpp
// (tests/test_prefix_pass_cpu.py does).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../edgerunner_amd/csrc/er_decode_plan.h"

#define CHECK(cond)                                                                                                        \
    do {                                                                                                                   \
        if (!(cond)) {                                                                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at %s\n", __FILE__, __LINE__, #cond, where);                          \
            exit(1);                                                                                                       \
        }                                                                                                                  \
    } while (0)

using namespace er;

int main() {
    const int HEADS = 16, LAYERS = 24;
    const AttnChunking ch{16, 16 * 512, 128};
    long plans = 0, mfma_plans = 0;
    char where[256] = "";
    static_assert(ER_PREFIX_PASS_VALU == 0 && ER_PREFIX_PASS_MFMA == 1 && ER_ATTN_SHARED == 5 && ER_ATTN_SHARED_MFMA == 6, "the ABI's values");
    CHECK(DecodeKnobs{}.prefix_pass == ER_PREFIX_PASS_VALU);      // off by default
    for (int bi = 1; bi <= 41; ++bi) {
        const int B = bi <= 40 ? bi : 64;
        for (int D : {64, 96})
        for (int fast = 0; fast <= 1; ++fast)
        for (int kv8 = 0; kv8 <= fast; ++kv8)          // a byte cache comes with fast weights only
        for (int shared = 0; shared <= 1; ++shared)
        for (int pass : {ER_PREFIX_PASS_VALU, ER_PREFIX_PASS_MFMA})
        for (int attn_v : {0, 1, 3})
        for (int sw = 0; sw < 8; ++sw)
        for (int Lcap : {64, 8192, 8224}) {
            DecodeKnobs k;
            k.attn_v_batched = attn_v; k.prefix_pass = pass;
            const ReserveKnobs rk{(sw & 1) != 0, (sw & 2) != 0, (sw & 4) != 0};
            const int hid = HEADS * D;
            const DecodePlan p = make_decode_plan(k, rk, fast != 0, B, Lcap, LAYERS, HEADS, D, hid, ch, shared != 0, kv8 != 0);
            snprintf(where, sizeof(where), "B=%d D=%d fast=%d kv8=%d shared=%d pass=%d attn_v=%d force=%d valu=%d xt=%d Lcap=%d", B, D, fast, kv8,
                     shared, pass, attn_v, rk.force_batched, rk.batched_valu, rk.xt, Lcap);
            ++plans;
            const bool batched = B > 4 || rk.force_batched;
            CHECK(p.shared_attn == (shared && !kv8 && batched && D == 96));
            CHECK(p.shared_mfma == (shared && batched && fast && !kv8 && D == 96 && pass == ER_PREFIX_PASS_MFMA));
            CHECK(!p.shared_mfma || p.shared_attn);
            CHECK(!(p.shared_mfma && p.kv8));
            CHECK((p.sel.attn_kernel == ER_ATTN_SHARED_MFMA) == p.shared_mfma);
            CHECK((p.sel.attn_kernel == ER_ATTN_SHARED) == (p.shared_attn && !p.shared_mfma));
            if (p.shared_attn) CHECK(p.sel.merge_launch == 1 && p.sel.batched == 1 && !p.stream_attn);
            mfma_plans += p.shared_mfma;
            // the knob moves nothing but the kernel of kind 1
            DecodeKnobs k0 = k;
            k0.prefix_pass = ER_PREFIX_PASS_VALU;
            const DecodePlan p0 = make_decode_plan(k0, rk, fast != 0, B, Lcap, LAYERS, HEADS, D, hid, ch, shared != 0, kv8 != 0);
            CHECK(p0.shared_attn == p.shared_attn && !p0.shared_mfma && p0.batched == p.batched && p0.mfma == p.mfma && p0.xt == p.xt);
            CHECK(p0.stream_attn == p.stream_attn && p0.v3 == p.v3 && p0.outproj_partials == p.outproj_partials && p0.outproj_rows8 == p.outproj_rows8);
            CHECK(p0.sel.merge_launch == p.sel.merge_launch && p0.sel.decode_version == p.sel.decode_version && p0.S_splits == p.S_splits);
            for (int layer : {0, LAYERS - 1})
                for (int pi = 0; pi < 5; ++pi) {
                    const ProjForm f = proj_form(p, k, fast != 0, (Proj)pi, layer), f0 = proj_form(p0, k0, fast != 0, (Proj)pi, layer);
                    CHECK(f.form == f0.form && f.nw == f0.nw && f.rw == f0.rw && f.defer == f0.defer);
                }
            // the shape-only rule never reports a shared kernel
            er_decode_plan sel{};
            plan_decode(k.decode_v, k.attn_v_batched, rk.force_batched, B, HEADS, D, hid, Lcap, ch, &sel, kv8 != 0);
            CHECK(sel.attn_kernel != ER_ATTN_SHARED && sel.attn_kernel != ER_ATTN_SHARED_MFMA);
        }
    }
    snprintf(where, sizeof(where), "totals");
    CHECK(mfma_plans > 0);
    printf("prefix_pass_plan_check: ok (%ld plans, %ld with the matrix-core prefix pass)\n", plans, mfma_plans);
    return 0;
}
