// Stand-alone check of the decode step's decision table (edgerunner_amd/csrc/er_decode_plan.h): every plan a reserve can produce for
// the 16 x 96 decoder, every projection's form under it, the relations launch_kind_t relies on, and the list of distinct
// (projection, form, waves x rows, weight type) the step can reach.  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o decode_plan_check tests/host/decode_plan_check.cpp
// (tests/test_decode_plan_cpu.py does).  Exit status 0 = every check held; the reached tuples are printed one per line.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

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
    const int HEADS = 16, D = 96, HID = 1536, LAYERS = 24;
    const AttnChunking ch{16, 16 * 512, 128};      // the 16-head decoder: 16 chunks of 512 keys (balanced kernel), 128-key chunks (fixed-chunk kernels)
    const char* pname[] = {"qkv", "out", "fc1", "fc2", "head"};
    const char* fname[] = {"row", "rows8", "valu", "mfma", "xt", "narrow", "defer"};
    std::set<std::string> reached;
    long plans = 0;
    char where[256] = "";
    for (int bi = 1; bi <= 41; ++bi) {
        const int B = bi <= 40 ? bi : 64;
        for (int half = 0; half <= 1; ++half)
        for (int decode_v : {2, 3})
        for (int attn_v : {0, 1, 3})
        for (int sw = 0; sw < 8; ++sw)
        for (int nw_qkv : {4, 6, 9})
        for (int nw_fc1 : {4, 12})
        for (int rw_fc2 : {2, 4, 6})
        for (int Lcap : {64, 8192, 8224}) {
            DecodeKnobs k;
            k.decode_v = decode_v; k.attn_v_batched = attn_v; k.nw_qkv = nw_qkv; k.nw_fc1 = nw_fc1; k.rw_fc2 = rw_fc2;
            const ReserveKnobs rk{(sw & 1) != 0, (sw & 2) != 0, (sw & 4) != 0};
            const DecodePlan p = make_decode_plan(k, rk, half != 0, B, Lcap, LAYERS, HEADS, D, HID, ch);
            snprintf(where, sizeof(where), "B=%d half=%d decode_v=%d attn_v=%d force=%d valu=%d xt=%d nw_qkv=%d nw_fc1=%d rw_fc2=%d Lcap=%d",
                     B, half, decode_v, attn_v, rk.force_batched, rk.batched_valu, rk.xt, nw_qkv, nw_fc1, rw_fc2, Lcap);
            ++plans;
            // the plan's own flags
            CHECK(p.batched == (B > 4 || rk.force_batched));
            CHECK(p.mfma == (p.batched && !rk.batched_valu));
            CHECK(p.xt == (half && p.mfma && rk.xt));
            CHECK(p.v3 == (decode_v == 3 && B == 1 && !rk.force_batched && Lcap <= 8192));
            CHECK(p.S_splits * 128 >= Lcap && (p.S_splits - 1) * 128 < Lcap);
            CHECK(p.stream_attn == (p.batched && (attn_v == 3 || (attn_v == 0 && B * HEADS >= 256))));
            CHECK(p.sel.merge_launch == (!p.v3 && !p.stream_attn));
            CHECK(!p.outproj_partials || (p.xt && p.stream_attn && B > 8));
            for (int layer : {0, LAYERS / 2, LAYERS - 1})
                for (int pi = 0; pi < 5; ++pi) {
                    const Proj proj = (Proj)pi;
                    const ProjForm f = proj_form(p, k, half != 0, proj, layer);
                    CHECK(f.form >= ER_FORM_ROW && f.form <= ER_FORM_NARROW_DEFER);
                    CHECK(proj_form_legal(proj, f, half != 0, B));
                    CHECK(form_batched(f.form) == (p.batched && f.form != ER_FORM_ROWS8));
                    CHECK(half || !form_tiled_in(f.form));                       // no tiled form with fp32 weights
                    CHECK(f.defer == (f.form == ER_FORM_NARROW_DEFER));
                    if (proj == PROJ_FC2) CHECK(f.defer == (p.xt && layer != LAYERS - 1));     // what the next layer's LayerNorm launch asks
                    if (proj == PROJ_FC2) CHECK(f.defer == p.fc2_defers(layer));
                    if (proj == PROJ_OUT) CHECK(f.defer == p.outproj_partials);               // what fc1's LayerNorm launch asks
                    if (proj == PROJ_OUT) CHECK((f.form == ER_FORM_ROWS8) == (p.mfma && B >= 5 && B <= 8));
                    CHECK(f.form != ER_FORM_ROWS8 || proj == PROJ_OUT);
                    if (proj != PROJ_OUT && proj != PROJ_FC2) CHECK(!f.defer);
                    if (p.xt && proj != PROJ_HEAD && f.form != ER_FORM_ROWS8 && !(proj == PROJ_OUT && !p.outproj_partials)) CHECK(form_tiled_in(f.form));
                    char t[64];
                    snprintf(t, sizeof(t), "%s %s %dx%d %s", pname[pi], fname[f.form], f.nw, f.rw, half ? "fp16" : "fp32");
                    reached.insert(t);
                }
            CHECK(!proj_form(p, k, half != 0, PROJ_FC2, -1).defer);              // layer 0 asks its (absent) predecessor
        }
    }
    // what the step can NOT launch is not legal
    snprintf(where, sizeof(where), "refusals");
    CHECK(!proj_form_legal(PROJ_QKV, ProjForm{ER_FORM_ROW, 12, 2, false}, true, 3));
    CHECK(!proj_form_legal(PROJ_QKV, ProjForm{ER_FORM_ROW, 9, 2, false}, true, 5));
    CHECK(!proj_form_legal(PROJ_OUT, ProjForm{ER_FORM_ROW, 4, 1, false}, false, 1));
    CHECK(!proj_form_legal(PROJ_FC2, ProjForm{ER_FORM_ROW, 4, 6, false}, true, 2));
    CHECK(!proj_form_legal(PROJ_FC2, ProjForm{ER_FORM_ROW, 4, 6, false}, false, 1));
    CHECK(!proj_form_legal(PROJ_FC2, ProjForm{ER_FORM_NARROW, 0, 0, false}, false, 5));
    CHECK(!proj_form_legal(PROJ_OUT, ProjForm{ER_FORM_NARROW, 0, 0, false}, true, 40));
    CHECK(!proj_form_legal(PROJ_OUT, ProjForm{ER_FORM_NARROW_DEFER, 0, 0, false}, true, 40));
    CHECK(!proj_form_legal(PROJ_HEAD, ProjForm{ER_FORM_MFMA, 0, 0, false}, true, 5));
    CHECK(!proj_form_legal(PROJ_FC1, ProjForm{ER_FORM_ROWS8, 3, 1, false}, true, 5));
    CHECK(!proj_form_legal(PROJ_OUT, ProjForm{ER_FORM_ROWS8, 3, 1, false}, true, 9));
    CHECK(!proj_form_legal(PROJ_QKV, ProjForm{ER_FORM_MFMA_XT, 0, 0, false}, false, 8));
    CHECK(!proj_form_legal(PROJ_QKV, ProjForm{ER_FORM_PREP, 0, 0, false}, true, 8));
    for (const std::string& t : reached) printf("reached %s\n", t.c_str());
    printf("decode_plan_check: ok (%ld plans)\n", plans);
    return 0;
}
