// Stand-alone check of the rule that names the weight copy each decode projection streams (edgerunner_amd/csrc/er_weight_source.h
// weight_source): every mode, batch, reserve switch, fused launch, row class, cache type and knob a context can have for the 16 x 96
// decoder, held against the conditions written out below and against the relations its readers rely on.  No device call: build with the
// host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o weight_source_check tests/host/weight_source_check.cpp
// (tests/test_weight_source_cpu.py does).  Exit status 0 = every check held.  With --dump it prints one line per case:
//     <mode> B=<n> force=<0|1> valu=<0|1> xt=<0|1> v=<2|3> mlp=<0|1> rc=<0|1> kv8=<0|1> w8b=<k> w4r=<k> w4b=<k> L=<layer> <proj> <source>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../edgerunner_amd/csrc/er_weight_source.h"

#define CHECK(cond)                                                                                                        \
    do {                                                                                                                   \
        if (!(cond)) {                                                                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at %s\n", __FILE__, __LINE__, #cond, where);                          \
            exit(1);                                                                                                       \
        }                                                                                                                  \
    } while (0)

using namespace er;

struct Case { WMode mode; int B; ReserveKnobs rk; int decode_v, mlp_v; bool row_class, kv8; int w8b, w4r, w4b; };

// The source of `proj` as the conditions of the step state it, written out without proj_form or the primitive rules.
static WSrc expected(const Case& c, Proj proj) {
    if (proj == PROJ_HEAD) return WSRC_PLAIN;
    const bool batched = c.B > 4 || c.rk.force_batched, one_row = c.B == 1 && !batched && !c.row_class;
    if (proj == PROJ_OUT && one_row && c.decode_v == 3 && !c.kv8) return c.mode == W_FP8 ? WSRC_BYTES : WSRC_PLAIN;      // the fused merge launch
    if ((proj == PROJ_FC1 || proj == PROJ_FC2) && one_row && c.mlp_v != 0) return proj == PROJ_FC2 ? WSRC_KMAJOR : WSRC_PLAIN;      // the fused MLP
    if (!batched) {      // row forms
        if (c.mode == W_FP8) return proj != PROJ_OUT || c.B <= 2 ? WSRC_BYTES : WSRC_PLAIN;
        if (c.mode == W_FP4 && proj != PROJ_OUT && c.w4r != 0)
            return c.w4r == 1 || proj == PROJ_FC1 || proj == PROJ_FC2 || c.B == 1 ? WSRC_QUADS : WSRC_PLAIN;
        return WSRC_PLAIN;
    }
    // batched: the matrix cores unless ER_BATCHED_VALU=1, and out_proj of 5 .. 8 rows is the eight-row VALU pass
    if (c.rk.batched_valu || (proj == PROJ_OUT && c.B >= 5 && c.B <= 8)) return WSRC_PLAIN;
    if (c.mode == W_FP8 && c.w8b != 0) return c.w8b == 1 || (c.B > 4 && proj != PROJ_OUT) ? WSRC_TILED_BYTES : WSRC_TILED;
    if (c.mode == W_FP4 && c.w4b != 0 && c.B > 4) return WSRC_TILED_NIBBLES;
    return WSRC_TILED;
}

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !strcmp(argv[1], "--dump");
    const int HEADS = 16, D = 96, HID = 1536, LAYERS = 24, LCAP = 2048;
    const AttnChunking ch{16, 16 * 512, 128};      // the 16-head decoder: 16 chunks of 512 keys (balanced kernel), 128-key chunks (fixed-chunk kernels)
    const char* mname[] = {"exact", "fast", "fp8", "fp4"};
    const char* pname[] = {"qkv", "out", "fc1", "fc2", "head"};
    const char* sname[] = {"plain", "tiled", "bytes", "tiled_bytes", "quads", "tiled_nibbles", "kmajor"};
    const int batches[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 40, 64};
    long cases = 0;
    char where[256] = "";
    for (int mi = 0; mi < 4; ++mi)
    for (int B : batches)
    for (int sw = 0; sw < 8; ++sw)
    for (int decode_v : {2, 3})
    for (int mlp_v : {0, 1})
    for (int rc = 0; rc <= 1; ++rc)
    for (int kv8 = 0; kv8 <= (mi == W_EXACT ? 0 : 1); ++kv8)      // the byte cache goes with fp16, byte or nibble weights
    for (int w8b = -1; w8b <= (mi == W_FP8 ? 1 : -1); ++w8b)       // each knob in the mode it belongs to
    for (int w4r = -1; w4r <= (mi == W_FP4 ? 1 : -1); ++w4r)
    for (int w4b = -1; w4b <= (mi == W_FP4 ? 1 : -1); ++w4b) {
        const Case c{(WMode)mi, B, ReserveKnobs{(sw & 1) != 0, (sw & 2) != 0, (sw & 4) != 0}, decode_v, mlp_v, rc != 0, kv8 != 0, w8b, w4r, w4b};
        DecodeKnobs k;
        k.decode_v = decode_v; k.mlp_v = mlp_v; k.w8_batched = w8b; k.w4_rows = w4r; k.w4_batched = w4b;
        const bool half = c.mode != W_EXACT;
        const DecodePlan p = make_decode_plan(k, c.rk, half, B, LCAP, LAYERS, HEADS, D, HID, ch, false, c.kv8);
        const bool v3 = p.v3 && !c.row_class, fused = p.mlp_fused && !c.row_class;
        int32_t rep8[4] = {}, rep4[4] = {}, rep4b[4] = {};
        for (int layer : {0, LAYERS - 1})
            for (int pi = 0; pi < 5; ++pi) {
                const Proj proj = (Proj)pi;
                snprintf(where, sizeof(where), "%s B=%d force=%d valu=%d xt=%d v=%d mlp=%d rc=%d kv8=%d w8b=%d w4r=%d w4b=%d L=%d %s", mname[mi], B,
                         c.rk.force_batched, c.rk.batched_valu, c.rk.xt, decode_v, mlp_v, rc, kv8, w8b, w4r, w4b, layer, pname[pi]);
                const WSrc s = weight_source(p, k, c.mode, c.row_class, proj, layer);
                ++cases;
                if (dump) printf("%s %s\n", where, sname[s]);
                CHECK(s >= WSRC_PLAIN && s < WSRC_COUNT);
                CHECK(s == expected(c, proj));
                CHECK(s == weight_source(p, k, c.mode, c.row_class, proj, 0));      // one copy per projection: ensure_weight_copies asks layer 0
                const int form = proj_form(p, k, half, proj, layer).form;
                const bool merge = v3 && proj == PROJ_OUT, in_mlp = fused && (proj == PROJ_FC1 || proj == PROJ_FC2);
                // a quantised source only in its own mode; exact mode only plain, tiled or k-major
                CHECK(!wsrc_bytes(s) || c.mode == W_FP8);
                CHECK(!wsrc_nibbles(s) || c.mode == W_FP4);
                if (c.mode == W_EXACT || c.mode == W_FAST) CHECK(s == WSRC_PLAIN || s == WSRC_TILED || s == WSRC_KMAJOR);
                // tiled sources with the matrix-core forms and only with them; row sources with ER_FORM_ROW or the fused merge launch
                CHECK(wsrc_tiled(s) == (form_mfma(form) && !merge && !in_mlp));
                if (s == WSRC_QUADS) CHECK(form == ER_FORM_ROW && !merge && !in_mlp);
                if (s == WSRC_BYTES) CHECK(form == ER_FORM_ROW && !in_mlp);
                if (merge) CHECK(s == (c.mode == W_FP8 ? WSRC_BYTES : WSRC_PLAIN));
                if (proj == PROJ_HEAD || form == ER_FORM_VALU || form == ER_FORM_ROWS8) CHECK(s == WSRC_PLAIN);
                CHECK((s == WSRC_KMAJOR) == (fused && proj == PROJ_FC2));
                if (fused && proj == PROJ_FC1) CHECK(s == WSRC_PLAIN);
                CHECK(wsrc_derived(s) == (s != WSRC_PLAIN && s != WSRC_BYTES));
                if (layer == 0 && pi < 4) { rep8[pi] = wsrc_bytes(s); rep4[pi] = s == WSRC_QUADS; rep4b[pi] = s == WSRC_TILED_NIBBLES; }
            }
        // what er_ctx_w8_streams, er_ctx_w4_streams and er_ctx_w4_streams_batched report, stated from the primitive rules
        for (int pi = 0; pi < 4; ++pi) {
            const Proj proj = (Proj)pi;
            snprintf(where, sizeof(where), "reporters: %s B=%d sw=%d v=%d mlp=%d rc=%d kv8=%d w8b=%d w4r=%d w4b=%d %s", mname[mi], B, sw, decode_v, mlp_v, rc, kv8, w8b, w4r, w4b, pname[pi]);
            const int form = proj_form(p, k, true, proj, 0).form;
            const bool in_mlp = fused && (proj == PROJ_FC1 || proj == PROJ_FC2);
            bool bytes = false;
            if (c.mode != W_FP8 || in_mlp) bytes = false;
            else if (proj == PROJ_OUT && v3) bytes = w8_streams(PROJ_OUT, 1);
            else if (form == ER_FORM_ROW) bytes = w8_streams(proj, B);
            else bytes = form_mfma(form) && w8_streams_batched(proj, B, w8b);
            CHECK(rep8[pi] == (bytes ? 1 : 0));
            CHECK(rep4[pi] == (c.mode == W_FP4 && !p.batched && !in_mlp && w4_streams(proj, B, w4r) ? 1 : 0));
            CHECK(rep4b[pi] == (c.mode == W_FP4 && p.batched && form_mfma(form) && w4_streams_batched(proj, B, w4b) ? 1 : 0));
        }
    }
    if (!dump) printf("weight_source_check: ok (%ld cases)\n", cases);
    return 0;
}
