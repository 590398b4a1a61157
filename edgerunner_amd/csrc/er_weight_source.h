// Which device copy of its matrix a decode projection streams: the sources, the measured rules of fp8 mode (w8_streams, w8_streams_batched;
// fp4 mode's are in er_w4_rule.h) and weight_source, the ONE function that composes them with proj_form.  The decode step (launch_kind_t),
// the builder of the derived copies (ensure_weight_copies), the reporters (er_ctx_w8_streams, er_ctx_w4_streams, er_ctx_w4_streams_batched)
// and the profile's byte accounting all read it and decide nothing themselves.  Pure C++ with no device call, like er_decode_plan.h, so
// that tests/host/weight_source_check.cpp can enumerate the whole table.
#pragma once
#include "er_decode_plan.h"
#include "er_w4_rule.h"

namespace er {

enum WMode { W_EXACT = 0, W_FAST, W_FP8, W_FP4 };      // fp32 weights; fp16; fp16 + e4m3 byte blocks; fp16 + MXFP4 blocks

enum WSrc {
    WSRC_PLAIN = 0,       // the row-major matrix as loaded: fp32 (exact mode) or fp16
    WSRC_TILED,           // ... tiled for the matrix cores (tile_weights_kernel)
    WSRC_BYTES,           // fp8 mode: the byte block, e4m3 [N][K] then a scale per row (k_gemv.h w8_scales)
    WSRC_TILED_BYTES,     // ... tiled (er_w8_tile_map.h)
    WSRC_QUADS,           // fp4 mode: the quad-interleaved nibble copy of the row kernels (er_w4_map.h)
    WSRC_TILED_NIBBLES,   // fp4 mode: the tiled nibble copy (er_w4_tile_map.h)
    WSRC_KMAJOR,          // fc2 k-major, [intermediate][hidden]: the fused single-row MLP (k_mlp_sparse.h)
    WSRC_COUNT
};
constexpr bool wsrc_tiled(WSrc s) { return s == WSRC_TILED || s == WSRC_TILED_BYTES || s == WSRC_TILED_NIBBLES; }
constexpr bool wsrc_bytes(WSrc s) { return s == WSRC_BYTES || s == WSRC_TILED_BYTES; }
constexpr bool wsrc_nibbles(WSrc s) { return s == WSRC_QUADS || s == WSRC_TILED_NIBBLES; }
// a copy the context makes of a loaded matrix (the plain matrix and the byte block are what the weight table loads)
constexpr bool wsrc_derived(WSrc s) { return s != WSRC_PLAIN && s != WSRC_BYTES; }

// Which projections of an fp8 context stream bytes in their row forms at B rows.  Measured in situ against the fp16 forms of the same
// build in the same session (profiles/w8_bench.json): a projection streams bytes only where its byte form is faster
// by more than the run-to-run spread of the fp16 runs.  qkv, fc1 and fc2 are at B = 1, 2 and 4; out_proj is at B = 1 (the fused merge
// launch) and 2, and is not at B = 4 (4.10 against 4.15 us, spread 0.18) - B = 3 was not measured and goes with 4.
constexpr bool w8_streams(Proj proj, int B) {
    return proj == PROJ_QKV || proj == PROJ_FC1 || proj == PROJ_FC2 || (proj == PROJ_OUT && B <= 2);
}
// The same question for the matrix-core forms (ER_FORM_MFMA, _MFMA_XT, _NARROW, _NARROW_DEFER) of a batch of B rows.  knob = ER_W8_BATCHED
// as er_create read it: 0 = the fp16 tiled copies everywhere, 1 = bytes in every matrix-core form, anything else = the measured rule.
// The rule, by the criterion above (profiles/w8_batched_bench.json, scripts/bench_w8_batched.py: fp16 and byte caches, B = 8, 16, 32;
// DESIGN.md section 4): qkv, fc1 and fc2 are faster beyond the fp16 spread in all six cases (0.65 - 1.36 us of 5.6 - 12.1); out_proj is
// not - its 0.04 - 0.31 us of 3.2 - 4.0 are inside the spread in three of the four cases it has a matrix-core form in - and keeps the fp16 copy.
// Batches other than 8, 16 and 32 were not measured: they launch the same two instantiations per form (one batch half up to 16 rows, two
// up to 32, groups of 32 above that) and go with them; B <= 4 gets here under ER_FORCE_BATCHED=1 only and keeps the fp16 copies.
constexpr bool w8_streams_batched(Proj proj, int B, int knob) {
    if (proj == PROJ_HEAD || knob == 0) return false;
    if (knob == 1) return true;
    return B > 4 && (proj == PROJ_QKV || proj == PROJ_FC1 || proj == PROJ_FC2);
}

// The copy the decode step streams for `proj` of `layer` under plan p.  row_class: the step runs a one-row plan as the kernels of 2 .. 4
// rows (KvMem::row_class), which takes the two fused launches out.  The layer picks between fc2's two narrow forms only, which read the
// same copy: the source of a projection is the same in every layer.
inline WSrc weight_source(const DecodePlan& p, const DecodeKnobs& k, WMode mode, bool row_class, Proj proj, int layer) {
    if (proj == PROJ_HEAD) return WSRC_PLAIN;      // the lm_head is not quantised and stays on the VALU kernels
    // the fused attention merge + out_proj launch of version 3: the byte block in fp8 mode (the row form's measurement at one row), never nibbles
    if (p.v3 && !row_class && proj == PROJ_OUT) return mode == W_FP8 && w8_streams(PROJ_OUT, 1) ? WSRC_BYTES : WSRC_PLAIN;
    // the fused single-row MLP reads fc1 row-major and the live rows of fc2 k-major, in the plain weight type of the mode
    if (p.mlp_fused && !row_class && (proj == PROJ_FC1 || proj == PROJ_FC2)) return proj == PROJ_FC2 ? WSRC_KMAJOR : WSRC_PLAIN;
    const int form = proj_form(p, k, mode != W_EXACT, proj, layer).form;
    if (form == ER_FORM_ROW) {
        if (mode == W_FP8 && w8_streams(proj, p.B)) return WSRC_BYTES;
        if (mode == W_FP4 && w4_streams(proj, p.B, k.w4_rows)) return WSRC_QUADS;
        return WSRC_PLAIN;
    }
    if (form_mfma(form)) {
        if (mode == W_FP8 && w8_streams_batched(proj, p.B, k.w8_batched)) return WSRC_TILED_BYTES;
        if (mode == W_FP4 && w4_streams_batched(proj, p.B, k.w4_batched)) return WSRC_TILED_NIBBLES;
        return WSRC_TILED;
    }
    return WSRC_PLAIN;      // ER_FORM_VALU and ER_FORM_ROWS8 have no packed form and read no tiled copy
}

}   // namespace er
