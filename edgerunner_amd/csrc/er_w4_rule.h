// The launch rules of fp4 mode (er_w4.h): which decode projections stream e2m1 nibbles in their row forms (w4_streams) and in their
// matrix-core batched forms (w4_streams_batched).  Pure constexpr C++ with no device call, included by er_weight_source.h (whose weight_source
// alone asks it) and enumerated on the host by tests/host/w4_map_check.cpp and tests/host/w4_tile_check.cpp.
#pragma once
#include "er_decode_plan.h"

namespace er {

// the projections that have a nibble row form: the three wide ones.  out_proj (the fused merge launch included) and the lm_head run
// the fp16 copy
constexpr bool w4_has_row_form(Proj proj) { return proj == PROJ_QKV || proj == PROJ_FC1 || proj == PROJ_FC2; }
// Which projections of an fp4 context stream nibbles in their row forms at B rows.  knob = ER_W4_ROWS as er_create read it: 0 = the fp16
// copies everywhere, 1 = nibbles in every row form that has one, anything else = the measured rule - a projection streams nibbles at B
// rows only where its nibble form measured faster than the fp16 form of the same build, in the same session, by more than the fp16
// runs' spread (profiles/w4_bench.json).  Measured at B = 1, 2, 3 and 4: fc1 (1.47 - 1.76 us of 5.1 - 8.8) and fc2
// (1.58 - 2.32 us of 5.3 - 8.3) are in all four; qkv is at B = 1 only (0.45 us of 4.81) - at B = 2 its nibble form ties the fp16 form and
// at B = 3 and 4 it is 0.6 - 1.1 us SLOWER (4 rows x NB epilogue operand sets per wave: 242 VGPRs at NB = 4).
constexpr bool w4_streams(Proj proj, int B, int knob = -1) {
    if (!w4_has_row_form(proj) || B < 1 || B > 4 || knob == 0) return false;
    if (knob == 1) return true;
    return proj == PROJ_FC1 || proj == PROJ_FC2 || (proj == PROJ_QKV && B == 1);
}

// The same question for the matrix-core forms (ER_FORM_MFMA, _MFMA_XT, _NARROW, _NARROW_DEFER) of a batch of B rows, which stream the
// tiled nibble copy of er_w4_tile_map.h.  knob = ER_W4_BATCHED as er_create read it: 0 = the fp16 tiled copies everywhere, 1 = nibbles in
// every matrix-core form of qkv, out_proj, fc1 and fc2, anything else = the measured rule, by the criterion above.  The lm_head and B <= 4
// (which gets a batched plan under ER_FORCE_BATCHED=1 only) are never included, whatever the knob.
// Measured (profiles/w4_batched_bench.json, scripts/bench_w4_batched.py: 24 layers, fp4 contexts under ER_W4_BATCHED=0 and =1 alternated
// with a fast-mode and an fp8 context in one process, fp16 and byte caches, B = 8, 16, 32; us per launch, fp16 form -> nibble form):
//     qkv       9.41 - 12.36 -> 8.20 - 10.92    1.12 - 1.44 us faster, fp16 spread 0.02 - 0.04: in all six cases
//     fc1       8.63 - 11.19 -> 7.27 -  9.68    1.35 - 1.88 us faster, spread 0.01 - 0.31:     in all six cases
//     fc2       5.64 -  7.83 -> 4.09 -  6.19    1.55 - 1.96 us faster, spread 0.01 - 0.03:     in all six cases
//     out_proj  3.30 -  3.84 -> 3.02 -  3.67    0.17 - 0.36 us faster, spread 0.05 - 0.20:     in the four cases (B = 16, 32) in which it
//               has a matrix-core form - at B = 8 it is the eight-row VALU pass on the fp16 copy in both contexts (weight_source says plain)
// So the rule is all four projections at every B > 4, the same set as ER_W4_BATCHED=1.  The fp8 forms of the same session: qkv 8.59 - 11.18,
// fc1 7.67 - 10.10, fc2 4.50 - 6.54, out_proj (fp16 copy under fp8 mode's rule) 3.23 - 4.41 - the nibble forms are 0.2 - 0.8 us below them.
// Batches other than 8, 16 and 32 were not measured: they launch the same two instantiations per form (one batch half up to 16 rows, two
// up to 32, groups of 32 above that) and go with them.
constexpr bool w4_streams_batched(Proj proj, int B, int knob) {
    if (proj == PROJ_HEAD || B <= 4 || knob == 0) return false;
    if (knob == 1) return true;
    return proj == PROJ_QKV || proj == PROJ_OUT || proj == PROJ_FC1 || proj == PROJ_FC2;
}

}   // namespace er
