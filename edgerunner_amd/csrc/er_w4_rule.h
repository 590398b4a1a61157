// The launch rule of fp4 mode (er_w4.h): which decode projections stream e2m1 nibbles in their row forms.  Pure constexpr C++ with no
// device call, included by er_decode_proj.h (whose launch_proj asks it) and enumerated on the host by tests/host/w4_map_check.cpp.
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

}   // namespace er
