// The QUAD lane mapping of the byte KV cache (kv8 mode: one e4m3fn byte per element, head_dim 96), as index arithmetic only: which 16
// bytes of which key row a (load, lane) slot holds, which slots make up a key's score, and how the fold brings the four slots of an
// output piece together.  Pure constexpr C++ with no device call (er_gemm_map.h / er_mlp_map.h are the precedents): KMap<kv8_t, 96>
// in k_attn_lanes.h is written over these functions and tests/host/kv8_map_check.cpp enumerates them on the host.
//
// A byte row of D = 96 is 96 bytes, three quarters of a 128-byte line; four consecutive rows from a key that is a multiple of 4 are 384
// bytes = three whole lines (a head's base is line-aligned: the reserved Lcap is a multiple of 32).  8 lanes x 3 loads of 16 bytes take
// such a quad: slot t = 8 j + p (load j, lane p of the group) holds piece t % 6 (elements 16 (t % 6) .. + 15) of row t / 6, which in a
// quad of consecutive rows is simply byte 16 t - lane p of load j reads the p-th 16 bytes of line j, and no load straddles a row.
//     load 0: p < 6 ? row 0 piece p     : row 1 piece p - 6
//     load 1: p < 4 ? row 1 piece 2 + p : row 2 piece p - 4
//     load 2: p < 2 ? row 2 piece 4 + p : row 3 piece p - 2
#pragma once

namespace er {
namespace kv8 {

constexpr int D = 96;          // elements (= bytes) per key row
constexpr int ROWS = 4;        // key rows per quad: NK of the mapping
constexpr int GL = 8;          // lanes per quad
constexpr int NV = 3;          // 16-byte loads per lane and cache
constexpr int EPL = 16;        // elements per load
constexpr int PIECES = D / EPL;          // 6 pieces of 16 elements per row
constexpr int SLOTS = GL * NV;           // 24 = ROWS * PIECES
constexpr int KPW = 64 / GL * ROWS;      // 32 keys per wave-step

constexpr int slot(int j, int p) { return GL * j + p; }
constexpr int slot_row(int t) { return t / PIECES; }
constexpr int slot_piece(int t) { return t % PIECES; }
// load j holds row j in its lanes p < load_split(j) and row j + 1 in the others
constexpr int load_split(int j) { return PIECES - 2 * j; }
constexpr int load_row(int j, int p) { return p < load_split(j) ? j : j + 1; }
constexpr int load_piece(int j, int p) { return slot_piece(slot(j, p)); }
// byte offset of slot (j, p) from the first byte of row `row` (the slot's own row: a masked key names another row it may read)
constexpr int load_byte_in_row(int j, int p) { return load_piece(j, p) * EPL; }

// The score of row r is the sum, over the 8 lanes of the group, of the dot products of the slots that hold row r: load r - 1 (its upper
// lanes) and load r (its lower lanes).
constexpr bool score_takes(int r, int j, int p) { return load_row(j, p) == r; }
constexpr bool score_load(int r, int j) { return j == r - 1 || j == r; }      // the only loads that can hold row r

// The fold.  Every piece c sits in four slots, one per row, in lanes c, c + 6, c + 4, c + 2 (mod 8): lane c < 6 ends up with piece c as
//     o[0] (its own)  +  from lane c + 2: o[2]  +  from lane c + 4: (p >= 4 ? o[1] : o[2])  +  from lane c + 6: (p >= 6 ? o[0] : o[1])
// with p the SENDING lane.  fold_shift(i) is the distance of term i's sender above the receiver, fold_load(i, p) the accumulator it sends.
constexpr int FOLD_TERMS = 4;
constexpr int fold_shift(int i) { return 2 * i; }
constexpr int fold_load(int i, int p) { return i == 0 ? 0 : i == 1 ? 2 : i == 2 ? (p >= 4 ? 1 : 2) : (p >= 6 ? 0 : 1); }
// a term's accumulator takes at most two values over the lanes: the lowest lane's and the highest lane's (the kernel selects between them)
constexpr bool fold_load_two_valued(int i) {
    for (int p = 0; p < GL; ++p)
        if (fold_load(i, p) != fold_load(i, 0) && fold_load(i, p) != fold_load(i, GL - 1)) return false;
    return true;
}
// Of a row of 16 lanes the first group (lanes < GL) stores, and of it the lanes that hold a piece: lane p stores piece p.
constexpr bool fold_stores(int lane16) { return lane16 < GL && (lane16 & (GL - 1)) < PIECES; }
constexpr int store_piece(int p) { return p; }

}   // namespace kv8
}   // namespace er
