// Which fc1 neurons a workgroup of the fused single-row MLP (k_mlp_sparse.h) owns, and in which order it feeds them to fc2's sum.
// Pure C++ with no device call (er_decode_plan.h is the precedent): the kernel includes it, and tests/host/mlp_map_check.cpp checks it
// against the index formula of gemv_kernel on the host.
//
// fc2's row kernel (gemv_kernel<WT, 4, 1, RW, PRO_NONE, EPI_RESID>) splits K = 6144 into 4 slices of 1536, one wave each; lane l of
// the wave of slice s runs ONE fmaf chain over the EPL elements of its 16-byte loads j = 0 .. J-1, i.e. over the neurons
//     k(i) = s * 1536 + (j * 64 + l) * EPL + e,   i = j * EPL + e ascending,   J * EPL = 24
// (EPL = 4 for fp32 weights, 8 for fp16).  Workgroup wg = s * 64 + l of the fused kernel owns exactly that chain: it computes the 24
// fc1 outputs f[k(i)] and then, for every output column, the chain's partial sum in the chain's own order.
#pragma once

namespace er {

constexpr int MLP_HIDDEN = 1536, MLP_INTER = 6144;      // the widths the fused kernel is built for
constexpr int MLP_SLICES = MLP_INTER / MLP_HIDDEN;      // 4 K-slices of fc2 (one wave each in the row kernel)
constexpr int MLP_WGS = MLP_SLICES * 64;                // one workgroup per (slice, lane) chain
constexpr int MLP_CHAIN = MLP_INTER / MLP_WGS;          // 24 neurons per chain

struct MlpSlot { int wg, i; };

// neuron i (0 .. 23) of workgroup wg (0 .. 255); epl = elements per 16-byte weight load (4 or 8)
constexpr int mlp_neuron(int epl, int wg, int i) {
    return (wg >> 6) * MLP_HIDDEN + ((i / epl) * 64 + (wg & 63)) * epl + i % epl;
}
// the inverse: which workgroup owns neuron k, and at which place of its chain
constexpr MlpSlot mlp_slot(int epl, int k) {
    const int s = k / MLP_HIDDEN, q = (k % MLP_HIDDEN) / epl, e = k % epl;      // 1536 % epl == 0
    return MlpSlot{s * 64 + q % 64, (q / 64) * epl + e};
}

// ---- Which fc2 rows the fused kernel requests.  The chain is cut into two halves of 12 places (waves 0-5 and 6-11 of fc1); per half
// the live places (f != 0) are bit i of a 12-bit mask, i = place - 12 * half.  The kernel requests rows by SLOT: slot u holds the u-th
// live place in ascending order, the slots behind the live ones are pads (zero row, f = 0) up to the next multiple of 4, and the slots
// behind those are not requested at all.  Running the chain over the slots leaves out only steps fmaf(+0, +0, s), in the chain's order.
constexpr int MLP_HALF = MLP_CHAIN / 2;                 // 12 places per half
constexpr int MLP_LIVE_BLOCK = 4;                       // rows are requested in blocks of 4 slots
constexpr unsigned MLP_HALF_MASK = (1u << MLP_HALF) - 1u;
constexpr int mlp_live_count(unsigned mask) { return __builtin_popcount(mask & MLP_HALF_MASK); }
// slots to request for a half: the live count rounded up to whole blocks; 0 for the empty mask
constexpr int mlp_live_slots(unsigned mask) { return (mlp_live_count(mask) + MLP_LIVE_BLOCK - 1) / MLP_LIVE_BLOCK * MLP_LIVE_BLOCK; }
// the mask behind its lowest live place (the kernel walks the slots by peeling)
constexpr unsigned mlp_live_peel(unsigned mask) { return mask & (mask - 1u); }
// the lane the next slot of a (peeled) mask reads: its lowest live place, or lane 12 for a pad - the column waves keep place i's f and
// row in lane i, and f = 0 and the zero row in the lanes from 12 on
constexpr int MLP_PAD_LANE = MLP_HALF;
constexpr int mlp_live_lane(unsigned mask) { return __builtin_ctz((mask & MLP_HALF_MASK) | (1u << MLP_PAD_LANE)); }
// the place (0 .. 11) slot u holds, or -1 for a pad
constexpr int mlp_live_place(unsigned mask, int u) {
    for (int i = 0; i < u; ++i) mask = mlp_live_peel(mask);
    return mlp_live_lane(mask) < MLP_PAD_LANE ? mlp_live_lane(mask) : -1;
}

// ---- The finish launch (mlp_finish_kernel<NC>; launched with NC = 32, the map holds for 8 and 16 as well): NC consecutive outputs per
// workgroup, wave s = slice s.  The wave reads the NC * 4 bytes of each of its 64 chain vectors as 16-byte pieces: g = NC / 4 adjacent
// lanes share one chain, so one wave-load covers 64 / g chains with g * 16 contiguous bytes each (NC = 32: eight whole 128-byte
// lines), and a lane issues g loads.
//     load j of lane l reads chain j * (64 / g) + l / g of the slice, piece l % g
// The sum over the 64 chains is wave_sum's butterfly on the CHAIN index (xor 32, 16, 8, 4, 2, 1 in that order).  The chain's high bits
// are the load index, its low bits sit in the lane's high bits, so level k (xor 32 >> k) is either an add of two of the lane's own
// registers, r[j] + r[j ^ off], or the lanes l and l ^ off meeting: mlp_fin_level says which.  Both operands of every add are the ones
// the butterfly adds at that level, hence the same bits (tests/host/mlp_finish_tree_check.cpp).
constexpr bool mlp_fin_nc_ok(int nc) { return nc == 8 || nc == 16 || nc == 32; }
constexpr int mlp_fin_group(int nc) { return nc / 4; }                           // g: lanes per chain = 16-byte pieces per chain = loads per lane
constexpr int mlp_fin_chains_per_load(int nc) { return 64 / mlp_fin_group(nc); }
constexpr int mlp_fin_chain(int nc, int load, int lane) { return load * mlp_fin_chains_per_load(nc) + lane / mlp_fin_group(nc); }
constexpr int mlp_fin_piece(int nc, int lane) { return lane % mlp_fin_group(nc); }

struct MlpFinLevel { bool reg; int off; };      // reg: r[j] + r[j ^ off] in every lane; else: lane l + lane l ^ off
constexpr int MLP_FIN_LEVELS = 6;
constexpr MlpFinLevel mlp_fin_level(int nc, int k) {      // level k = 0 .. 5 pairs the chains c and c ^ (32 >> k)
    const int x = 32 >> k, cpl = mlp_fin_chains_per_load(nc);
    return x >= cpl ? MlpFinLevel{true, x / cpl} : MlpFinLevel{false, x * mlp_fin_group(nc)};
}

}   // namespace er
