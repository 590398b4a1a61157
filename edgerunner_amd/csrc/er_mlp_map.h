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

}   // namespace er
