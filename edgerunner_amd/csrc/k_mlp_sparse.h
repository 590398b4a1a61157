// Single-row decode MLP that does not read the fc2 weights behind zero ReLU outputs (B = 1, hidden 1536, intermediate 6144).
//
//   ypre = W2 . relu(W1 . LN(x) + b1) + b2 + LN(x)
//
// Every column k of W2 whose f_k = relu(...) is exactly zero contributes fmaf(w, +0, s) = s to every sum it takes part in, yet the
// row-major GEMV (k_gemv.h) streams all of W2.  Here W2 is kept k-major (W2T[6144][1536], one contiguous row per neuron) and a row is
// fetched only when its neuron is alive.  Two launches replace fc1 + fc2:
//
//   mlp_sparse_kernel   256 workgroups of 12 waves.  Workgroup wg owns the 24 neurons of ONE lane chain of fc2's row kernel
//                       (er_mlp_map.h).  Phase 1 is fc1 for those 24 rows of W1 with gemv_kernel's arithmetic (same LayerNorm
//                       prologue, same per-lane fmaf chain, same butterfly, + b1, max 0).  Phase 2 runs, for every output column, the
//                       chain s = fmaf(W2T[k(i)][n], f_i, s), i = 0 .. 23 - the chain lane l of slice s runs in the row kernel, element
//                       for element - and stores the 1536 chain values as one partial vector.  A dead neuron's row address is replaced
//                       by a zero row (the load stays): fmaf(+0, +0, s) == s for every s but -0, which the tree's first add turns into +0
//                       either way.  FINITE weights are assumed: the row kernel would turn an Inf / NaN weight behind a zero activation
//                       into NaN, here it is never read.  The 6 KB zero row is served by the caches: the HBM counters show
//                       W1 + live rows * 6 KB per launch within 0.8 %.
//   mlp_finish_kernel   rebuilds the row kernel's tree from the 256 partial vectors: the 64 chains of a slice in wave_sum's order
//                       (read as whole 128-byte lines, 32 outputs per workgroup), the four slice sums in the order
//                       ((0 + p0) + p1) + p2) + p3, then + b2 + residual.
//
// Both results are therefore bit-identical to fc1 + fc2 of the row kernels (tests/test_gpu_mlp_sparse.py).  No inter-workgroup
// wait: the finish is a launch, every word of the partial block is rewritten by every launch.
#pragma once
#include "er_common.h"
#include "er_mlp_map.h"
#include "k_gemv.h"

namespace er {

struct MlpArgs {
    const void* W1;        // [6144][1536] in the weight type
    const float* b1;       // [6144]
    const void* W2T;       // [6144][1536]: fc2.weight transposed (transpose_w2_kernel)
    const void* zero_row;  // 1536 zeros of at least the weight type's size
    const float* xin;      // pre-LN vector [1536]
    const float* ln_w;
    const float* ln_b;
    float eps;
    float* hout;           // workgroup 0 stores LN(x) here (fc2's residual); may be null
    float* part;           // [256][1536] chain values
    int* nnz;              // [256] live neurons per workgroup; may be null
    // finish
    const float* b2;       // [1536]
    const float* resid;    // [1536]
    float* out;            // [1536]
};

// W2 [N][K] -> W2T [K][N]; N and K multiples of 64
template <typename WT>
__global__ __launch_bounds__(ER_WG) void transpose_w2_kernel(const WT* __restrict__ src, WT* __restrict__ dst, int N, int K) {
    __shared__ WT tile[64][65];
    const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) tile[r][tx] = src[(long long)(n0 + r) * K + k0 + tx];
    __syncthreads();
    for (int r = ty; r < 64; r += 4) dst[(long long)(k0 + r) * N + n0 + tx] = tile[tx][r];
}

template <typename WT>
inline hipError_t launch_transpose_w2(const void* w2, void* w2t, hipStream_t st) {
    hipLaunchKernelGGL((transpose_w2_kernel<WT>), dim3(MLP_INTER / 64, MLP_HIDDEN / 64), dim3(ER_WG), 0, st, reinterpret_cast<const WT*>(w2),
                       reinterpret_cast<WT*>(w2t), MLP_HIDDEN, MLP_INTER);
    return hipGetLastError();
}

// four consecutive columns of a W2T row: 16 bytes of fp32 or 8 bytes of fp16
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <typename WT> struct MlpCol;
template <> struct MlpCol<float> { typedef f32x4 V; };
template <> struct MlpCol<_Float16> { typedef f16x4 V; };

constexpr int MLP_NW = 12, MLP_TPB = 64 * MLP_NW;      // 12 waves x 2 rows of W1 = the 24 neurons of the workgroup
constexpr int MLP_COLS = MLP_HIDDEN / 4;               // 384 threads cover the 1536 columns, four each

// Phase 2 runs on waves 0-5, 24 row loads per thread (handing the chain from waves 0-5 to waves 6-11 half way, 12 loads per thread,
// measured equal: profiles/mlp_sparse_ab_decode.log, and was dropped).  The five pointers the first loads need lead the argument list (kernarg preload, see gemv_kernel).
template <typename WT>
__global__ __launch_bounds__(MLP_TPB) void mlp_sparse_kernel(const void* pW1, const float* pxin, const float* pln_w, const float* pln_b,
                                                             const float* pb1, MlpArgs a_) {
    MlpArgs a = a_;
    a.W1 = pW1; a.xin = pxin; a.ln_w = pln_w; a.ln_b = pln_b; a.b1 = pb1;
    constexpr int EPL = WTraits<WT>::EPL, XV = EPL / 4, K = MLP_HIDDEN, J = K / (64 * EPL), RW = 2;
    constexpr int PW = 4, PTPB = 64 * PW, PT = K / PTPB;      // the prologue runs on 4 waves with the 256-thread element map (gemv_kernel)
    static_assert(MLP_NW * RW == MLP_CHAIN && J * EPL == MLP_CHAIN, "one workgroup = one lane chain of fc2");
    typedef typename MlpCol<WT>::V ColV;
    __shared__ __attribute__((aligned(16))) float xs[K];
    __shared__ float red[64];
    __shared__ __attribute__((aligned(16))) float fs[MLP_CHAIN];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wg = blockIdx.x;
    const bool pro = wid < PW;

    // ---------------- phase 1: fc1 of the 24 rows.  Loads in the order their consumers run (gemv_kernel): prologue operands, bias,
    // then the whole weight stream
    float v[PT], lw[PT], lb[PT];
    if (pro) {
#pragma unroll
        for (int i = 0; i < PT; ++i) v[i] = a.xin[tid + i * PTPB];
#pragma unroll
        for (int i = 0; i < PT; ++i) { lw[i] = a.ln_w[tid + i * PTPB]; lb[i] = a.ln_b[tid + i * PTPB]; }
    }
    int krow[RW];
    float bias[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        krow[r] = mlp_neuron(EPL, wg, wid * RW + r);
        bias[r] = a.b1[krow[r]];
    }
    f32x4 w[RW][J];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const f32x4* wr = reinterpret_cast<const f32x4*>(reinterpret_cast<const WT*>(a.W1) + (long long)krow[r] * K);
#pragma unroll
        for (int j = 0; j < J; ++j) w[r][j] = __builtin_nontemporal_load(wr + j * 64 + lane);
    }
    __builtin_amdgcn_sched_barrier(0);

    {   // LayerNorm: gemv_kernel's PRO_LN at NB = 1, statement for statement
        float s[1], s2[1];
        s[0] = 0.f;
#pragma unroll
        for (int i = 0; i < PT; ++i) s[0] += pro ? v[i] : 0.f;
        block_sum_slots<PW, 1>(s, red, 8, pro);
        const float mean = s[0] / (float)K;
        s2[0] = 0.f;
#pragma unroll
        for (int i = 0; i < PT; ++i) { const float d = (pro ? v[i] : 0.f) - mean; s2[0] = fmaf(d, d, s2[0]); }
        block_sum_slots<PW, 1>(s2, red + 4, 8, pro);
        if (pro) {
            const float rstd = 1.0f / sqrtf(s2[0] / (float)K + a.eps);
#pragma unroll
            for (int i = 0; i < PT; ++i) v[i] = (v[i] - mean) * rstd * lw[i] + lb[i];
#pragma unroll
            for (int i = 0; i < PT; ++i) xs[tid + i * PTPB] = v[i];
            if (a.hout != nullptr && wg == 0) {
#pragma unroll
                for (int i = 0; i < PT; ++i) a.hout[tid + i * PTPB] = v[i];
            }
        }
    }
    __syncthreads();

    {
        f32x4 xr[J * XV];      // the EPL inputs matching load j are float4 #(j*64+lane)*XV .. +XV
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int u = 0; u < XV; ++u) xr[j * XV + u] = reinterpret_cast<const f32x4*>(xs)[(j * 64 + lane) * XV + u];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) s = dot_w<WT>(w[r][j], &xr[j * XV], s);
            float f = wave_sum(s);
            f += bias[r];                  // gemv_epilogue<EPI_RELU>
            f = fmaxf(f, 0.0f);
            if (lane == 0) fs[wid * RW + r] = f;
        }
    }
    __syncthreads();

    // ---------------- phase 2: the chain over the live rows of W2T
    constexpr int NCH = MLP_CHAIN;
    if (wid >= MLP_NW / 2) return;             // no barrier behind this point
    const int col = tid;                       // 0 .. 383
    float f[NCH];
    ColV wv[NCH];
#pragma unroll
    for (int u = 0; u < NCH; u += 4) {         // all f in one round of LDS reads
        const f32x4 t = reinterpret_cast<const f32x4*>(fs)[u / 4];
        f[u] = t.x; f[u + 1] = t.y; f[u + 2] = t.z; f[u + 3] = t.w;
    }
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        // f_i is the same in every lane: say so, and the address select is scalar
        f[u] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(f[u])));
        const char* row = f[u] != 0.f ? reinterpret_cast<const char*>(a.W2T) + (long long)mlp_neuron(EPL, wg, u) * K * (long long)sizeof(WT)
                                      : reinterpret_cast<const char*>(a.zero_row);
        wv[u] = __builtin_nontemporal_load(reinterpret_cast<const ColV*>(row) + col);
    }
    __builtin_amdgcn_sched_barrier(0);         // every row request is out before the first one is consumed
    if (tid == 0 && a.nnz != nullptr) {
        int c = 0;
#pragma unroll
        for (int i = 0; i < MLP_CHAIN; ++i) c += fs[i] != 0.f ? 1 : 0;
        a.nnz[wg] = c;
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
        s.x = fmaf((float)wv[u].x, f[u], s.x);
        s.y = fmaf((float)wv[u].y, f[u], s.y);
        s.z = fmaf((float)wv[u].z, f[u], s.z);
        s.w = fmaf((float)wv[u].w, f[u], s.w);
    }
    // a plain store: as a write-through (sc1) store it measured equal or slower in the decode loop (profiles/mlp_finish_bench.log)
    reinterpret_cast<f32x4*>(a.part + (long long)wg * K)[col] = s;
}

// NC consecutive outputs per workgroup, wave s = slice s.  The partial block is [chain][1536] and the fused kernel writes whole rows,
// so the finish gathers NC * 4 bytes per chain: g = NC / 4 adjacent lanes read one chain's bytes as 16-byte pieces, a wave-load
// covers 64 / g chains and a lane issues g loads (er_mlp_map.h).  At NC = 32 a wave-load is eight whole 128-byte lines and no line
// of the block is requested twice on the chip (48 workgroups); that form is the one launched.  With 32-byte pieces (NC = 8, 192
// workgroups, every line wanted by four of them) the HBM-side counters showed 6.38 MB read for the 1.57 MB block, and the decode
// loop ran 2.4 % slower; NC = 16 lay between.  The sum over the 64 chains is wave_sum's butterfly on the chain
// index: the levels that pair two loads are adds of the lane's own registers, the others xor_sum steps across lanes (mlp_fin_level),
// four outputs at a time.  Then NC threads add the four slice sums in slice order, + b2, + residual (gemv_kernel's split-K tail and
// gemv_epilogue<EPI_RESID>).
constexpr int MLP_FIN_NC = 32;
template <int NC, int K>
__device__ __forceinline__ void mlp_fin_tree_level(f32x4 (&r)[NC / 4]) {
    constexpr MlpFinLevel lv = mlp_fin_level(NC, K);
    if constexpr (lv.reg) {
#pragma unroll
        for (int j = 0; j < lv.off; ++j) r[j] = r[j] + r[j ^ lv.off];      // the loads above 2 * off are already folded in
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[0][e] = xor_sum<lv.off>(r[0][e]);
    }
}

template <int NC>
__global__ __launch_bounds__(ER_WG) void mlp_finish_kernel(MlpArgs a) {
    static_assert(mlp_fin_nc_ok(NC) && MLP_HIDDEN % NC == 0 && MLP_SLICES == ER_NWAVES && MLP_FIN_LEVELS == 6, "finish shape");
    constexpr int G = mlp_fin_group(NC);
    __shared__ __attribute__((aligned(16))) float red[MLP_SLICES * NC];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, n0 = blockIdx.x * NC;
    float bias = 0.f, resid = 0.f;
    if (tid < NC) { bias = a.b2[n0 + tid]; resid = a.resid[n0 + tid]; }
    const float* p = a.part + (long long)wid * 64 * MLP_HIDDEN + n0 + mlp_fin_piece(NC, lane) * 4;
    f32x4 r[G];
#pragma unroll
    for (int j = 0; j < G; ++j) r[j] = *reinterpret_cast<const f32x4*>(p + (long long)mlp_fin_chain(NC, j, lane) * MLP_HIDDEN);
    __builtin_amdgcn_sched_barrier(0);         // every chain request is out before the first one is consumed
    mlp_fin_tree_level<NC, 0>(r); mlp_fin_tree_level<NC, 1>(r); mlp_fin_tree_level<NC, 2>(r);
    mlp_fin_tree_level<NC, 3>(r); mlp_fin_tree_level<NC, 4>(r); mlp_fin_tree_level<NC, 5>(r);
    if (lane < G) reinterpret_cast<f32x4*>(red + wid * NC)[lane] = r[0];      // the lanes of chain 0: one per piece
    __syncthreads();
    if (tid < NC) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MLP_SLICES; ++k) s += red[k * NC + tid];
        s += bias;
        s += resid;
        a.out[n0 + tid] = s;
    }
}

// the two launches of one layer's MLP
template <typename WT>
inline hipError_t launch_mlp_fused(const MlpArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((mlp_sparse_kernel<WT>), dim3(MLP_WGS), dim3(MLP_TPB), 0, st, a.W1, a.xin, a.ln_w, a.ln_b, a.b1, a);
    return hipGetLastError();
}
inline hipError_t launch_mlp_finish(const MlpArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(mlp_finish_kernel<MLP_FIN_NC>, dim3(MLP_HIDDEN / MLP_FIN_NC), dim3(ER_WG), 0, st, a);
    return hipGetLastError();
}

}   // namespace er
