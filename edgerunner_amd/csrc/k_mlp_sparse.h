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
//                       for element - and stores the 1536 chain values as one partial vector.  The steps of dead neurons are LEFT OUT:
//                       per half-chain of 12 places only the live rows are requested, in chain order, padded with the zero row and
//                       f = +0 to whole blocks of four (er_mlp_map.h).  A left-out step fmaf(w, +0, s) with a finite w returns s for
//                       every s but a zero and a zero for a zero, so a chain value can differ from the row kernel's only in the SIGN
//                       OF A ZERO; the finish tree adds chain values pairwise and starts its last stage from +0, a zero of either
//                       sign leaves a non-zero partner unchanged, gives a zero with a zero, and +0 + (+-0) = +0, so no bit of the
//                       output depends on it (tests/host/mlp_live_check.cpp walks all 4096 masks of a half).  FINITE weights are
//                       assumed: the row kernel would turn an Inf / NaN weight behind a zero activation into NaN, here it is never
//                       read.  The 6 KB zero row is served by the caches: the HBM counters show W1 + live rows * 6 KB per launch
//                       within 0.8 %.
//                       The two phases overlap: waves 0-5 (group A, places 0-11) request their W1 rows at entry; waves 6-11 (group B,
//                       places 12-23) first request the LayerNorm prologue's operands, which they run, and then their W1 rows, so the
//                       CU's address unit takes A's 72 kilobyte-requests before B's.  When A's rows are in, A computes f[0..11] and,
//                       behind a workgroup barrier, requests the live rows of its places while B's half of W1 is still arriving; B's
//                       f[12..23] and rows follow behind a second barrier, and the chain runs over both halves in chain order.  In
//                       the parent form every W1 byte landed on the chip before the first W2T request went out, and 24 requests per
//                       thread (half of them for the zero row) stood between "f known" and "last live row requested"
//                       (profiles/mlp_stagger_timeline.log).
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

// Timeline hooks: ER_TPM(i, w) stamps the clock into slot i on the first thread of wave w (scripts/probes/mlp_timeline_probe.hip
// defines them); nothing in the library build.
#ifndef ER_TPM
#define ER_TPM(i, w)
#endif

// lane i < 12 of a column wave: where the W2T row of place i of a half starts, in bytes from W2T (known at entry)
template <typename WT>
__device__ __forceinline__ long long mlp_lane_row(int half, int wg, int lane) {
    return (long long)mlp_neuron(WTraits<WT>::EPL, wg, half * MLP_HALF + (lane < MLP_HALF ? lane : 0)) * MLP_HIDDEN * (long long)sizeof(WT);
}

// One half of phase 2's requests on the column threads: the live mask of the half's 12 places from fs, the slots (er_mlp_map.h), the
// loads.  f is workgroup-uniform, so lane i keeps place i: its f (0 in the lanes from 12 on) and where its row starts, counted from
// W2T (lrow; the zero row's distance for a dead place and in the lanes from 12 on).  The mask is a ballot; slot u reads the lane of
// its place, a pad reads lane 12, so the slot walk is a find-first-bit and three readlanes per slot.  Only nb = slots / 4 blocks of
// four rows are requested; the condition stands around a BLOCK of loads whose registers nothing else writes (a condition around a
// single load makes hipcc branch and wait: k_attn_decode.h), and mlp_half_chain runs the steps of the same blocks only.  Returns the
// mask.
template <typename WT>
__device__ __forceinline__ unsigned mlp_half_request(const MlpArgs& a, const float* fs, int half, long long lrow, int lane, int col,
                                                     float (&f)[MLP_HALF], typename MlpCol<WT>::V (&wv)[MLP_HALF], int& nb) {
    typedef typename MlpCol<WT>::V ColV;
    float fl = fs[half * MLP_HALF + (lane < MLP_HALF ? lane : 0)];
    fl = lane < MLP_HALF ? fl : 0.f;
    const unsigned mask = (unsigned)__builtin_amdgcn_ballot_w64(fl != 0.f);
    const char* w2t = reinterpret_cast<const char*>(a.W2T);
    const long long lr = fl != 0.f ? lrow : (long long)(reinterpret_cast<unsigned long long>(a.zero_row) - reinterpret_cast<unsigned long long>(a.W2T));
    const unsigned lr_lo = (unsigned)lr, lr_hi = (unsigned)((unsigned long long)lr >> 32);
    const char* row[MLP_HALF];
    unsigned m = mask;
#pragma unroll
    for (int u = 0; u < MLP_HALF; ++u) {
        const int p = mlp_live_lane(m);        // mlp_live_place(mask, u) walked by peeling; lane 12 = a pad
        m = mlp_live_peel(m);
        f[u] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(fl), p));
        row[u] = w2t + (long long)((unsigned long long)(unsigned)__builtin_amdgcn_readlane(lr_lo, p) |
                                   ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(lr_hi, p) << 32));
    }
    nb = mlp_live_slots(mask) / MLP_LIVE_BLOCK;      // workgroup-uniform
#pragma unroll
    for (int b = 0; b < MLP_HALF / MLP_LIVE_BLOCK; ++b) {
        if (b < nb) {
#pragma unroll
            for (int u = b * MLP_LIVE_BLOCK; u < (b + 1) * MLP_LIVE_BLOCK; ++u)
                wv[u] = __builtin_nontemporal_load(reinterpret_cast<const ColV*>(row[u]) + col);
        }
    }
    __builtin_amdgcn_sched_barrier(0);         // every row request of the half is out
    return mask;
}

// the chain steps of a half's requested blocks, in slot order
template <typename WT>
__device__ __forceinline__ void mlp_half_chain(f32x4& s, const typename MlpCol<WT>::V (&wv)[MLP_HALF], const float (&f)[MLP_HALF], int nb) {
#pragma unroll
    for (int b = 0; b < MLP_HALF / MLP_LIVE_BLOCK; ++b) {
        if (b < nb) {
#pragma unroll
            for (int u = b * MLP_LIVE_BLOCK; u < (b + 1) * MLP_LIVE_BLOCK; ++u) {
                s.x = fmaf((float)wv[u].x, f[u], s.x);
                s.y = fmaf((float)wv[u].y, f[u], s.y);
                s.z = fmaf((float)wv[u].z, f[u], s.z);
                s.w = fmaf((float)wv[u].w, f[u], s.w);
            }
        }
    }
}

// The kernel's body (the timeline probe wraps it in a kernel of its own).
template <typename WT>
__device__ __forceinline__ void mlp_sparse_body(const MlpArgs& a) {
    constexpr int EPL = WTraits<WT>::EPL, XV = EPL / 4, K = MLP_HIDDEN, J = K / (64 * EPL), RW = 2;
    constexpr int PW = 4, PTPB = 64 * PW, PT = K / PTPB;      // the prologue runs on 4 waves with the 256-thread element map (gemv_kernel)
    constexpr int GW = MLP_NW / 2;                            // waves per group: A = waves 0-5 (places 0-11), B = waves 6-11 (places 12-23)
    static_assert(MLP_NW * RW == MLP_CHAIN && J * EPL == MLP_CHAIN && GW * RW == MLP_HALF && GW * 64 == MLP_COLS && PW <= GW, "one workgroup = one lane chain of fc2");
    typedef typename MlpCol<WT>::V ColV;
    __shared__ __attribute__((aligned(16))) float xs[K];
    __shared__ float red[8];
    __shared__ __attribute__((aligned(16))) float fs[MLP_CHAIN];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wg = blockIdx.x;
    const bool grpB = __builtin_amdgcn_readfirstlane(wid) >= GW;      // scalar: the groups branch, they are not masked
    const bool pro = wid >= GW && wid < GW + PW;                      // the prologue runs on group B's first four waves
    const int ptid = tid - GW * 64;
    ER_TPM(0, 0);

    // ---------------- phase 1: fc1 of the 24 rows.  Loads in the order their consumers run (gemv_kernel): prologue operands, bias,
    // then the weight stream.  Group A's waves have nothing in front of their stream; group B's request theirs behind the prologue's
    // operands, and the CU's address unit takes the workgroup's 144 one-kilobyte requests in that order, A's 72 first
    float v[PT], lw[PT], lb[PT];
    if (pro) {
#pragma unroll
        for (int i = 0; i < PT; ++i) v[i] = a.xin[ptid + i * PTPB];
#pragma unroll
        for (int i = 0; i < PT; ++i) { lw[i] = a.ln_w[ptid + i * PTPB]; lb[i] = a.ln_b[ptid + i * PTPB]; }
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
    const long long lrow0 = mlp_lane_row<WT>(0, wg, lane), lrow1 = mlp_lane_row<WT>(1, wg, lane);      // for phase 2, off its critical path
    ER_TPM(1, 0);
    ER_TPM(2, GW);
    const auto fc1_rows = [&]() {              // f of this wave's two rows: gemv_kernel's chain, butterfly and gemv_epilogue<EPI_RELU>
        f32x4 xr[J * XV];                      // the EPL inputs matching load j are float4 #(j*64+lane)*XV .. +XV
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
            f += bias[r];
            f = fmaxf(f, 0.0f);
            if (lane == 0) fs[wid * RW + r] = f;
        }
    };

    {   // LayerNorm: gemv_kernel's PRO_LN at NB = 1 on the prologue's four waves, block_sum_slots' sums restated for their wave numbers
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < PT; ++i) s += pro ? v[i] : 0.f;
        s = wave_sum(s);
        if (pro && lane == 0) red[wid - GW] = s;
        __syncthreads();
        s = (red[0] + red[1]) + (red[2] + red[3]);
        const float mean = s / (float)K;
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < PT; ++i) { const float d = (pro ? v[i] : 0.f) - mean; s2 = fmaf(d, d, s2); }
        s2 = wave_sum(s2);
        if (pro && lane == 0) red[4 + wid - GW] = s2;
        __syncthreads();
        if (pro) {
            s2 = (red[4] + red[5]) + (red[6] + red[7]);
            const float rstd = 1.0f / sqrtf(s2 / (float)K + a.eps);
#pragma unroll
            for (int i = 0; i < PT; ++i) v[i] = (v[i] - mean) * rstd * lw[i] + lb[i];
#pragma unroll
            for (int i = 0; i < PT; ++i) xs[ptid + i * PTPB] = v[i];
            if (a.hout != nullptr && wg == 0) {
#pragma unroll
                for (int i = 0; i < PT; ++i) a.hout[ptid + i * PTPB] = v[i];
            }
        }
    }
    __syncthreads();

    // ---------------- phase 2: the chain over the live rows of W2T, on the column threads (group A's waves, four columns each).  Group
    // A's f and the requests for its places' rows first, while group B's half of W1 is still arriving; then group B's.  Every wave
    // passes the same two barriers, but the two groups reach them in straight-line code of their own (a scalar branch on the wave
    // number).  With the barriers in common code and the groups' work under conditions between them, hipcc counts its waits along
    // paths no wave takes - a column wave "with W1 still pending" - and put s_waitcnt vmcnt(0) in front of the second half's
    // requests, which waits for the first half's rows.  As written the saved assembly has bare s_barriers on both paths and no
    // vmcnt wait between the first row request and the first chain step.
    if (grpB) {
        __syncthreads();                       // f[0..11] ready; this group's stream stays in flight across it
        fc1_rows();
        ER_TPM(9, GW);
        __syncthreads();                       // f[12..23] ready
        return;
    }
    const int col = tid;                       // 0 .. 383 on the column threads
    float f0[MLP_HALF], f1[MLP_HALF];
    ColV wv0[MLP_HALF], wv1[MLP_HALF];
    int nb0, nb1;
    fc1_rows();
    ER_TPM(8, 0);
    __syncthreads();                           // f[0..11] ready
    ER_TPM(3, 0);
    const unsigned m0 = mlp_half_request<WT>(a, fs, 0, lrow0, lane, col, f0, wv0, nb0);
    ER_TPM(4, 0);
    __syncthreads();                           // f[12..23] ready; the first half's rows stay in flight across it.  No barrier behind this point
    ER_TPM(5, 0);
    const unsigned m1 = mlp_half_request<WT>(a, fs, 1, lrow1, lane, col, f1, wv1, nb1);
    ER_TPM(6, 0);
    if (tid == 0 && a.nnz != nullptr) a.nnz[wg] = mlp_live_count(m0) + mlp_live_count(m1);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    mlp_half_chain<WT>(s, wv0, f0, nb0);
    ER_TPM(10, 0);                             // the first half's rows have landed
    mlp_half_chain<WT>(s, wv1, f1, nb1);
    // a plain store: as a write-through (sc1) store it measured equal or slower in the decode loop (profiles/mlp_finish_bench.log)
    reinterpret_cast<f32x4*>(a.part + (long long)wg * K)[col] = s;
    ER_TPM(7, 0);
}

// The five pointers the first loads need lead the argument list (kernarg preload, see gemv_kernel).
template <typename WT>
__global__ __launch_bounds__(MLP_TPB) void mlp_sparse_kernel(const void* pW1, const float* pxin, const float* pln_w, const float* pln_b,
                                                             const float* pb1, MlpArgs a_) {
    MlpArgs a = a_;
    a.W1 = pW1; a.xin = pxin; a.ln_w = pln_w; a.ln_b = pln_b; a.b1 = pb1;
    mlp_sparse_body<WT>(a);
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
