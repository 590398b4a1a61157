// Scoring head of er_score (LMM.forward in eval mode, core/models.py:147-202 -> ShapeOPT.forward with labels,
// core/transformer/modeling_opt.py:497-510): per-position log-softmax NLL of the shifted target and argmax, then a
// deterministic reduction of the loss.  The logits come from the prefill GEMMs; these two kernels only read them.
#pragma once
#include "er_common.h"
#include "k_head.h"

namespace er {

constexpr int ER_IGNORE_INDEX = -100;     // F.cross_entropy's default ignore_index (the reference's collate_fn pads labels with it)
constexpr int SCORE_MAXPL = (ER_HEAD_MAX_VOCAB + 63) / 64;   // logits per lane: the whole row lives in registers

// target of position r = b * S + s: labels[b, s + 1] (the shift of modeling_opt.py:502-503); the last position has none
__device__ __forceinline__ int score_target(const int* labels, int r, int S) {
    return r % S + 1 < S ? labels[r + 1] : ER_IGNORE_INDEX;
}

// One wave per row of logits[rows][V] (V <= ER_HEAD_MAX_VOCAB), one read of the row:
//   nll[r]  = -log_softmax(logits[r])[target]   (0 where the target is ignored; NaN for a target outside [0, V), which F.cross_entropy
//             would reject - the mean then comes out NaN instead of silently dropping the position)
//   pred[r] = argmax(logits[r]), lowest index on ties (torch.argmax); pred may be null
// max / sum / arg-min through the cross-lane butterflies of er_common.h, no LDS.
__global__ __launch_bounds__(ER_WG) void score_rows_kernel(const float* logits, const int* labels, int rows, int S, int V, float* nll,
                                                           int* pred) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * ER_NWAVES + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* x = logits + (long long)r * V;
    float v[SCORE_MAXPL];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < SCORE_MAXPL; ++i) {
        const int col = lane + 64 * i;
        v[i] = col < V ? x[col] : -INFINITY;
        m = fmaxf(m, v[i]);
    }
    m = wave_max(m);
    float s = 0.f, first = 3.0e38f;          // lowest column holding the maximum (exact in float: V < 2^24)
#pragma unroll
    for (int i = 0; i < SCORE_MAXPL; ++i) {
        const int col = lane + 64 * i;
        if (col < V) {
            s += expf(v[i] - m);
            if (v[i] == m) first = fminf(first, (float)col);
        }
    }
    s = wave_sum(s);
    first = -wave_max(-first);
    if (lane != 0) return;
    const int t = score_target(labels, r, S);
    float out = 0.f;
    if (t != ER_IGNORE_INDEX) out = (t >= 0 && t < V) ? logf(s) - (x[t] - m) : NAN;     // -((x_t - m) - log s), log_softmax's order
    nll[r] = out;
    if (pred) pred[r] = (int)first;
}

inline hipError_t launch_score_rows(const float* logits, const int* labels, int rows, int S, int V, float* nll, int* pred,
                                    hipStream_t st) {
    if (rows <= 0 || S <= 0 || V <= 0 || V > ER_HEAD_MAX_VOCAB) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_rows_kernel, dim3((rows + ER_NWAVES - 1) / ER_NWAVES), dim3(ER_WG), 0, st, logits, labels, rows, S, V, nll,
                       pred);
    return hipGetLastError();
}

// One workgroup, fixed order (thread t owns elements t, t + 256, ...; then a fixed LDS tree), accumulation in double:
//   labels != null: out[0] = mean of x over the supervised positions (NaN if there are none, like F.cross_entropy), out[1] = their count
//   labels == null: out[0] = 0.5 * sum(x^2)   (DummyLatent.kl, core/transformer/point.py:32-34)
__global__ __launch_bounds__(ER_WG) void score_reduce_kernel(const float* x, const int* labels, int n, int S, float* out) {
    __shared__ double ssum[ER_WG];
    __shared__ long long scnt[ER_WG];
    const int tid = threadIdx.x;
    double acc = 0.0;
    long long cnt = 0;
    for (int i = tid; i < n; i += ER_WG) {
        if (labels) {
            if (score_target(labels, i, S) != ER_IGNORE_INDEX) { acc += (double)x[i]; ++cnt; }
        } else {
            const double d = (double)x[i];
            acc = fma(d, d, acc);
        }
    }
    ssum[tid] = acc;
    scnt[tid] = cnt;
    __syncthreads();
    for (int off = ER_WG / 2; off > 0; off >>= 1) {
        if (tid < off) { ssum[tid] += ssum[tid + off]; scnt[tid] += scnt[tid + off]; }
        __syncthreads();
    }
    if (tid != 0) return;
    if (labels) {
        out[0] = scnt[0] > 0 ? (float)(ssum[0] / (double)scnt[0]) : NAN;
        out[1] = (float)scnt[0];
    } else {
        out[0] = (float)(0.5 * ssum[0]);
    }
}

inline hipError_t launch_score_reduce(const float* x, const int* labels, int n, int S, float* out, hipStream_t st) {
    if (n <= 0 || (labels && S <= 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_reduce_kernel, dim3(1), dim3(ER_WG), 0, st, x, labels, n, S, out);
    return hipGetLastError();
}

}  // namespace er
