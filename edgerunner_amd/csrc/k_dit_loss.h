// Eval-mode loss of MDiT.forward (core/models_dit.py:137-177): the noised latent that enters the DiT, then the min-SNR-weighted
// MSE of its prediction against the v-prediction (or epsilon) target.  Streaming kernels around the DiT forward; the per-sample
// coefficients sa = sqrt(alphas_cumprod[t]), sb = sqrt(1 - alphas_cumprod[t]) and the loss weight w come from the host (er_dit.h).
// fp contraction is off in all three: x_t and the target round exactly as the reference's separate torch ops do, so a caller can
// rebuild x_t bit for bit.
#pragma once
#include <cfloat>
#include "er_common.h"

namespace er {

enum { DIT_PRED_V = 0, DIT_PRED_EPS = 1 };       // ER_PRED_V_PREDICTION / ER_PRED_EPSILON
constexpr int DIT_LOSS_SLICE = 4096;              // elements of one sample per workgroup of dit_loss_partial_kernel (16 per thread)

__device__ __forceinline__ float nan_to_num_f(float v) {     // torch.nan_to_num(v, 0): NaN -> 0, +-inf -> +-FLT_MAX (models_dit.py:143)
    if (__builtin_isnan(v)) return 0.f;
    if (__builtin_isinf(v)) return v > 0.f ? FLT_MAX : -FLT_MAX;
    return v;
}

// x_t = sa[b] * nan_to_num(x0) + sb[b] * eps       (DDPMScheduler.add_noise, models_dit.py:148); n4 = float4 per sample
__global__ __launch_bounds__(ER_WG) void dit_add_noise_kernel(const f32x4* x0, const f32x4* eps, f32x4* xt, const float* sa,
                                                              const float* sb, long long n4, int B) {
#pragma clang fp contract(off)
    const long long total = n4 * B;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / n4);
        const float a = sa[b], s = sb[b];
        const f32x4 x = x0[i], e = eps[i];
        f32x4 o;
        o.x = a * nan_to_num_f(x.x) + s * e.x;
        o.y = a * nan_to_num_f(x.y) + s * e.y;
        o.z = a * nan_to_num_f(x.z) + s * e.z;
        o.w = a * nan_to_num_f(x.w) + s * e.w;
        xt[i] = o;
    }
}

// grid (chunks, B): workgroup (c, b) sums (pred - target)^2 over elements [c * SLICE, (c + 1) * SLICE) of sample b (n per sample,
// n % 4 == 0), in double and in a fixed order (per-thread strided sums, then a fixed LDS tree) -> partial[b * chunks + c].
// target = sa * eps - sb * nan_to_num(x0) (DDPMScheduler.get_velocity, PRED = DIT_PRED_V) or eps (DIT_PRED_EPS: x0 is not read)
template <int PRED>
__global__ __launch_bounds__(ER_WG) void dit_loss_partial_kernel(const float* pred, const float* x0, const float* eps, const float* sa,
                                                                 const float* sb, long long n, double* partial) {
#pragma clang fp contract(off)
    __shared__ double red[ER_WG];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long base = (long long)b * n, lo = (long long)blockIdx.x * DIT_LOSS_SLICE;
    const long long hi = lo + DIT_LOSS_SLICE < n ? lo + DIT_LOSS_SLICE : n;
    const float a = sa[b], s = sb[b];
    double acc = 0.0;
    for (long long i = lo + 4 * tid; i < hi; i += 4 * ER_WG) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(pred + base + i);
        const f32x4 e = *reinterpret_cast<const f32x4*>(eps + base + i);
        f32x4 t = e;
        if (PRED == DIT_PRED_V) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x0 + base + i);
            t.x = a * e.x - s * nan_to_num_f(x.x);
            t.y = a * e.y - s * nan_to_num_f(x.y);
            t.z = a * e.z - s * nan_to_num_f(x.z);
            t.w = a * e.w - s * nan_to_num_f(x.w);
        }
        const double d0 = (double)(p.x - t.x), d1 = (double)(p.y - t.y), d2 = (double)(p.z - t.z), d3 = (double)(p.w - t.w);
        acc = fma(d0, d0, acc);
        acc = fma(d1, d1, acc);
        acc = fma(d2, d2, acc);
        acc = fma(d3, d3, acc);
    }
    red[tid] = acc;
    __syncthreads();
    for (int off = ER_WG / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) partial[(long long)b * gridDim.x + blockIdx.x] = red[0];
}

// One workgroup, fixed order: mse[b] = (sum of the chunks of b, in chunk order) / n; loss[0] = mean_b(w[b] * mse[b]) (thread t owns
// samples t, t + 256, ...; then a fixed LDS tree; all in double).  No atomics: bitwise the same from run to run.
__global__ __launch_bounds__(ER_WG) void dit_loss_reduce_kernel(const double* partial, int chunks, int B, long long n, const float* w,
                                                                float* mse, float* loss) {
    __shared__ double red[ER_WG];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int b = tid; b < B; b += ER_WG) {
        double s = 0.0;
        for (int c = 0; c < chunks; ++c) s += partial[(long long)b * chunks + c];
        const double m = s / (double)n;
        mse[b] = (float)m;
        acc = fma((double)w[b], m, acc);
    }
    red[tid] = acc;
    __syncthreads();
    for (int off = ER_WG / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) loss[0] = (float)(red[0] / (double)B);
}

inline int dit_loss_chunks(long long n) { return (int)((n + DIT_LOSS_SLICE - 1) / DIT_LOSS_SLICE); }

inline hipError_t launch_dit_add_noise(const float* x0, const float* eps, float* xt, const float* sa, const float* sb, int B, long long n,
                                       hipStream_t st) {
    if (B <= 0 || n <= 0 || n % 4) return hipErrorInvalidValue;
    const long long n4 = n / 4, total = n4 * B;
    const unsigned grid = (unsigned)std::min<long long>((total + ER_WG - 1) / ER_WG, 4096);
    hipLaunchKernelGGL(dit_add_noise_kernel, dim3(grid), dim3(ER_WG), 0, st, reinterpret_cast<const f32x4*>(x0),
                       reinterpret_cast<const f32x4*>(eps), reinterpret_cast<f32x4*>(xt), sa, sb, n4, B);
    return hipGetLastError();
}

// partial: B * dit_loss_chunks(n) doubles of scratch
inline hipError_t launch_dit_loss(const float* pred, const float* x0, const float* eps, const float* sa, const float* sb, const float* w,
                                  int B, long long n, int pred_type, double* partial, float* mse, float* loss, hipStream_t st) {
    if (B <= 0 || B > 65535 || n <= 0 || n % 4 || (pred_type != DIT_PRED_V && pred_type != DIT_PRED_EPS)) return hipErrorInvalidValue;
    const int chunks = dit_loss_chunks(n);
    if (pred_type == DIT_PRED_V)
        hipLaunchKernelGGL(dit_loss_partial_kernel<DIT_PRED_V>, dim3(chunks, B), dim3(ER_WG), 0, st, pred, x0, eps, sa, sb, n, partial);
    else
        hipLaunchKernelGGL(dit_loss_partial_kernel<DIT_PRED_EPS>, dim3(chunks, B), dim3(ER_WG), 0, st, pred, x0, eps, sa, sb, n, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dit_loss_reduce_kernel, dim3(1), dim3(ER_WG), 0, st, partial, chunks, B, n, w, mse, loss);
    return hipGetLastError();
}

}  // namespace er
