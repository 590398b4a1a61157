// Where do the ~11 us of the fused single-row MLP launch go?  The library's own mlp_sparse_body (k_mlp_sparse.h) compiled with
// timeline hooks: a wave's first thread stamps s_memtime (shader clock) at
//   0 entry | 1 group A's W1 loads issued | 2 group B's W1 loads issued (wave 6) | 8 group A's W1 landed, f[0..11] computed
//   3 first "f ready" barrier passed | 4 first half's rows requested | 9 group B's W1 landed, f[12..23] computed (wave 6)
//   5 second barrier passed | 6 second half's rows requested | 10 first half's rows landed and summed | 7 chain vector stored
// (wave 0 unless noted) and s_memrealtime (100 MHz, chip-wide) at entry and exit, so the launch boundary can be read too.
// In situ stand-in: a graph of 24 x (plain 28 MB weight-streaming kernel, the MLP launch over its own layer's 2 x 37.7 MB of weights),
// W1 random with zero bias, so about half of the neurons are dead.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-kernarg-preload-count=16 -I ../../edgerunner_amd/csrc \
//         -o mlp_timeline_probe mlp_timeline_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

constexpr int TPM_N = 13;                              // [0..10] s_memtime stamps, [11..12] s_memrealtime at entry / exit
extern __shared__ unsigned long long er_tpm_dyn[];
#define ER_TPM(i, w)                                                                     \
    do {                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                               \
        if (threadIdx.x == (w) * 64) {                                                   \
            er_tpm_dyn[i] = __builtin_amdgcn_s_memtime();                                \
            if ((i) == 0) er_tpm_dyn[11] = __builtin_amdgcn_s_memrealtime();             \
            if ((i) == 7) er_tpm_dyn[12] = __builtin_amdgcn_s_memrealtime();             \
        }                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                               \
    } while (0)
#include "k_mlp_sparse.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)
using namespace er;

// the library kernel's argument list (the five pointers the first loads need lead it) + where this launch's stamps go
__global__ __launch_bounds__(MLP_TPB) void mlp_timed(const void* pW1, const float* pxin, const float* pln_w, const float* pln_b, const float* pb1,
                                                     MlpArgs a_, unsigned long long* out) {
    MlpArgs a = a_;
    a.W1 = pW1; a.xin = pxin; a.ln_w = pln_w; a.ln_b = pln_b; a.b1 = pb1;
    if (threadIdx.x == (MLP_NW / 2) * 64) er_tpm_dyn[2] = er_tpm_dyn[9] = 0;      // wave 6's stamps: 0 where the form takes none
    mlp_sparse_body<float>(a);
    if (threadIdx.x == 0) {                    // group B's waves have left; their stamps were written before the last barrier
        unsigned long long* o = out + (long long)blockIdx.x * TPM_N;
        for (int i = 0; i < TPM_N; ++i) o[i] = er_tpm_dyn[i];
    }
}

typedef float f32x4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void filler_kernel(const float* __restrict__ W, const float* __restrict__ xin, float* __restrict__ yout, int N,
                                                     unsigned long long* end_rt) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wid;
    const f32x4v* wr = reinterpret_cast<const f32x4v*>(W + (long long)min(row, N - 1) * 1536);
    f32x4v w[6], x[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) w[j] = __builtin_nontemporal_load(wr + j * 64 + lane);
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = reinterpret_cast<const f32x4v*>(xin)[j * 64 + lane];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) { s = fmaf(w[j].x, x[j].x, s); s = fmaf(w[j].y, x[j].y, s); s = fmaf(w[j].z, x[j].z, s); s = fmaf(w[j].w, x[j].w, s); }
    s = wave_sum(s);
    if (lane == 0 && row < N) yout[row] = s;
    if (threadIdx.x == 0) end_rt[blockIdx.x] = __builtin_amdgcn_s_memrealtime();
}

int main() {
    const int NL = 24, NQ = 4608;
    const size_t welems = (size_t)MLP_INTER * MLP_HIDDEN;
    float *W1, *W2T, *Wf;
    CHECK(hipMalloc(&W1, welems * 4 * NL));
    CHECK(hipMalloc(&W2T, welems * 4 * NL));
    CHECK(hipMalloc(&Wf, (size_t)NQ * 1536 * 4 * NL));
    CHECK(hipMemset(Wf, 0, (size_t)NQ * 1536 * 4 * NL));
    std::vector<float> hx(MLP_HIDDEN), ones(MLP_HIDDEN, 1.f);
    {   // W1, W2T: uniform in (-0.02, 0.02), a different rotation of one host image per layer; x: uniform in (-1, 1)
        std::vector<float> hw(welems + NL);
        unsigned s = 99u;
        for (auto& v : hw) { s = s * 1664525u + 1013904223u; v = ((float)(s >> 8) / 8388608.f - 1.f) * 0.02f; }
        for (auto& v : hx) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) / 8388608.f - 1.f; }
        for (int l = 0; l < NL; ++l) {
            CHECK(hipMemcpy(W1 + l * welems, hw.data() + l, welems * 4, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(W2T + l * welems, hw.data() + (NL - l), welems * 4, hipMemcpyHostToDevice));
        }
    }
    float *x, *lnw, *lnb, *b1, *zero, *hout, *part, *xa, *xb;
    int* nnz;
    CHECK(hipMalloc(&x, MLP_HIDDEN * 4));
    CHECK(hipMalloc(&lnw, MLP_HIDDEN * 4));
    CHECK(hipMalloc(&lnb, MLP_HIDDEN * 4));
    CHECK(hipMalloc(&zero, MLP_HIDDEN * 4));
    CHECK(hipMalloc(&hout, MLP_HIDDEN * 4));
    CHECK(hipMalloc(&b1, MLP_INTER * 4));
    CHECK(hipMalloc(&part, (size_t)MLP_WGS * MLP_HIDDEN * 4));
    CHECK(hipMalloc(&nnz, (size_t)NL * MLP_WGS * 4));
    CHECK(hipMalloc(&xa, 8192 * 4));
    CHECK(hipMalloc(&xb, 8192 * 4));
    CHECK(hipMemcpy(x, hx.data(), MLP_HIDDEN * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(lnw, ones.data(), MLP_HIDDEN * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(lnb, 0, MLP_HIDDEN * 4));
    CHECK(hipMemset(zero, 0, MLP_HIDDEN * 4));
    CHECK(hipMemset(b1, 0, MLP_INTER * 4));
    CHECK(hipMemset(xa, 0, 8192 * 4));
    unsigned long long *tp, *frt;
    CHECK(hipMalloc(&tp, (size_t)NL * MLP_WGS * TPM_N * 8));
    CHECK(hipMemset(tp, 0, (size_t)NL * MLP_WGS * TPM_N * 8));
    CHECK(hipMalloc(&frt, (size_t)NL * (NQ / 4) * 8));
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    hipGraph_t graph;
    hipGraphExec_t gexec;
    CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    for (int l = 0; l < NL; ++l) {
        hipLaunchKernelGGL(filler_kernel, dim3(NQ / 4), dim3(256), 0, st, Wf + (size_t)l * NQ * 1536, xa, xb, NQ, frt + (size_t)l * (NQ / 4));
        MlpArgs a{};
        a.W1 = W1 + l * welems; a.b1 = b1; a.W2T = W2T + l * welems; a.zero_row = zero; a.xin = x; a.ln_w = lnw; a.ln_b = lnb; a.eps = 1e-5f;
        a.hout = hout; a.part = part; a.nnz = nnz + l * MLP_WGS;
        hipLaunchKernelGGL(mlp_timed, dim3(MLP_WGS), dim3(MLP_TPB), TPM_N * 8, st, a.W1, a.xin, a.ln_w, a.ln_b, a.b1, a, tp + (size_t)l * MLP_WGS * TPM_N);
    }
    CHECK(hipStreamEndCapture(st, &graph));
    CHECK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int r = 0; r < 3; ++r) CHECK(hipGraphLaunch(gexec, st));
    CHECK(hipEventRecord(e0, st));
    CHECK(hipGraphLaunch(gexec, st));
    CHECK(hipEventRecord(e1, st));
    CHECK(hipStreamSynchronize(st));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> h((size_t)NL * MLP_WGS * TPM_N), hf((size_t)NL * (NQ / 4));
    std::vector<int> hn((size_t)NL * MLP_WGS);
    CHECK(hipMemcpy(h.data(), tp, h.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hf.data(), frt, hf.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hn.data(), nnz, hn.size() * 4, hipMemcpyDeviceToHost));
    long long live = 0;
    for (int v : hn) live += v;
    printf("graph of 24 x (filler 28 MB, fused MLP) = %.1f us -> %.2f us per pair | live neurons %.1f %%\n", ms * 1e3, ms * 1e3 / NL,
           100.0 * (double)live / ((double)NL * MLP_INTER));
    // per launch: boundary (filler's last exit -> the MLP's first entry), entry skew, total (first entry -> last exit), in us (realtime = 100 MHz)
    double acc[11] = {0}, mx[11] = {0}, bnd = 0, skew = 0, tot = 0;
    int n = 0;
    for (int l = 4; l < NL; ++l) {
        unsigned long long fend = 0, smin = ~0ull, smax = 0, emax = 0;
        for (int i = 0; i < NQ / 4; ++i) fend = std::max(fend, hf[(size_t)l * (NQ / 4) + i]);
        double d[11] = {0}, dm[11] = {0};
        for (int w = 0; w < MLP_WGS; ++w) {
            const unsigned long long* t = &h[((size_t)l * MLP_WGS + w) * TPM_N];
            smin = std::min(smin, t[11]); smax = std::max(smax, t[11]); emax = std::max(emax, t[12]);
            for (int i = 1; i < 11; ++i) {
                if (t[i] == 0) continue;       // a stamp this form does not take
                const double c = (double)(long long)(t[i] - t[0]);
                d[i] += c / MLP_WGS; dm[i] = std::max(dm[i], c);
            }
        }
        for (int i = 1; i < 11; ++i) { acc[i] += d[i]; mx[i] += dm[i]; }
        bnd += (double)(long long)(smin - fend) / 100.0; skew += (double)(smax - smin) / 100.0; tot += (double)(emax - smin) / 100.0;
        ++n;
    }
    printf("boundary filler-exit -> first MLP entry %.2f us | entry skew %.2f us | first entry -> last exit %.2f us\n", bnd / n, skew / n, tot / n);
    const int order[10] = {1, 2, 8, 3, 4, 9, 5, 6, 10, 7};
    const char* names[11] = {"entry", "A: W1 issued", "B: W1 issued", "first barrier passed", "first half requested", "second barrier passed",
                             "second half requested", "stored", "A: W1 landed, f done", "B: W1 landed, f done", "first half landed"};
    printf("stamps relative to the workgroup's entry, shader-clock cycles (mean over workgroups | max; 0 = not taken by this form):\n");
    for (int k = 0; k < 10; ++k) printf("  %2d %-24s %8.0f | %8.0f\n", order[k], names[order[k]], acc[order[k]] / n, mx[order[k]] / n);
    return 0;
}
