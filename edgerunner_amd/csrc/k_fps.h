// Farthest point sampling for the downsample point encoder (core/transformer/point.py:150-157, torch_cluster.fps with
// random_start=False): per cloud, sample 0 is point 0, dist[i] = d(p_i, p_0); then for k = 1 .. S-1, s_k = argmax(dist) with the
// lowest index on ties and dist = min(dist, d(p_i, p_{s_k})).  d(a, b) = (dx*dx + dy*dy) + dz*dz in fp32, every product and sum
// rounded on its own (no FMA contraction), so the indices are bit-exact against a plain fp32 restatement.
//
// One 1024-thread workgroup per cloud, all clouds of a call in one launch.  The S - 1 rounds are dependent, so the design is about
// the latency of one round: each thread owns points tid, tid + 1024, ...; the arg-max is one max over the packed 64-bit key
// (float_bits(dist) << 32) | (0xFFFFFFFF - i) (dist >= 0, so the float bits order like the values and the larger low word is the
// lower index), reduced across the wave with v_permlane32/16_swap + DPP (er_common.h) and across the 16 waves with one LDS exchange
// per round: each wave's winner writes its key and coordinates into a double-buffered slot, one barrier, then a 16-lane DPP
// reduction over the slots that carries the coordinates along.
//   fps_reg_kernel<PER>: N <= 1024 * PER (PER <= 16, N <= 16384): coordinates and running distances stay in registers.
//   fps_global_kernel:   any N: dist lives in a [B][N] scratch block and the coordinates are re-read every round (same arithmetic,
//                        same keys, identical indices).
#pragma once
#include "er_common.h"

namespace er {

constexpr int FPS_WG = 1024;
constexpr int FPS_WAVES = FPS_WG / ER_WAVE;
constexpr int FPS_REG_MAX = 16 * FPS_WG;      // largest N of the register form

__device__ __forceinline__ float fps_d2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ unsigned long long fps_key(float dist, int i) {
    return ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}

// max of the key over the 64 lanes of the wave (every lane gets it)
__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long v, int lane) {
#define FPS_STEP(OFF)                                                                                  \
    {                                                                                                  \
        const unsigned hi = lane_xor_bits<OFF>((unsigned)(v >> 32), lane);                             \
        const unsigned lo = lane_xor_bits<OFF>((unsigned)v, lane);                                     \
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;                              \
        v = o > v ? o : v;                                                                             \
    }
    FPS_STEP(32) FPS_STEP(16) FPS_STEP(8) FPS_STEP(4) FPS_STEP(2) FPS_STEP(1)
#undef FPS_STEP
    return v;
}

struct alignas(16) FpsSlot {    // one wave's winner of one round (32 bytes: two 16-byte LDS reads)
    unsigned long long key;
    float x, y, z, pad[3];
};

// The round's exchange: the wave winner (best == wave max) publishes its slot, one barrier, then every row of 16 lanes reads the 16
// slots (lane l reads slot l % 16) and reduces them with DPP, carrying the coordinates along.  Returns the winning index;
// (cx, cy, cz) = its coordinates.  Waves without a valid point publish key 0, which never wins.
__device__ __forceinline__ int fps_block_argmax(unsigned long long best, float bx, float by, float bz, FpsSlot* slots, float& cx,
                                                float& cy, float& cz) {
    static_assert(FPS_WAVES == 16, "one slot per lane of a DPP row");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long wmax = fps_wave_max(best, lane);
    if (best == wmax) slots[wave] = FpsSlot{wmax, bx, by, bz, {0.f, 0.f, 0.f}};   // keys are unique: one writer per wave
    __syncthreads();
    const FpsSlot sl = slots[lane & 15];
    unsigned long long m = sl.key;
    float x = sl.x, y = sl.y, z = sl.z;
#define FPS_ROW_STEP(OFF)                                                                              \
    {                                                                                                  \
        const unsigned hi = lane_xor_bits<OFF>((unsigned)(m >> 32), lane);                             \
        const unsigned lo = lane_xor_bits<OFF>((unsigned)m, lane);                                     \
        const float ox = lane_xor<OFF>(x), oy = lane_xor<OFF>(y), oz = lane_xor<OFF>(z);              \
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;                              \
        if (o > m) { m = o; x = ox; y = oy; z = oz; }                                                  \
    }
    FPS_ROW_STEP(8) FPS_ROW_STEP(4) FPS_ROW_STEP(2) FPS_ROW_STEP(1)
#undef FPS_ROW_STEP
    cx = x; cy = y; cz = z;
    return (int)(0xFFFFFFFFu - (unsigned)m);
}

template <int PER>
__global__ __launch_bounds__(FPS_WG) void fps_reg_kernel(const float* __restrict__ pts, int N, int S, int32_t* __restrict__ idx) {
    __shared__ FpsSlot slots[2][FPS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* p = pts + (size_t)b * N * 3;
    int32_t* out = idx + (size_t)b * S;
    float x[PER], y[PER], z[PER], d[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * FPS_WG + tid;
        const bool ok = i < N;
        x[j] = ok ? p[(size_t)i * 3 + 0] : 0.f;
        y[j] = ok ? p[(size_t)i * 3 + 1] : 0.f;
        z[j] = ok ? p[(size_t)i * 3 + 2] : 0.f;
        d[j] = __builtin_huge_valf();
    }
    float cx = p[0], cy = p[1], cz = p[2];
    if (tid == 0) out[0] = 0;
    for (int k = 1; k < S; ++k) {
        unsigned long long best = 0;       // below every valid key (the low word of a valid key is > 0)
        float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = j * FPS_WG + tid;
            d[j] = fminf(d[j], fps_d2(x[j], y[j], z[j], cx, cy, cz));
            const unsigned long long key = i < N ? fps_key(d[j], i) : 0ull;
            if (key > best) { best = key; bx = x[j]; by = y[j]; bz = z[j]; }
        }
        const int s = fps_block_argmax(best, bx, by, bz, slots[k & 1], cx, cy, cz);
        if (tid == 0) out[k] = s;
    }
}

// dist: [B][N] scratch (written before it is read: no initialisation needed)
__global__ __launch_bounds__(FPS_WG) void fps_global_kernel(const float* __restrict__ pts, int N, int S, int32_t* __restrict__ idx,
                                                            float* __restrict__ dist) {
    __shared__ FpsSlot slots[2][FPS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* p = pts + (size_t)b * N * 3;
    float* dd = dist + (size_t)b * N;
    int32_t* out = idx + (size_t)b * S;
    float cx = p[0], cy = p[1], cz = p[2];
    if (tid == 0) out[0] = 0;
    for (int k = 1; k < S; ++k) {
        unsigned long long best = 0;
        float bx = 0.f, by = 0.f, bz = 0.f;
        for (int i = tid; i < N; i += FPS_WG) {
            const float px = p[(size_t)i * 3 + 0], py = p[(size_t)i * 3 + 1], pz = p[(size_t)i * 3 + 2];
            const float e = fps_d2(px, py, pz, cx, cy, cz);
            const float v = k == 1 ? e : fminf(dd[i], e);      // round 1: min(+inf, e) == e
            dd[i] = v;
            const unsigned long long key = fps_key(v, i);
            if (key > best) { best = key; bx = px; by = py; bz = pz; }
        }
        const int s = fps_block_argmax(best, bx, by, bz, slots[k & 1], cx, cy, cz);
        if (tid == 0) out[k] = s;
    }
}

// B clouds of N points ([B][N][3] fp32) -> S indices per cloud ([B][S] int32, 0-based within the cloud).  dist_scratch: B * N floats,
// read only when N > FPS_REG_MAX.
inline hipError_t launch_fps(const float* pts, int B, int N, int S, int32_t* idx, float* dist_scratch, hipStream_t st) {
    const dim3 grid(B), block(FPS_WG);
    const int per = (N + FPS_WG - 1) / FPS_WG;
    if (per <= 1) hipLaunchKernelGGL(fps_reg_kernel<1>, grid, block, 0, st, pts, N, S, idx);
    else if (per <= 2) hipLaunchKernelGGL(fps_reg_kernel<2>, grid, block, 0, st, pts, N, S, idx);
    else if (per <= 4) hipLaunchKernelGGL(fps_reg_kernel<4>, grid, block, 0, st, pts, N, S, idx);
    else if (per <= 8) hipLaunchKernelGGL(fps_reg_kernel<8>, grid, block, 0, st, pts, N, S, idx);
    else if (per <= 16) hipLaunchKernelGGL(fps_reg_kernel<16>, grid, block, 0, st, pts, N, S, idx);
    else hipLaunchKernelGGL(fps_global_kernel, grid, block, 0, st, pts, N, S, idx, dist_scratch);
    return hipGetLastError();
}

// rows[b][k][:] = x[b * N + idx[b][k]][:]  (the queries of the downsample encoder: pre-LayerNorm point_embed rows of the samples).
// One workgroup per output row (grid = B * S), C % 4 == 0.
__global__ __launch_bounds__(ER_WG) void fps_gather_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx, int N,
                                                                int S, int C, float* __restrict__ out) {
    const long long r = blockIdx.x;
    const long long src = (r / S) * N + idx[r];
    const f32x4* in = reinterpret_cast<const f32x4*>(x + src * C);
    f32x4* o = reinterpret_cast<f32x4*>(out + r * C);
    for (int c = threadIdx.x; c < C / 4; c += blockDim.x) o[c] = in[c];
}

}  // namespace er
