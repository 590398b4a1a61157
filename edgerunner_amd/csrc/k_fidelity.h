// Reconstruction fidelity of a generated mesh against the cloud it was conditioned on: nearest-neighbour squared distances in both
// directions without a distance matrix, area-weighted surface sampling of a ragged batch of meshes, and the reduction of the two
// distance arrays to Chamfer L1 / L2, Hausdorff and F-score.  Every step is specified to the bit (tests/fidelity_ref.py restates it
// in numpy): fp32 / double arithmetic with contraction off, integer face weights, Philox4x32-10 random words, fixed-order sums.
//
//   nn_dist2_kernel<Q>:     grid (query blocks, key splits, B).  A workgroup holds Q queries per lane in registers (256 Q per
//                           workgroup) and walks its share of the keys in tiles of NN_TILE staged in LDS as float4; every lane reads the
//                           same tile entry (one broadcast ds_read_b128 feeds Q distance evaluations).  Q = 4 when that still gives
//                           NN_TARGET_WGS workgroups at one key tile each, else 2, else 1 (nn_pick_q).  Within a lane the key index
//                           only grows, so "strictly smaller float bits wins" is the minimum of the packed key
//                           (float_bits(d) << 32) | j; the key splits of a query meet in a 64-bit atomicMin on that packed key in a
//                           buffer pre-filled with ones.  Keys are unique and min is associative: the result does not depend on the order
//                           of arrival.  nn_unpack_kernel splits the packed minimum into d2 / idx.
//   face_weight_kernel:     w_f = llrint(area_f * 2^32) in double from the fp32 coordinates; checks every face index against the
//                           mesh's vertex range BEFORE a vertex is read through it (bad[m] = 1, weight 0).
//   face_scan_kernel:       in-place inclusive uint64 prefix sum of the weights, one workgroup per mesh.
//   surface_sample_kernel:  one lane per sample: face by binary search of mulhi64(r0:r1, total) in the prefix sums, barycentric
//                           coordinates from r2 / r3.
//   fidelity_metrics_kernel: one workgroup per batch entry, per-thread strided sums in double and one fixed LDS tree.
#pragma once
#include <cstdlib>
#include "er_common.h"
#include "k_fps.h"
#include "k_head.h"

namespace er {

constexpr int NN_TILE = 256;                 // keys per LDS tile (one per thread to stage); the smallest key share of a workgroup
constexpr int NN_TARGET_WGS = 1024;          // 4 workgroups per CU: the keys are split, and the queries per lane lowered, to get there
constexpr int FID_MAX_N = 1 << 30;           // points per cloud
constexpr int FID_MAX_FACES = 1 << 22;       // faces per mesh (weights < 2^41 at |coordinate| <= 8: the total stays below 2^63)
constexpr int FID_SCAN_ITEMS = 8;            // consecutive faces per thread and round of face_scan_kernel
constexpr unsigned FID_PHILOX_TAG = 0x53555246u;   // "SURF": third counter word of the sampler's draws

struct FidMesh {      // one mesh of a ragged batch: first vertex / face in the concatenated arrays, their counts, Philox stream id
    int v0, nv, f0, nf;
    unsigned stream;
};

// keys_per_wg: a multiple of NN_TILE with blockIdx.y * keys_per_wg < Nb for every workgroup of the launch
template <int NN_Q>
__global__ __launch_bounds__(ER_WG) void nn_dist2_kernel(const float* __restrict__ a, const float* __restrict__ b, int Na, int Nb,
                                                         int keys_per_wg, unsigned long long* __restrict__ packed) {
    __shared__ f32x4 tile[NN_TILE];
    const int tid = threadIdx.x, bi = blockIdx.z;
    const float* qa = a + (size_t)bi * Na * 3;
    const float* kb = b + (size_t)bi * Nb * 3;
    const int q0 = blockIdx.x * (ER_WG * NN_Q);
    const int k_lo = blockIdx.y * keys_per_wg;
    const int k_hi = Nb - k_lo < keys_per_wg ? Nb : k_lo + keys_per_wg;
    float qx[NN_Q], qy[NN_Q], qz[NN_Q];
    unsigned best[NN_Q], besti[NN_Q];
#pragma unroll
    for (int q = 0; q < NN_Q; ++q) {
        const int i = q0 + q * ER_WG + tid;
        const bool ok = i < Na;
        qx[q] = ok ? qa[(size_t)i * 3 + 0] : 0.f;
        qy[q] = ok ? qa[(size_t)i * 3 + 1] : 0.f;
        qz[q] = ok ? qa[(size_t)i * 3 + 2] : 0.f;
        best[q] = 0xFFFFFFFFu;
        besti[q] = 0xFFFFFFFFu;
    }
    for (int t0 = k_lo; t0 < k_hi; t0 += NN_TILE) {
        const int kn = k_hi - t0 < NN_TILE ? k_hi - t0 : NN_TILE;
        __syncthreads();                       // the previous tile has been read
        if (tid < kn) {
            const float* p = kb + (size_t)(t0 + tid) * 3;
            tile[tid] = f32x4{p[0], p[1], p[2], 0.f};
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kn; ++k) {
            const f32x4 c = tile[k];           // the same address in every lane: a broadcast read
#pragma unroll
            for (int q = 0; q < NN_Q; ++q) {
                const unsigned d = __float_as_uint(fps_d2(qx[q], qy[q], qz[q], c.x, c.y, c.z));
                if (d < best[q]) { best[q] = d; besti[q] = (unsigned)(t0 + k); }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NN_Q; ++q) {
        const int i = q0 + q * ER_WG + tid;
        if (i < Na) atomicMin(&packed[(size_t)bi * Na + i], ((unsigned long long)best[q] << 32) | besti[q]);
    }
}

__global__ __launch_bounds__(ER_WG) void nn_unpack_kernel(const unsigned long long* __restrict__ packed, long long total,
                                                          float* __restrict__ d2, int32_t* __restrict__ idx) {
    for (long long i = (long long)blockIdx.x * ER_WG + threadIdx.x; i < total; i += (long long)gridDim.x * ER_WG) {
        const unsigned long long k = packed[i];
        d2[i] = __uint_as_float((unsigned)(k >> 32));
        if (idx) idx[i] = (int32_t)(unsigned)k;
    }
}

// Queries per lane: the most (fewest key reads per distance) that still fills the chip when every workgroup takes one key tile.
// ER_NN_Q = 1 / 2 / 4 forces a form (A/B handle and unit tests: all forms give identical bits); read per launch.
inline int nn_pick_q(int B, int Na, int tiles) {
    if (const char* e = getenv("ER_NN_Q")) {
        const int v = atoi(e);
        if (v == 1 || v == 2 || v == 4) return v;
    }
    for (int q = 4; q > 1; q >>= 1) {
        const long long qblocks = (Na + ER_WG * q - 1) / (ER_WG * q);
        if ((long long)B * qblocks * tiles >= NN_TARGET_WGS) return q;
    }
    return 1;
}

// a [B][Na][3], b [B][Nb][3] -> d2 [B][Na], idx [B][Na] (nullable).  packed: B * Na 64-bit words of scratch.
inline hipError_t launch_nn_dist2(const float* a, const float* b, int B, int Na, int Nb, float* d2, int32_t* idx,
                                  unsigned long long* packed, hipStream_t st) {
    if (B <= 0 || B > 65535 || Na <= 0 || Nb <= 0 || Na > FID_MAX_N || Nb > FID_MAX_N) return hipErrorInvalidValue;
    const long long total = (long long)B * Na;
    hipError_t e = hipMemsetAsync(packed, 0xFF, (size_t)total * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const int tiles = (Nb + NN_TILE - 1) / NN_TILE;
    const int nq = nn_pick_q(B, Na, tiles);
    const int qblocks = (Na + ER_WG * nq - 1) / (ER_WG * nq);
    const long long wgs = (long long)B * qblocks;
    const int want = (int)std::min<long long>((NN_TARGET_WGS + wgs - 1) / wgs, 65535);
    const int tiles_per_wg = (tiles + std::min(want, tiles) - 1) / std::min(want, tiles);
    const int splits = (tiles + tiles_per_wg - 1) / tiles_per_wg;          // no workgroup without keys
    if (splits > 65535) return hipErrorInvalidValue;
    const dim3 grid(qblocks, splits, B), block(ER_WG);
    const int keys_per_wg = tiles_per_wg * NN_TILE;
    if (nq == 4) hipLaunchKernelGGL(nn_dist2_kernel<4>, grid, block, 0, st, a, b, Na, Nb, keys_per_wg, packed);
    else if (nq == 2) hipLaunchKernelGGL(nn_dist2_kernel<2>, grid, block, 0, st, a, b, Na, Nb, keys_per_wg, packed);
    else hipLaunchKernelGGL(nn_dist2_kernel<1>, grid, block, 0, st, a, b, Na, Nb, keys_per_wg, packed);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned ugrid = (unsigned)std::min<long long>((total + ER_WG - 1) / ER_WG, 4096);
    hipLaunchKernelGGL(nn_unpack_kernel, dim3(ugrid), dim3(ER_WG), 0, st, packed, total, d2, idx);
    return hipGetLastError();
}

// grid (chunks, B): w[f0 + f] of mesh blockIdx.y
__global__ __launch_bounds__(ER_WG) void face_weight_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                            const FidMesh* __restrict__ meshes, unsigned long long* __restrict__ w,
                                                            int* __restrict__ bad) {
#pragma clang fp contract(off)
    const FidMesh m = meshes[blockIdx.y];
    for (int f = blockIdx.x * ER_WG + threadIdx.x; f < m.nf; f += gridDim.x * ER_WG) {
        const int32_t* t = faces + (size_t)(m.f0 + f) * 3;
        const int i0 = t[0], i1 = t[1], i2 = t[2];
        if ((unsigned)i0 >= (unsigned)m.nv || (unsigned)i1 >= (unsigned)m.nv || (unsigned)i2 >= (unsigned)m.nv) {
            atomicOr(&bad[blockIdx.y], 1);
            w[m.f0 + f] = 0;
            continue;
        }
        const float* p0 = verts + (size_t)(m.v0 + i0) * 3;
        const float* p1 = verts + (size_t)(m.v0 + i1) * 3;
        const float* p2 = verts + (size_t)(m.v0 + i2) * 3;
        const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
        const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        w[m.f0 + f] = (unsigned long long)llrint(area * 4294967296.0);
    }
}

// grid (B): w of mesh blockIdx.x becomes its inclusive prefix sum; total[mesh] = the last entry (0 for a mesh without faces)
__global__ __launch_bounds__(ER_WG) void face_scan_kernel(unsigned long long* __restrict__ w, const FidMesh* __restrict__ meshes,
                                                          unsigned long long* __restrict__ total) {
    __shared__ unsigned long long s[ER_WG];
    const FidMesh m = meshes[blockIdx.x];
    const int tid = threadIdx.x;
    unsigned long long* base = w + m.f0;
    unsigned long long carry = 0;
    for (int c0 = 0; c0 < m.nf; c0 += ER_WG * FID_SCAN_ITEMS) {
        const int lo = c0 + tid * FID_SCAN_ITEMS;
        unsigned long long v[FID_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int j = 0; j < FID_SCAN_ITEMS; ++j) {
            v[j] = lo + j < m.nf ? base[lo + j] : 0ull;
            sum += v[j];
        }
        s[tid] = sum;
        __syncthreads();
        for (int off = 1; off < ER_WG; off <<= 1) {
            const unsigned long long t = tid >= off ? s[tid - off] : 0ull;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        unsigned long long run = carry + s[tid] - sum;
#pragma unroll
        for (int j = 0; j < FID_SCAN_ITEMS; ++j) {
            run += v[j];
            if (lo + j < m.nf) base[lo + j] = run;
        }
        carry += s[ER_WG - 1];
        __syncthreads();                       // s is rewritten by the next round
    }
    if (tid == 0) total[blockIdx.x] = carry;
}

// grid (chunks, B): sample i of mesh blockIdx.y -> points[mesh][i][:], face[mesh][i] (nullable).  total[mesh] > 0.
__global__ __launch_bounds__(ER_WG) void surface_sample_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                               const FidMesh* __restrict__ meshes,
                                                               const unsigned long long* __restrict__ cum,
                                                               const unsigned long long* __restrict__ total, int n, unsigned seed_lo,
                                                               unsigned seed_hi, float* __restrict__ points, int32_t* __restrict__ face) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * ER_WG + threadIdx.x;
    if (i >= n) return;
    const FidMesh m = meshes[blockIdx.y];
    unsigned r[4];
    philox4x32_10((unsigned)i, m.stream, FID_PHILOX_TAG, 0u, seed_lo, seed_hi, r);
    const unsigned long long t = __umul64hi(((unsigned long long)r[0] << 32) | r[1], total[blockIdx.y]);
    const unsigned long long* c = cum + m.f0;
    int lo = 0, hi = m.nf - 1;                 // the smallest f with c[f] > t; t < total = c[nf - 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int32_t* tri = faces + (size_t)(m.f0 + lo) * 3;
    const float* p0 = verts + (size_t)(m.v0 + tri[0]) * 3;
    const float* p1 = verts + (size_t)(m.v0 + tri[1]) * 3;
    const float* p2 = verts + (size_t)(m.v0 + tri[2]) * 3;
    float u = (float)(r[2] >> 8) * (1.0f / 16777216.0f), v = (float)(r[3] >> 8) * (1.0f / 16777216.0f);
    if (u + v > 1.f) { u = 1.f - u; v = 1.f - v; }
    float* o = points + ((size_t)blockIdx.y * n + i) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (p0[k] + u * (p1[k] - p0[k])) + v * (p2[k] - p0[k]);
    if (face) face[(size_t)blockIdx.y * n + i] = lo;
}

constexpr int FID_METRICS = 8;      // doubles per batch entry of the metrics output
// grid (B).  Thread t sums elements t, t + 256, ... of each direction in double, then one fixed LDS tree over eight slots per thread
// ({sum of distances, sum of squared distances, max squared distance, count within tau} x {a -> b, b -> a}): no atomics, the same
// bits from run to run.
__global__ __launch_bounds__(ER_WG) void fidelity_metrics_kernel(const float* __restrict__ d2_ab, const float* __restrict__ d2_ba, int Na,
                                                                 int Nb, float tau, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[8][ER_WG];
    const int tid = threadIdx.x, b = blockIdx.x;
    const double dtau = (double)tau;
    double v[8];
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const float* d2 = dir == 0 ? d2_ab + (size_t)b * Na : d2_ba + (size_t)b * Nb;
        const int n = dir == 0 ? Na : Nb;
        double s1 = 0.0, s2 = 0.0, mx = 0.0, cnt = 0.0;
        for (int i = tid; i < n; i += ER_WG) {
            const double q = (double)d2[i], d = sqrt(q);
            s1 += d;
            s2 += q;
            mx = q > mx ? q : mx;
            cnt += d < dtau ? 1.0 : 0.0;
        }
        v[4 * dir + 0] = s1; v[4 * dir + 1] = s2; v[4 * dir + 2] = mx; v[4 * dir + 3] = cnt;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[k][tid] = v[k];
    __syncthreads();
    for (int off = ER_WG / 2; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double x = red[k][tid], y = red[k][tid + off];
                red[k][tid] = (k & 3) == 2 ? (y > x ? y : x) : x + y;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double mean_ab = red[0][0] / (double)Na, mean_ba = red[4][0] / (double)Nb;
        const double mx = red[2][0] > red[6][0] ? red[2][0] : red[6][0];
        const double recall = red[3][0] / (double)Na, precision = red[7][0] / (double)Nb;
        double* o = out + (size_t)b * FID_METRICS;
        o[0] = mean_ab + mean_ba;
        o[1] = red[1][0] / (double)Na + red[5][0] / (double)Nb;
        o[2] = sqrt(mx);
        o[3] = precision;
        o[4] = recall;
        o[5] = precision + recall > 0.0 ? 2.0 * precision * recall / (precision + recall) : 0.0;
        o[6] = mean_ab;
        o[7] = mean_ba;
    }
}

inline hipError_t launch_fidelity_metrics(const float* d2_ab, const float* d2_ba, int B, int Na, int Nb, float tau, double* out,
                                          hipStream_t st) {
    if (B <= 0 || Na <= 0 || Nb <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fidelity_metrics_kernel, dim3(B), dim3(ER_WG), 0, st, d2_ab, d2_ba, Na, Nb, tau, out);
    return hipGetLastError();
}

}  // namespace er
