// Forking cache rows (er_prefill_fork, er_k_kv_fork): positions [0, len) of K and V, every layer and head, copied from SOURCE rows to
// DESTINATION rows of one cache [layer][B][H][Lcap][D], as bytes - the element size only scales the slab, so fp32, fp16 and the e4m3 byte
// cache take the same kernel.  A GROUP is one source row and the rows that receive its copy.
//
// Within a head the first len positions are one contiguous slab of len * D * esz bytes, a multiple of 16 at a 16-byte aligned offset
// for D % 16 == 0 (96, 64) - what prefix_check_kernel (k_attn_shared.h) rests on, and the slab is addressed the same way (head_bytes,
// row_bytes, layer_bytes; 16 bytes per lane).  Grid (H, 2 * layers, groups of the launch): one workgroup per (head, K | V x layer,
// group).  It walks the slab in pieces of KVF_LOADS x 256 x 16 bytes (and a rest of single rounds): KVF_LOADS independent loads per lane
// are issued before the first store (the loads of a piece are in flight together; a load-store-load-store chain would wait out one
// HBM latency per 16 bytes), then the piece goes to every destination of the group from registers - the source crosses HBM once per
// group, not once per destination.  No LDS, no barrier: a lane stores what it loaded.
//
// Load / store flavour: both non-temporal (__builtin_nontemporal_load / _store, the `nt` bit).  A source byte is read exactly once by
// exactly one lane of the whole launch, so a line in the CU's L1 buys nothing: `nt` loads skip L1 and are served by L2.  A destination is
// not read by this launch and not soon after it (the first decode step reads it once, after the head and under prefix groups never),
// so the stores carry the same hint.  `nt` stores are plain write-back stores to the memory system: the consumer is a LATER kernel on
// the same stream, and the kernel boundary makes them visible - no write-through (sc1) store, fence or flag is needed, and none is used.
//
// The group table travels in the kernel arguments (no device table to allocate, upload or keep alive, so the launch can be captured in
// a graph): at most KVF_MAX_GROUPS sources and KVF_MAX_DSTS destinations per launch, more are cut into several launches (a group with
// more destinations than a launch holds is continued in the next one and reads its source again).
#pragma once
#include "er_common.h"

namespace er {

constexpr int KVF_LOADS = 4;            // 16-byte loads per lane in flight before the first store (16 VGPRs of payload)
constexpr int KVF_MAX_GROUPS = 64, KVF_MAX_DSTS = 64;

struct KvForkArgs {
    char *kc, *vc;               // [layers][B][H][Lcap][D]
    long long head_bytes, row_bytes, layer_bytes;      // Lcap * D, H * Lcap * D, B * H * Lcap * D elements in bytes
    long long slab_vecs;         // len * D * element size / 16
    int src[KVF_MAX_GROUPS];     // source row of group g
    int off[KVF_MAX_GROUPS + 1]; // its destinations: dst[off[g]] .. dst[off[g + 1] - 1]
    int dst[KVF_MAX_DSTS];
};

__global__ __launch_bounds__(ER_WG) void kv_fork_kernel(KvForkArgs p) {
    const int h = blockIdx.x, layer = blockIdx.y >> 1, g = blockIdx.z;
    char* base = ((blockIdx.y & 1) ? p.vc : p.kc) + layer * p.layer_bytes + h * p.head_bytes;
    const er_u32x4* src = reinterpret_cast<const er_u32x4*>(base + p.src[g] * p.row_bytes);
    const int d0 = p.off[g], d1 = p.off[g + 1];
    // whole pieces: the KVF_LOADS loads are unconditional, so nothing but the first store waits for them
    constexpr long long PIECE = (long long)KVF_LOADS * ER_WG;
    const long long whole = p.slab_vecs / PIECE * PIECE;
    for (long long i0 = threadIdx.x; i0 < whole; i0 += PIECE) {
        er_u32x4 r[KVF_LOADS];
#pragma unroll
        for (int j = 0; j < KVF_LOADS; ++j) r[j] = __builtin_nontemporal_load(src + i0 + j * ER_WG);
        for (int d = d0; d < d1; ++d) {
            er_u32x4* dst = reinterpret_cast<er_u32x4*>(base + p.dst[d] * p.row_bytes);
#pragma unroll
            for (int j = 0; j < KVF_LOADS; ++j) __builtin_nontemporal_store(r[j], dst + i0 + j * ER_WG);
        }
    }
    // the rest of the slab (fewer than PIECE vectors): at most KVF_LOADS - 1 rounds of one load per lane
    for (long long i = whole + threadIdx.x; i < p.slab_vecs; i += ER_WG) {
        const er_u32x4 r = __builtin_nontemporal_load(src + i);
        for (int d = d0; d < d1; ++d) __builtin_nontemporal_store(r, reinterpret_cast<er_u32x4*>(base + p.dst[d] * p.row_bytes) + i);
    }
}

// n_pairs copies src_rows[i] -> dst_rows[i] (host arrays; pairs of one source need not be adjacent: groups form in first-occurrence
// order of their source).  The caller has checked the rows, the slab and the alignment (er_api.hip kv_fork_check); nothing here blocks.
inline hipError_t launch_kv_fork(KvForkArgs a, int heads, int layers, const int* src_rows, const int* dst_rows, int n_pairs, hipStream_t st) {
    if (n_pairs < 1) return hipSuccess;
    int groups = 0, dsts = 0;
    const auto flush = [&]() -> hipError_t {
        if (!groups) return hipSuccess;
        a.off[groups] = dsts;
        hipLaunchKernelGGL(kv_fork_kernel, dim3(heads, 2 * layers, groups), dim3(ER_WG), 0, st, a);
        groups = dsts = 0;
        return hipGetLastError();
    };
    for (int i = 0; i < n_pairs; ++i) {
        bool seen = false;
        for (int k = 0; k < i && !seen; ++k) seen = src_rows[k] == src_rows[i];
        if (seen) continue;              // its group was written when the source first appeared
        bool open = false;
        for (int k = i; k < n_pairs; ++k) {
            if (src_rows[k] != src_rows[i]) continue;
            if (!open || dsts == KVF_MAX_DSTS) {
                if (dsts == KVF_MAX_DSTS || groups == KVF_MAX_GROUPS) {
                    const hipError_t e = flush();
                    if (e != hipSuccess) return e;
                }
                a.src[groups] = src_rows[i];
                a.off[groups] = dsts;
                ++groups;
                open = true;
            }
            a.dst[dsts++] = dst_rows[k];
        }
    }
    return flush();
}

}  // namespace er
