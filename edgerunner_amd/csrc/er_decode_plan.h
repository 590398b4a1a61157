// Which kernels a reserved cache shape decodes with, and in which form each of its five projections is launched: the knobs, the plan
// and the two functions launch_kind_t and the single-kernel entries take their decisions from.  Pure C++ with no device call
// (csrc/er_queue_host.h is the precedent), so that the whole decision table can be enumerated by a stand-alone program
// (tests/host/decode_plan_check.cpp).  csrc/er_weight_source.h decides, from the plan and the form, which copy of its matrix a projection
// streams (weight_source: the one rule), and csrc/er_decode_proj.h turns a (projection, form, source) into launches.
#pragma once
#include "../../include/edgerunner_hip.h"

namespace er {

struct DecodeKnobs {          // the environment knobs of the decode step, read once per context by er_create (read_knobs)
    bool use_graph = true;    // ER_NO_GRAPH=1: eager launches
    // waves per workgroup of the qkv / fc1 GEMVs (env ER_NW_QKV: 4, 6 or 9; ER_NW_FC1: 4 or 12).  Exact mode: qkv 6 waves x 1 row
    // = 768 workgroups (3 per CU), fc1 4 waves x 2 rows = 768; fast mode: one fat workgroup per CU (9 / 12 waves x 2 rows).  The other
    // shapes are fixed (out_proj 3 waves x 1 row, fc2 4 K-slices x 2 rows, 128-key chunks for the fixed-chunk attention): their
    // round-1/2 knobs (ER_RW_*, ER_NW_OUT, ER_ATTN_STEPS, ER_ATTN_V, ER_COMBINE_V, ER_ATTN_GRID_HS, ER_OUT_VALU) are settled and gone
    int nw_qkv = 6, nw_fc1 = 4;
    int prefill_attn_f16s = -1;   // fast-mode prefix attention on the fp16 matrix cores with hi/lo-split q and p (k_flash_attn_f16s.h): on unless
                                  // ER_PREFILL_ATTN_F16S=0 (the fp32-matrix-core kernel; kept for the parity matrix)
    int attn_v_batched = 0;   // attention kernel at B > 4 (env ER_ATTN_V_BATCHED): 0 = auto (streaming when B*H >= 256, else split + merge), 1 = split kernel + merge, 3 = one streaming workgroup per (row, head), no merge
    int decode_v = 3;         // single-row decode: 3 = balanced-chunk attention + merge fused into out_proj (one row, D = 96, 16 heads, Lcap <= 8192); ER_DECODE_V=2 = fixed 128-key chunks + merge kernel (also the fallback when the cache does not qualify)
    int rw_fc2 = 6;           // fast mode, one row: rows per fc2 workgroup (env ER_RW_FC2: 2 / 4 / 6, anything else runs as 2; proj_form)
    // single-row MLP (env ER_MLP_V): 0 = fc1 and fc2 as two row GEMVs, 1 = fused launch that skips the fc2 weights behind zero ReLU outputs
    // + finish launch (k_mlp_sparse.h)
    int mlp_v = 0;
    // the prefix pass under prefix groups (env ER_PREFIX_PASS=valu|mfma at er_create, er_set_prefix_pass later): ER_PREFIX_PASS_VALU =
    // attn_prefix_kernel, ER_PREFIX_PASS_MFMA = attn_prefix_mfma_kernel where the plan qualifies (make_decode_plan: shared_mfma)
    int prefix_pass = ER_PREFIX_PASS_VALU;
    // fp8 mode, matrix-core batched forms (env ER_W8_BATCHED): -1 = stream bytes where the measured rule says so (er_weight_source.h
    // w8_streams_batched: qkv, fc1, fc2 at B > 4), 0 = the fp16 tiled copies everywhere, 1 = bytes in every matrix-core form
    int w8_batched = -1;
    // fp4 mode, row forms (env ER_W4_ROWS): -1 = stream nibbles where the measured rule says so (er_w4_rule.h w4_streams), 0 = the
    // fp16 copies everywhere, 1 = nibbles in every row form that has one (qkv, fc1, fc2 at B <= 4)
    int w4_rows = -1;
    // fp4 mode, matrix-core batched forms (env ER_W4_BATCHED): -1 = stream nibbles where the measured rule says so (er_w4_rule.h
    // w4_streams_batched: all four at B > 4), 0 = the fp16 tiled copies everywhere, 1 = nibbles in every matrix-core form of qkv, out_proj, fc1 and fc2
    int w4_batched = -1;
};

// the three switches er_kv_reserve reads for the shape it reserves (tests flip them between two reserves of one context)
struct ReserveKnobs { bool force_batched, batched_valu, xt; };

// The chunking of the attention kernels as numbers: er_api.hip fills it from k_attn_decode.h (attn_chunking), so the host rules compare
// a cache length with the kernels' own figures.
struct AttnChunking {
    int nch3;    // chunks per head of the balanced kernel (attn3_num_chunks)
    int cap3;    // keys the balanced kernel covers: nch3 chunks of ATTN3_CAP
    int chunk;   // keys per workgroup of the fixed-chunk kernels (attn_chunk)
};

// Everything the decode step branches on for ONE reserved cache shape: make_decode_plan computes it once, kv_alloc stores it in the KvMem
// it describes, it is installed and dropped with that object, and launch_kind_t and the other readers take their decisions from here.
struct DecodePlan {
    int B = 0, Lcap = 0, layers = 0;            // B == 0: no cache reserved
    long long kv_bstride = 0, kv_lstride = 0;   // elements per batch row / per layer of the cache
    int S_splits = 0, nch3 = 0;                 // chunks per (row, head) of the fixed-chunk attention / per head of the balanced kernel
    er_decode_plan sel{};                       // what plan_decode chose (er_ctx_plan reports it) ...
    bool force_batched = false;                 // ... under this ER_FORCE_BATCHED
    bool batched = false;       // B > 4 (or ER_FORCE_BATCHED=1): weights streamed once per pass of 32 rows (matrix cores)
    bool valu = false;          // ER_BATCHED_VALU=1: the older VALU kernels (one pass per 16 rows), kept for A/B runs
    bool mfma = false;          // batched and not valu: the projections run on the matrix cores and read the tiled weight copies
    bool xt = false;            // fast-mode batches read the tiled activation images (KvMem::xt_*); ER_XT=0 keeps the row-major fp32 inputs (A/B + parity matrix)
    bool stream_attn = false;   // batched, D == 96 and (forced or B*H >= 256: at least one streaming workgroup per CU)
    bool shared_attn = false;   // prefix groups are set (er_set_prefix_groups; batched, D == 96): prefix pass + suffix / merge launch (k_attn_shared.h) in place of either batched kernel
    bool shared_mfma = false;   // shared_attn, knobs.prefix_pass == ER_PREFIX_PASS_MFMA, fp16 cache (fast, not kv8) and D == 96: kind 1 is the matrix-core prefix pass (k_attn_shared_mfma.h)
    ReserveKnobs rk{};          // the switches of the reserve, kept so that setting or clearing groups can derive the plan again
    bool kv8 = false;           // the cache holds e4m3 bytes (kv8 mode): version 2 at B <= 4, the streaming kernel at every batched shape, no prefix groups
    bool v3 = false;            // decode_v == 3 and the reserved cache qualifies
    bool mlp_fused = false;     // mlp_v != 0, one row, not batched, hidden 1536: kinds 4 and 5 are the fused MLP launch and its finish
    bool outproj_rows8 = false; // mfma and 5..8 rows: out_proj is ONE pass of the VALU kernel (ER_FORM_ROWS8)
    // xt, streaming (or shared) attention and B > 8: the attention writes the tiled image xt_att, out_proj reads it and leaves SK_SLICES_OUTPROJ partials, fc1's LayerNorm launch finishes them
    bool outproj_partials = false;
    // fc2 of `layer` leaves SK_SLICES_FC2 partials to the next layer's LayerNorm launch; the last layer finishes into ypre, which the lm_head reads
    bool fc2_defers(int layer) const { return xt && layer >= 0 && layer + 1 < layers; }
};

// ONE place for the selection rules.  er_plan_decode reports them for a hypothetical shape; make_decode_plan derives the DecodePlan of a
// reserved shape from them:
//   batched     : B > 4 (or forced) - weights streamed once per pass of 32 rows on the matrix cores
//   version 3   : one row, 16 heads of 96, hidden 1536, reserved cache <= 16 chunks x 512 keys; else version 2
//   attention B>4: streaming kernel when forced or (auto and B * heads >= 256: at least one workgroup per CU - at B = 16 it
//                  ties the split kernel and saves the merge launch, at B = 8 it is 1.5x slower), else split + merge
//   kv8 (e4m3 byte cache, D = 96): only attn_decode2_kernel and attn_stream_kernel have a byte form - never version 3, and every
//                  batched shape streams (also 5 <= B < 16 and ER_ATTN_V_BATCHED=1: the round-1 split kernel reads no bytes)
inline void plan_decode(int decode_v, int attn_v_batched, bool force_batched, int batch, int H, int D, int hid, int Lcap,
                        const AttnChunking& ch, er_decode_plan* p, bool kv8 = false) {
    p->batched = (batch > 4 || force_batched) ? 1 : 0;
    p->attn_chunks = ch.nch3;
    const bool v3 = !kv8 && decode_v == 3 && batch == 1 && !p->batched && D == 96 && H == 16 && hid == 1536 && Lcap <= ch.cap3;
    p->decode_version = v3 ? 3 : 2;
    const bool stream = p->batched && D == 96 && (kv8 || attn_v_batched == 3 || (attn_v_batched == 0 && batch * H >= 256));
    p->attn_kernel = !p->batched ? (v3 ? ER_ATTN_BALANCED : ER_ATTN_SPLIT2)
                                 : (stream ? ER_ATTN_STREAM : ER_ATTN_SPLIT1);
    p->merge_launch = (p->attn_kernel == ER_ATTN_SPLIT1 || p->attn_kernel == ER_ATTN_SPLIT2) ? 1 : 0;
    p->launches_per_layer = p->batched ? 0 : 5 + p->merge_launch;       // qkv, attention, (merge,) out_proj, fc1, fc2
}

// prefix groups need the batched class and the kernels' head_dim
inline bool shared_attn_supported(const er_decode_plan& sel, int D) { return sel.batched != 0 && D == 96; }

// the plan of one (batch, Lcap) of a model with `layers` layers of H heads of D (hid = hidden width), `fast` = fp16 weights and cache;
// kv8: the cache holds e4m3 bytes (with fast's fp16 weights or fp8 mode's bytes); shared: prefix groups are set on the reserved batch (the caller has asked shared_attn_supported), which replaces the attention kernel
// of plan_decode's shape-only rule by ER_ATTN_SHARED with its own merge launch - ER_ATTN_SHARED_MFMA when the knobs ask for the matrix-core
// prefix pass and the cache is fp16 (the kernel reads fp16 K/V at head_dim 96 only; anything else keeps the VALU pass)
inline DecodePlan make_decode_plan(const DecodeKnobs& k, const ReserveKnobs& rk, bool fast, int batch, int Lcap, int layers, int H, int D,
                                   int hid, const AttnChunking& ch, bool shared = false, bool kv8 = false) {
    DecodePlan p;
    p.B = batch; p.Lcap = Lcap; p.layers = layers;
    p.kv_bstride = (long long)H * Lcap * D; p.kv_lstride = p.kv_bstride * batch;
    p.S_splits = (Lcap + ch.chunk - 1) / ch.chunk;   // decode attention: one workgroup per (row, head, chunk of 32*steps keys)
    p.nch3 = ch.nch3;
    p.force_batched = rk.force_batched; p.valu = rk.batched_valu;
    p.rk = rk;
    plan_decode(k.decode_v, k.attn_v_batched, p.force_batched, batch, H, D, hid, Lcap, ch, &p.sel, kv8);
    p.kv8 = kv8;
    p.shared_attn = shared && !kv8 && shared_attn_supported(p.sel, D);      // the shared-prefix kernels have no byte form
    p.shared_mfma = p.shared_attn && k.prefix_pass == ER_PREFIX_PASS_MFMA && fast && D == 96;
    if (p.shared_attn) { p.sel.attn_kernel = p.shared_mfma ? ER_ATTN_SHARED_MFMA : ER_ATTN_SHARED; p.sel.merge_launch = 1; }
    p.batched = p.sel.batched != 0; p.mfma = p.batched && !p.valu; p.xt = fast && p.mfma && rk.xt;
    p.stream_attn = p.sel.attn_kernel == ER_ATTN_STREAM; p.v3 = p.sel.decode_version == 3;
    p.mlp_fused = k.mlp_v != 0 && batch == 1 && !p.batched && hid == 1536;      // the kernel's fixed widths (intermediate = 4 * hidden)
    p.outproj_rows8 = p.mfma && batch >= 5 && batch <= 8;
    p.outproj_partials = p.xt && (p.stream_attn || p.shared_attn) && batch > 8;      // the shared attention's last launch writes what the streaming kernel writes
    return p;
}

// ------------------------------------------------------------------------------------ the form of a projection
enum Proj { PROJ_QKV = 0, PROJ_OUT, PROJ_FC1, PROJ_FC2, PROJ_HEAD };      // qkv, out_proj, fc1, fc2, lm_head

struct ProjForm {
    int form = ER_FORM_ROW;   // er_gemv_form
    int nw = 0, rw = 0;       // ER_FORM_ROW / ER_FORM_ROWS8: waves per workgroup x weight rows per wave (0 in the batched forms: fixed per projection)
    bool defer = false;       // ER_FORM_NARROW_DEFER: the split-K partials are left to the next LayerNorm launch
};

inline bool form_batched(int form) { return form == ER_FORM_VALU || form == ER_FORM_MFMA || form == ER_FORM_MFMA_XT || form == ER_FORM_NARROW || form == ER_FORM_NARROW_DEFER; }
inline bool form_tiled_in(int form) { return form == ER_FORM_MFMA_XT || form == ER_FORM_NARROW || form == ER_FORM_NARROW_DEFER; }   // the input is a tiled hi | lo image
inline bool form_mfma(int form) { return form == ER_FORM_MFMA || form_tiled_in(form); }                                           // matrix cores: the weights are the tiled copy

// The form the decode step launches `proj` of `layer` in (the fused attention merge + out_proj of version 3 is no GEMV form: launch_kind_t
// asks plan.v3 first).  half: fp16 weights.
inline ProjForm proj_form(const DecodePlan& p, const DecodeKnobs& k, bool half, Proj proj, int layer) {
    const auto batched = [&](int tiled) { return ProjForm{p.xt && half ? tiled : p.mfma ? ER_FORM_MFMA : ER_FORM_VALU, 0, 0, false}; };
    switch (proj) {
        case PROJ_QKV:
            if (p.batched) return batched(ER_FORM_MFMA_XT);
            return ProjForm{ER_FORM_ROW, k.nw_qkv, k.nw_qkv == 9 ? 2 : 1, false};
        case PROJ_OUT:
            // 48 row tiles of 32: the matrix-core kernel runs on 48 CUs only, but streams the matrix ONCE for 32 rows where the VALU
            // kernel needs a pass per 16; the narrow form has 4-wave workgroups (48 row tiles x 4 K-ranges of 384), + bias + residual
            // then happen in fc1's LayerNorm-rows launch, which reads the four partials
            if (p.outproj_rows8) return ProjForm{ER_FORM_ROWS8, 3, 1, false};
            if (p.outproj_partials && half) return ProjForm{ER_FORM_NARROW_DEFER, 0, 0, true};
            if (p.mfma) return ProjForm{ER_FORM_MFMA, 0, 0, false};
            if (p.batched) return ProjForm{ER_FORM_VALU, 0, 0, false};
            return ProjForm{ER_FORM_ROW, 3, 1, false};       // 3 waves x 1 row: 512 workgroups = 2 per CU
        case PROJ_FC1:
            if (p.batched) return batched(ER_FORM_MFMA_XT);      // tiled: input and output images, fc2 reads xt_f
            return ProjForm{ER_FORM_ROW, k.nw_fc1, 2, false};
        case PROJ_FC2:
            // tiled: 4-wave workgroups, 48 row tiles x 16 K-ranges of 384 (768 workgroups = 3 per CU instead of 192 on 192 CUs); layers
            // 0 .. nl-2 leave the partials to the next layer's LayerNorm launch, the last layer finishes into ypre (after a prefill
            // ypre comes from the GEMM path, so the lm_head always reads ypre)
            if (p.xt && half) return p.fc2_defers(layer) ? ProjForm{ER_FORM_NARROW_DEFER, 0, 0, true} : ProjForm{ER_FORM_NARROW, 0, 0, false};
            if (p.mfma) return ProjForm{ER_FORM_MFMA, 0, 0, false};      // 48 tiles x 4 K-ranges
            if (p.batched) return ProjForm{ER_FORM_VALU, 0, 0, false};
            // fast mode, one row: FAT workgroups like qkv's and fc1's - 4 or 6 rows per workgroup instead of 2 (384 / 256 workgroups
            // instead of 768), so that a CU fetches the 24 KB input vector once or twice instead of three times beside its 72 KB of
            // fp16 weights: fc2 5.60 -> 5.37 us at 6 rows, 5.68 at 4, ids unchanged (profiles/r05_ab_fc2_rows.log; ER_RW_FC2 = 2 / 4 / 6,
            // read at er_create like every A/B knob of the step graph: the graph is captured with that value)
            if (half && p.B == 1 && (k.rw_fc2 == 6 || k.rw_fc2 == 4)) return ProjForm{ER_FORM_ROW, 4, k.rw_fc2, false};
            return ProjForm{ER_FORM_ROW, 4, 2, false};
        case PROJ_HEAD:
            return p.batched ? ProjForm{ER_FORM_VALU, 0, 0, false} : ProjForm{ER_FORM_ROW, 4, 1, false};
    }
    return ProjForm{};
}

// "The decode step can launch this": every proj_form result for `B` rows satisfies it, and er_k_gemv_form refuses what does not.
// The batched forms are legal at any batch (ER_FORCE_BATCHED=1 runs them at 1..4 rows); nw / rw count in the row forms only.
inline bool proj_form_legal(Proj proj, const ProjForm& f, bool half, int B) {
    if (B < 1 || f.defer != (f.form == ER_FORM_NARROW_DEFER)) return false;
    switch (f.form) {
        case ER_FORM_ROW:
            if (B > 4) return false;
            switch (proj) {
                case PROJ_QKV: return (f.nw == 4 && f.rw == 1) || (f.nw == 6 && f.rw == 1) || (f.nw == 9 && f.rw == 2);      // read_knobs: ER_NW_QKV
                case PROJ_OUT: return f.nw == 3 && f.rw == 1;
                case PROJ_FC1: return (f.nw == 4 || f.nw == 12) && f.rw == 2;                                                // ER_NW_FC1
                case PROJ_FC2: return f.nw == 4 && (f.rw == 2 || (half && B == 1 && (f.rw == 4 || f.rw == 6)));              // ER_RW_FC2
                case PROJ_HEAD: return f.nw == 4 && f.rw == 1;
            }
            return false;
        case ER_FORM_ROWS8: return proj == PROJ_OUT && B >= 5 && B <= 8;
        case ER_FORM_VALU: return true;
        case ER_FORM_MFMA: return proj != PROJ_HEAD;                                       // the lm_head stays on the VALU kernel
        case ER_FORM_MFMA_XT: return half && (proj == PROJ_QKV || proj == PROJ_FC1);       // wide tiled form
        case ER_FORM_NARROW: return half && proj == PROJ_FC2;                              // narrow + finish kernel: the last layer's fc2
        case ER_FORM_NARROW_DEFER: return half && (proj == PROJ_OUT || proj == PROJ_FC2);
    }
    return false;
}

}   // namespace er
