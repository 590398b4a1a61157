// The launch table of the decode projections (qkv, out_proj, fc1, fc2, lm_head): the group loops over batch rows and launch_proj, the
// ONLY function of the library that names a launcher with its template arguments for a decode projection.  The decode step
// (launch_kind_t) and the single-kernel entries (er_k_gemv, er_k_gemv_form and its _w8 / _w4 variants) all get here through run_proj.
// Which form a projection takes (csrc/er_decode_plan.h proj_form) and which copy of its matrix it streams (csrc/er_weight_source.h
// weight_source) are decided in host-only code; this file turns (projection, form, source) into launches and decides neither.
#pragma once
#include <hip/hip_runtime.h>

#include "er_weight_source.h"
#include "k_gemv.h"
#include "k_gemv_mfma.h"

namespace er {

constexpr int NBM = 32;   // batch rows per pass of the matrix-core decode projections (k_gemv_mfma.h)

// a with every per-row pointer advanced to batch row row0 (K = width of an input row): what a pass of the three group loops below launches with.
// The batched kernels read neither hout nor tok, and the tiled image of a group of 32 rows is K * 32 floats like its row-major form: one rule serves all.
static GemvArgs gemv_args_at(const GemvArgs& a, int row0, int K) {
    GemvArgs g = a;
    if (g.xin) g.xin += (long long)row0 * K;
    if (g.xt_out) g.xt_out = (char*)g.xt_out + (long long)row0 * a.N * 4;     // xt_entry() indexes inside a group
    if (g.hout) g.hout += (long long)row0 * K;
    if (g.tok) g.tok += row0;
    if (g.pos) g.pos += row0;
    if (g.out) g.out += (long long)row0 * a.N;
    if (g.resid) g.resid += (long long)row0 * a.N;
    if (g.q) g.q += (long long)row0 * a.hidden;
    const long long kvb = (long long)row0 * a.kv_bstride * kv_elem_bytes(a.kv_half);
    if (g.kcache) g.kcache = (char*)g.kcache + kvb;
    if (g.vcache) g.vcache = (char*)g.vcache + kvb;
    return g;
}

template <typename WT, int KS, int RW, int PRO, int EPI, int NW = ER_NWAVES>
static hipError_t gemv_groups(const GemvArgs& a, int B, int K, hipStream_t st) {
    // rows are processed in groups of up to 4 (one weight stream, 1..4 accumulators per row)
    int b = 0;
    while (b < B) {
        int nb = B - b;
        nb = nb >= 4 ? 4 : nb;
        const GemvArgs g = gemv_args_at(a, b, K);
        hipError_t e;
        if (nb == 4) e = launch_gemv<WT, KS, 4, RW, PRO, EPI, NW>(g, st);
        else if (nb == 3) e = launch_gemv<WT, KS, 3, RW, PRO, EPI, NW>(g, st);
        else if (nb == 2) e = launch_gemv<WT, KS, 2, RW, PRO, EPI, NW>(g, st);
        else e = launch_gemv<WT, KS, 1, RW, PRO, EPI, NW>(g, st);
        if (e != hipSuccess) return e;
        b += nb;
    }
    return hipSuccess;
}

// single-row GEMV with a LayerNorm / embedding prologue by waves per workgroup: 4 or 6 waves x 1 row (qkv), 4 waves x 2 rows (fc1),
// or ONE fat workgroup per CU - 9 waves x 2 rows = 4608 qkv rows / 256, 12 waves x 2 rows = 6144 fc1 rows / 256
template <typename WT, int PRO, int EPI>
static hipError_t gemv_nw(int nw, GemvArgs a, int B, int K, hipStream_t st) {
    if (nw == 6) return gemv_groups<WT, 1, 1, PRO, EPI, 6>(a, B, K, st);
    if (nw == 9) return gemv_groups<WT, 1, 2, PRO, EPI, 9>(a, B, K, st);
    if (nw == 12) return gemv_groups<WT, 1, 2, PRO, EPI, 12>(a, B, K, st);
    if (epi_qkv(EPI)) return gemv_groups<WT, 1, 1, PRO, EPI>(a, B, K, st);
    return gemv_groups<WT, 1, 2, PRO, EPI>(a, B, K, st);
}

// out_proj of 5..8 rows: ONE pass of the VALU kernel with 5..8 accumulators per weight row.  The matrix-core kernel has only 48
// row tiles for this 1536-row matrix (48 of 256 CUs: 9.3 us at B = 5 against 4.9 us for the four-row VALU launch), which left the
// aggregate rate of five rows below that of four (profiles/r03_batch_table_v2.log); same per-(row, batch row) arithmetic as every
// other path.
template <typename WT>
static hipError_t gemv_outproj_rows8(const GemvArgs& a, int B, hipStream_t st) {
    switch (B) {
        case 5: return launch_gemv<WT, 1, 5, 1, PRO_NONE, EPI_RESID, 3>(a, st);
        case 6: return launch_gemv<WT, 1, 6, 1, PRO_NONE, EPI_RESID, 3>(a, st);
        case 7: return launch_gemv<WT, 1, 7, 1, PRO_NONE, EPI_RESID, 3>(a, st);
        case 8: return launch_gemv<WT, 1, 8, 1, PRO_NONE, EPI_RESID, 3>(a, st);
    }
    return hipErrorInvalidValue;
}

// B > 4: weights streamed once per pass of up to 16 rows (gemv_batched_kernel)
constexpr int NBB = 16;
template <typename WT, int PH, int RW, int EPI>
static hipError_t gemv_batched_groups(const GemvArgs& a, int B, int K, hipStream_t st) {
    for (int b = 0; b < B; b += NBB) {
        const int nb = (B - b) < NBB ? (B - b) : NBB;
        hipError_t e = launch_gemv_batched<WT, PH, NBB, RW, EPI>(gemv_args_at(a, b, K), nb, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// XT: a.xin is the tiled image of the input (a group of 32 rows is K * 32 floats there as well, so the group offsets coincide)
struct SkPart { float* p; size_t floats; };       // the context's split-K partial block and its size
template <typename WT, int EPI, bool XT = false>
static hipError_t gemv_mfma_groups(const GemvArgs& a, int B, int K, SkPart part, hipStream_t st, bool defer_finish = false, bool narrow = false) {
    const int slices = narrow ? K / (4 * GM_KW) : K / (GM_WAVES * GM_KW);
    {   // the block was sized in er_kv_reserve for K <= 6144 (4 wide / 16 narrow slices) and, when the finish is not deferred, for ONE
        // group at a time on an in-order stream: refuse anything that would overrun it instead of writing past the end
        const size_t groups = (size_t)(B + NBM - 1) / NBM;
        const size_t need = (defer_finish ? groups : 1) * slices * NBM * (size_t)a.N;
        if (!part.p || need > part.floats) return hipErrorInvalidValue;
    }
    for (int b = 0; b < B; b += NBM) {
        const int nb = (B - b) < NBM ? (B - b) : NBM;
        // deferred: every group keeps its own partial block (prep_rows_kernel: g * 4 * 32 * K floats)
        hipError_t e = launch_gemv_mfma<WT, EPI, XT>(gemv_args_at(a, b, K), nb, K, defer_finish ? part.p + (long long)(b / NBM) * slices * NBM * a.N : part.p, st, defer_finish, narrow);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
template <int PRO>
static hipError_t prep_rows(const GemvArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL((prep_rows_kernel<PRO>), dim3(B), dim3(ER_WG), 0, st, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------ the launch table
// Projection `proj` in form `f` on the operands `a` (K = width of an input row).  The caller has pointed a.W at the copy the source names
// (WT is that copy's type) and a.xin at the tiled image for the tiled-input forms, and has run the batched forms' prologue (run_proj does all
// three); pro names the prologue FUSED into the qkv row kernel (PRO_LN, or PRO_EMBED for layer 0; fc1 and lm_head always fuse PRO_LN).
// Shapes: qkv 4608 rows = 192 VALU workgroups x 24 (one round) or 144 matrix-core tiles of 32; fc1 6144 rows = 256 x 24 or 192 tiles;
// fc2 48 tiles x 4 (narrow: 16) K-ranges.  The XT kernels exist for fp16 weights only: their forms are compiled out for float.
//
// Which copy of its matrix a projection streams is decided in csrc/er_weight_source.h (weight_source), host-only like the form; run_proj
// maps the source to the kernel's weight type and nothing here asks a rule.
//
// fp8 context (WSRC_BYTES: the byte block of the matrix, k_gemv.h w8_scales; WSRC_TILED_BYTES: its tiled copy, er_w8_tile_map.h): a row
// form runs the same (waves x rows) shape of the byte kernel, a matrix-core form the same form of gemv_mfma_kernel<w8_t>; the VALU batched
// kernel, the eight-row out_proj and the lm_head run the fp16 copy as in fast mode.  The byte type has the fp16 row shapes and the four
// matrix-core forms, nothing else.
//
// kv8 context (a.kv_half == 2: the KV cache holds e4m3 bytes): every QKV form - row, VALU, both matrix-core forms, with fp16 or byte
// weights - is launched with EPI_QKV8, the epilogue that encodes (k_gemv.h); nothing else depends on the cache type.
//
// fp4 context (WSRC_QUADS: the quad-interleaved nibble copy of the matrix, er_w4_map.h): a row form runs the nibble kernel in the
// projection's OWN nibble shape - a wave owns whole row quads, so the (waves x rows) of the fp16 form do not carry over:
//     qkv  4 waves x 4 rows        = 288 workgroups for 4608 rows
//     fc1  6 waves x 4 rows        = 256 workgroups for 6144 rows
//     fc2  4 K-slices x 4 rows     = 384 workgroups for 1536 rows
// (qkv with 6 waves and fc1 with 4 were measured too and lost: DESIGN.md section 4).  Both keep the four-wave prologue (gemv_kernel: PW),
// so the LayerNorm'd input - and with fp16's lane -> element map, fmaf chain and butterfly every output - is the fp16 form's bit for
// bit.  A matrix-core form (ER_FORM_MFMA, _MFMA_XT, _NARROW, _NARROW_DEFER) of qkv, out_proj, fc1 or fc2 on WSRC_TILED_NIBBLES runs the
// same form of gemv_mfma_kernel<w4_t> on the tiled nibble copy (er_w4_tile_map.h).  The single-row out_proj (the fused merge launch
// included), the lm_head, the VALU batched kernel, the eight-row out_proj and the fused sparse MLP have no nibble form.

// the nibble row form of `proj` on the streamed copy a.W; a.kv_half names the cache type
static hipError_t launch_proj_w4(Proj proj, int pro, const GemvArgs& a, int B, int K, hipStream_t st) {
    if (!w4_has_row_form(proj) || B < 1 || B > 4 || !w4map::shape_ok(a.N, K)) return hipErrorInvalidValue;
    switch (proj) {
        case PROJ_QKV:
            if (a.kv_half == 2) {
                if (pro == PRO_EMBED) return gemv_groups<w4_t, 1, 4, PRO_EMBED, EPI_QKV8, 4>(a, B, K, st);
                return gemv_groups<w4_t, 1, 4, PRO_LN, EPI_QKV8, 4>(a, B, K, st);
            }
            if (a.kv_half != 1) return hipErrorInvalidValue;      // fp32 caches go with fp32 weights
            if (pro == PRO_EMBED) return gemv_groups<w4_t, 1, 4, PRO_EMBED, EPI_QKV, 4>(a, B, K, st);
            return gemv_groups<w4_t, 1, 4, PRO_LN, EPI_QKV, 4>(a, B, K, st);
        case PROJ_FC1: return gemv_groups<w4_t, 1, 4, PRO_LN, EPI_RELU, 6>(a, B, K, st);
        case PROJ_FC2: return gemv_groups<w4_t, 4, 4, PRO_NONE, EPI_RESID>(a, B, K, st);
        default: break;
    }
    return hipErrorInvalidValue;
}

template <typename WT>
static hipError_t launch_proj(Proj proj, const ProjForm& f, int pro, const GemvArgs& a, int B, int K, SkPart sk, hipStream_t st) {
    constexpr bool W4 = WTraits<WT>::NIBBLES, W8 = WTraits<WT>::E4M3 || W4, HALF = sizeof(WT) <= 2;      // W8: a packed type (bytes or nibbles) - matrix-core forms only among the batched ones
    if (W8 && proj == PROJ_HEAD) return hipErrorInvalidValue;      // the lm_head is not quantised
    if (W4 && !form_mfma(f.form)) return hipErrorInvalidValue;     // the tiled nibble copy has the four matrix-core forms, nothing else (the row forms: launch_proj_w4)
    if (W4 && proj == PROJ_QKV && a.kv_half == 0) return hipErrorInvalidValue;      // fp4 weights go with an fp16 or a byte cache
    if constexpr (!W4) switch (f.form) {
        case ER_FORM_ROW:
            switch (proj) {
                case PROJ_QKV:
                    if (a.kv_half == 2) {      // byte cache: the epilogue that encodes (fp16 and byte weights only)
                        if constexpr (HALF) {
                            if (pro == PRO_EMBED) return gemv_nw<WT, PRO_EMBED, EPI_QKV8>(f.nw, a, B, K, st);
                            return gemv_nw<WT, PRO_LN, EPI_QKV8>(f.nw, a, B, K, st);
                        }
                        break;
                    }
                    if (pro == PRO_EMBED) return gemv_nw<WT, PRO_EMBED, EPI_QKV>(f.nw, a, B, K, st);
                    return gemv_nw<WT, PRO_LN, EPI_QKV>(f.nw, a, B, K, st);
                case PROJ_OUT:
                    if (f.nw == 3) return gemv_groups<WT, 1, 1, PRO_NONE, EPI_RESID, 3>(a, B, K, st);      // the step
                    if constexpr (!HALF) {
                        if (f.nw == ER_NWAVES) return gemv_groups<WT, 1, 1, PRO_NONE, EPI_RESID>(a, B, K, st);   // er_k_gemv (the prefill tail runs the same kernel: linear_tail)
                    }
                    break;
                case PROJ_FC1: return gemv_nw<WT, PRO_LN, EPI_RELU>(f.nw, a, B, K, st);
                case PROJ_FC2:
                    if constexpr (HALF) {
                        if (f.rw == 6 || f.rw == 4) {
                            if (B != 1) break;
                            return f.rw == 6 ? launch_gemv<WT, 4, 1, 6, PRO_NONE, EPI_RESID>(a, st) : launch_gemv<WT, 4, 1, 4, PRO_NONE, EPI_RESID>(a, st);
                        }
                    }
                    return gemv_groups<WT, 4, 2, PRO_NONE, EPI_RESID>(a, B, K, st);
                case PROJ_HEAD:
                    if constexpr (!W8) return gemv_groups<WT, 1, 1, PRO_LN, EPI_STORE>(a, B, K, st);
                    break;
            }
            break;
        default: break;
    }
    if constexpr (HALF) {
        if (proj == PROJ_QKV && a.kv_half == 2) switch (f.form) {      // the batched QKV forms into a byte cache
            case ER_FORM_VALU:
                if constexpr (!W8) return gemv_batched_groups<WT, 1, 3, EPI_QKV8>(a, B, K, st);
                return hipErrorInvalidValue;
            case ER_FORM_MFMA: return gemv_mfma_groups<WT, EPI_QKV8>(a, B, K, sk, st);
            case ER_FORM_MFMA_XT: return gemv_mfma_groups<WT, EPI_QKV8, true>(a, B, K, sk, st);
            default: return hipErrorInvalidValue;
        }
    }
    if (proj == PROJ_QKV && a.kv_half == 2) return hipErrorInvalidValue;      // fp32 weights keep an fp32 cache
    switch (f.form) {      // the batched forms (the bytes: the matrix-core forms only)
        case ER_FORM_ROW: break;
        case ER_FORM_ROWS8:
            if constexpr (!W8) {
                if (proj == PROJ_OUT) return gemv_outproj_rows8<WT>(a, B, st);
            }
            break;
        case ER_FORM_VALU:
            if constexpr (!W8) switch (proj) {
                case PROJ_QKV: return gemv_batched_groups<WT, 1, 3, EPI_QKV>(a, B, K, st);
                case PROJ_OUT: return gemv_batched_groups<WT, 1, 1, EPI_RESID>(a, B, K, st);
                case PROJ_FC1: return gemv_batched_groups<WT, 1, 3, EPI_RELU>(a, B, K, st);
                case PROJ_FC2: return gemv_batched_groups<WT, 4, 1, EPI_RESID>(a, B, K, st);
                case PROJ_HEAD: return gemv_batched_groups<WT, 1, 1, EPI_STORE>(a, B, K, st);
            }
            break;
        case ER_FORM_MFMA:
            switch (proj) {
                case PROJ_QKV: return gemv_mfma_groups<WT, EPI_QKV>(a, B, K, sk, st);
                case PROJ_FC1: return gemv_mfma_groups<WT, EPI_RELU>(a, B, K, sk, st);
                case PROJ_OUT:
                case PROJ_FC2: return gemv_mfma_groups<WT, EPI_RESID>(a, B, K, sk, st);
                case PROJ_HEAD: break;
            }
            break;
        case ER_FORM_MFMA_XT:
            if constexpr (HALF) {
                if (proj == PROJ_QKV) return gemv_mfma_groups<WT, EPI_QKV, true>(a, B, K, sk, st);
                if (proj == PROJ_FC1) return gemv_mfma_groups<WT, EPI_RELU, true>(a, B, K, sk, st);      // writes a.xt_out, the image fc2 reads
            }
            break;
        case ER_FORM_NARROW:
        case ER_FORM_NARROW_DEFER:
            if constexpr (HALF) {
                if (proj == PROJ_FC2 || (proj == PROJ_OUT && f.defer)) return gemv_mfma_groups<WT, EPI_RESID, true>(a, B, K, sk, st, f.defer, true);
            }
            break;
    }
    return hipErrorInvalidValue;
}

// A split-K finish that the previous producer deferred to this prologue launch: rows = ((p_0 + .. + p_{slices-1}) + bias) + resid.
struct SkRead { const float* part = nullptr; const float* bias = nullptr; const float* resid = nullptr; int slices = 0; };

// The batched forms' prologue: LayerNorm (or token + position embedding) of B rows into a.hout by its own launch, optionally of the
// rows a deferred split-K finish yields (rd.part) and optionally also into the tiled image `image`; the projection then reads a.hout.
static hipError_t launch_prologue(int pro, GemvArgs& a, int B, const SkRead& rd, void* image, hipStream_t st) {
    a.xt_out = image;
    if (rd.part) { a.sk_part = rd.part; a.sk_bias = rd.bias; a.sk_resid = rd.resid; a.sk_batch = B; a.sk_slices = rd.slices; }
    const hipError_t e = pro == PRO_EMBED ? prep_rows<PRO_EMBED>(a, B, st) : prep_rows<PRO_LN>(a, B, st);
    a.xin = a.hout;
    a.xt_out = nullptr;
    a.sk_part = nullptr;
    return e;
}

// What a projection launches with beside the GemvArgs of its row-major form (`a` of run_proj: row-major input; a.W is not read)
struct ProjIo {
    int pro = PRO_NONE;               // PRO_LN / PRO_EMBED: fused into the row kernels, launch_prologue in front of the batched forms
    SkRead rd;                        // ... which then also finishes the previous producer's partials
    void* pro_image = nullptr;        // ... and writes the tiled image of its rows
    const void* x_image = nullptr;    // the input as the tiled-input forms read it
    void* out_image = nullptr;        // fc1, ER_FORM_MFMA_XT: the tiled image of the output
    WSrc src = WSRC_PLAIN;            // the copy of the matrix this launch streams (weight_source; the unit entries: the caller's word) ...
    const void* w = nullptr;          // ... and where it is; null while that copy does not match the loaded weights: the launch fails
};

// (projection, form, source) -> launches: the prologue launch of a batched form, the operands the form reads, and launch_proj in the
// weight type of the source - WT (float or _Float16) for the plain and the tiled copy, w8_t for the bytes, w4_t for the nibbles.
template <typename WT>
static hipError_t run_proj(Proj proj, const ProjForm& f, const ProjIo& io, GemvArgs a, int B, int K, SkPart sk, hipStream_t st) {
    // the copy the source names is not there: an error in front of every launch, never the fp16 copy quietly
    if (!io.w || io.src == WSRC_KMAJOR || wsrc_tiled(io.src) != form_mfma(f.form)) return hipErrorInvalidValue;
    if ((wsrc_bytes(io.src) || wsrc_nibbles(io.src)) && sizeof(WT) != 2) return hipErrorInvalidValue;      // the packed copies stand in for fp16
    if (io.src == WSRC_TILED_NIBBLES && !w4t::shape_ok(a.N, K)) return hipErrorInvalidValue;
    if (io.pro != PRO_NONE && form_batched(f.form)) {
        const hipError_t e = launch_prologue(io.pro, a, B, io.rd, io.pro_image, st);
        if (e != hipSuccess) return e;
    }
    a.W = io.w;
    if (form_tiled_in(f.form)) a.xin = (const float*)io.x_image;
    if (f.form == ER_FORM_MFMA_XT && proj == PROJ_FC1) a.xt_out = io.out_image;
    switch (io.src) {
        case WSRC_QUADS: return f.form == ER_FORM_ROW ? launch_proj_w4(proj, io.pro, a, B, K, st) : hipErrorInvalidValue;
        case WSRC_TILED_NIBBLES: return launch_proj<w4_t>(proj, f, io.pro, a, B, K, sk, st);
        case WSRC_BYTES: return f.form == ER_FORM_ROW ? launch_proj<w8_t>(proj, f, io.pro, a, B, K, sk, st) : hipErrorInvalidValue;
        case WSRC_TILED_BYTES: return launch_proj<w8_t>(proj, f, io.pro, a, B, K, sk, st);
        default: return launch_proj<WT>(proj, f, io.pro, a, B, K, sk, st);
    }
}

}   // namespace er
