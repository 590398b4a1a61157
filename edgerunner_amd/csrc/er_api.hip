// C-ABI implementation (see include/edgerunner_hip.h): context, checkpoint loading,
// KV cache, prefill, point encoder, device-side generation loop (hipGraph replay).
// Single translation unit: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC.
#include "../../include/edgerunner_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "er_common.h"
#include "k_attn_lanes.h"
#include "k_attn_decode.h"
#include "k_attn_shared.h"
#include "k_attn_shared_mfma.h"
#include "k_attn_extend.h"
#include "k_kv_fork.h"
#include "k_outproj_merge.h"
#include "k_flash_attn_f16s.h"
#include "k_gemm.h"
#include "k_gemm_stream.h"
#include "k_gemv.h"
#include "k_gemv_mfma.h"
#include "k_head.h"
#include "k_rowops.h"
#include "k_dit.h"
#include "k_score.h"
#include "k_flash_attn.h"
#include "k_flash_attn_f32.h"
#include "k_fps.h"
#include "k_fidelity.h"
#include "meto_decode.h"
#include "meto_encode.h"
#include "er_queue_host.h"
#include "er_decode_plan.h"
#include "er_extend_plan.h"
#include "er_decode_proj.h"
#include "k_mlp_sparse.h"

using namespace er;

// ------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ER_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)
#define ERCHK(expr)                 \
    do {                            \
        int r_ = (expr);            \
        if (r_ < 0) return r_;      \
    } while (0)

// ------------------------------------------------------------------------------------ context
struct LayerW {
    // fast mode (fp16 storage): *_h hold the streamed fp16 matrices; the fp32 copies then hold the SAME
    // fp16-rounded values (used by the prefill GEMMs), so prefill and decode see one model
    _Float16 *wqkv_h = nullptr, *wo_h = nullptr, *w1_h = nullptr, *w2_h = nullptr;
    // fp8 mode (er_w8.h): the byte blocks of the same four matrices (e4m3 [N][K], then 2^e per row); *_h and the fp32 copies then hold
    // the dequantised values
    unsigned char *wqkv_q = nullptr, *wo_q = nullptr, *w1_q = nullptr, *w2_q = nullptr;
    // fp4 mode (er_w4.h): the canonical MXFP4 blocks of the same four matrices (nibble bytes [N][K / 2], then e8m0 bytes [N][K / 32]) - *_h and
    // the fp32 copies hold the dequantised values
    unsigned char *wqkv_q4 = nullptr, *wo_q4 = nullptr, *w1_q4 = nullptr, *w2_q4 = nullptr;
    // What the context derives from them, by (projection, source): the tiled copies of the matrix-core kernels (k_gemv_mfma.h, er_w8_tile_map.h,
    // er_w4_tile_map.h), the quad-interleaved nibble copies (er_w4_map.h) and fc2 k-major (k_mlp_sparse.h).  ensure_weight_copies makes the
    // ones a reserved plan streams, er_ctx::copy_made says which match the loaded weights, weight_ptr hands them out.
    void* copy[4][WSRC_COUNT] = {};
    float *wqkv = nullptr, *bqkv = nullptr;   // fused [3*hidden][hidden] in q,k,v order
    float *wo = nullptr, *bo = nullptr, *ln1w = nullptr, *ln1b = nullptr;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *ln2w = nullptr, *ln2b = nullptr;
};

#include "er_devbuf.h"
#include "er_weights.h"

// PointEncoderEmbed (core/transformer/point.py:172-206) or, with mode ER_PE_DOWNSAMPLE, PointEncoder (:129-169): weights, shape and
// scratch.  Embedded in er_ctx (cond_mode POINT) and, after er_dit_attach_point_encoder, in er_dit_ctx; the same helpers
// (pe_attach / pe_latent / point_latent_chunk) serve both.
struct PointEnc {
    int PH = 0, heads = 0, Lq = 0, LD = 0, freq = 0;     // point_hidden_dim, point_num_heads, latent size / dim, point_freq_dim
    int mode = ER_PE_EMBED;  // ER_PE_DOWNSAMPLE: the queries are the point embeddings of a farthest-point subsample (no query_embed)
    float eps = 1e-5f;
    float *query = nullptr, *basis = nullptr, *mlp_w = nullptr, *mlp_b = nullptr, *ln_w = nullptr, *ln_b = nullptr;
    float *ca_ln1_w = nullptr, *ca_ln1_b = nullptr, *ca_ln2_w = nullptr, *ca_ln2_b = nullptr;
    float *ca_q_w = nullptr, *ca_q_b = nullptr, *ca_k_w = nullptr, *ca_k_b = nullptr, *ca_v_w = nullptr, *ca_v_b = nullptr,
          *ca_o_w = nullptr, *ca_o_b = nullptr;
    float *ff0_w = nullptr, *ff0_b = nullptr, *ff2_w = nullptr, *ff2_b = nullptr, *lin_w = nullptr, *lin_b = nullptr;
    int kpad = 0;            // padded input width of point_embed.mlp (51 -> 64), set by pe_attach
    DevBuf<float> a0, x, k, v, qln, q, sc, att, l, ln, u, g, lat;   // scratch of point_latent_chunk; lat = the latent mean [nb][Lq][LD]
    DevBuf<float> q0, fdist;                              // downsample mode: gathered query rows [nb][Lq][PH], FPS distances (large N)
    DevBuf<int32_t> fidx;                                 // ... and the FPS indices [nb][Lq]
};

// The generation state of b rows is one block of ints: seven per-row arrays, then the two scalars.
static size_t gen_state_ints(size_t b) { return 7 * b + 8; }
static GenState gen_state_carve(int* sb, size_t b) {
    GenState s{};
    s.tok = sb; s.pos = sb + b; s.counter = sb + 2 * b; s.ngen = sb + 3 * b; s.unfinished = sb + 4 * b;
    s.eos_step = sb + 5 * b; s.base_pos = sb + 6 * b; s.n_unfinished = sb + 7 * b; s.error = sb + 7 * b + 1;
    return s;
}

// What the sampling heads read of a call: its decode parameters (top_k as the call resolved it, max_new as the caller counts
// steps), the model's token ids and the seed as the two Philox key words.
static DecodeParamsDev decode_params_dev(const er_decode_params& p, int top_k, int max_new, int eos, int pad, int vocab) {
    DecodeParamsDev dp{};
    dp.mode = p.mode; dp.top_k = top_k; dp.grammar = p.grammar; dp.max_new = max_new; dp.min_new = p.min_new_tokens;
    dp.eos = eos; dp.pad = pad; dp.vocab = vocab;
    dp.seed_lo = (unsigned int)(p.seed & 0xffffffffu); dp.seed_hi = (unsigned int)(p.seed >> 32);
    return dp;
}

// K-range partials per row that a 4-wave split-K launch leaves to a LATER launch: out_proj 1536 / 384, fc2 6144 / 384 (4 is also the most
// a 16-wave launch leaves to its own finish: 6144 / 1536).  KvMem::skpart is sized from them; the launches that write and read pass them.
constexpr int SK_SLICES_OUTPROJ = 4, SK_SLICES_FC2 = 16;
static_assert(1536 / (4 * GM_KW) == SK_SLICES_OUTPROJ && 6144 / (4 * GM_KW) == SK_SLICES_FC2 && 6144 / (GM_WAVES * GM_KW) == SK_SLICES_OUTPROJ, "k_gemv_mfma.h");

// Everything er_kv_reserve allocates for one (batch, Lcap), with the plan of that shape.  It lives and dies as a whole: a new shape replaces
// the object, a reserve that fails half way never installs its own, er_destroy drops it - and the captured step goes with the buffers it points into.
struct KvMem {
    DecodePlan plan;
    DevBuf<char> kc, vc;          // KV cache [layers][B][H][Lcap][D], fp32 or fp16 (fast)
    DevBuf<float> ypre, hbuf, ypre1, h1buf, qbuf, abuf, fbuf, logits;   // decode workspace ([B][...])
    DevBuf<float> part, part_ml;  // attention partials; version 3: {m, l} of the partials
    DevBuf<float> mlp_part;       // fused single-row MLP: the 256 chain vectors of one layer ([256][hidden]), rewritten by every launch
    DevBuf<int> mlp_nnz;          // ... and the live neurons per (layer, workgroup) of the last step ([layers][256])
    DevBuf<float> skpart;         // split-K partials of the batched projections (gemv_mfma_groups checks launches against skpart.n)
    // fast-mode batches on the matrix cores: activations in the tiled hi | lo operand layout (k_gemv.h xt_entry), one image per producer
    DevBuf<char> xt_h, xt_att, xt_f;     // LayerNorm rows (qkv / fc1 input), attention output, fc1 output
    DevBuf<int> state_block;      // backing store of st
    GenState st{};
    DevBuf<DecodeParamsDev> d_params;
    DevBuf<int> d_ids_tmp;
    DevBuf<unsigned int> d_row_stream;   // [B] Philox stream id per row (identity until er_set_row_streams)
    DevBuf<int> d_row_budget;     // [B] token budget per row: INT_MAX (= er_decode's max_new_tokens decides) outside the queue mode
    DevBuf<long long> d_out_ids;  // [B][Lcap] generated ids (graph writes here; copied to the caller at the end)
    hipGraphExec_t step_exec = nullptr;  // hipGraph of one step
    // the head with controls (er_set_sampling): which head the current generation ends its step in, that step's own capture, the device
    // copy of the controls and the log-prob tables beside d_out_ids (allocated when log-probs are first asked for)
    bool head_ctl = false, lp_on = false, lp_valid = false, ctl_exec_lp = false;
    // A generation that keeps log-probs runs a one-row exact plan as the kernels that 2 .. 4 rows run: split attention + merge + plain out_proj
    // in place of version 3, the row fc1 / fc2 in place of the fused MLP.  Those one-row kernels associate their sums differently, their logits
    // differ in the last place, and a job's log-probs are promised to be the same bits whether it runs alone or in a queue of a few slots.
    // The stored plan (er_ctx_plan) and the default step do not change.
    bool row_class = false;
    hipGraphExec_t step_exec_ctl = nullptr;   // captured with the log-prob pointers of the time (ctl_exec_lp: they were set)
    DevBuf<HeadCtlDev> d_ctl;
    DevBuf<float> d_lp_model, d_lp_policy;    // [B][Lcap]
    // prefix groups (er_set_prefix_groups; prefix_len == 0: none): the leader of every row, and for the prefix pass the rows of every group,
    // group after group with the leader first, behind the groups' offsets
    std::vector<int> grp_leader;
    int prefix_len = 0, n_groups = 0;
    // the past er_prefill_extend may keep: positions [0, valid_prefix) were written for ALL rows by the last er_prefill / er_prefill_fork /
    // er_score / er_prefill_extend on this reservation (0: by none, or that pass failed); it counts while have_hidden holds
    int valid_prefix = 0;
    DevBuf<int> grp_rows, grp_off, grp_leader_dev, grp_followers, grp_first;
    KvMem() = default;
    KvMem(const KvMem&) = delete;
    KvMem& operator=(const KvMem&) = delete;
    void drop_steps() {
        if (step_exec) hipGraphExecDestroy(step_exec);
        if (step_exec_ctl) hipGraphExecDestroy(step_exec_ctl);
        step_exec = step_exec_ctl = nullptr;
    }
    ~KvMem() { drop_steps(); }
};

struct er_ctx {
    er_config cfg{};
    int device = 0;
    int D = 0;               // head_dim
    hipStream_t own_stream = nullptr;
    // weights
    std::vector<LayerW> layers;
    float *embd = nullptr, *posemb = nullptr, *lm_head = nullptr, *embed_num_face = nullptr;
    _Float16* lm_head_h = nullptr;
    bool fast = false;       // fp16 weights + fp16 KV cache, fp32 accumulate
    bool kv8 = false;        // kv8 mode: fast (or fp8), with the KV cache stored as e4m3 bytes without a scale (er_w8.h kv8_encode)
    int kv_type = 0;         // the cache type as the kernels' kv_half argument takes it: 0 = fp32, 1 = fp16, 2 = e4m3 bytes
    bool w8 = false;         // fp8 mode: fast, with the six decoder matrices per layer quantised by row; the row forms and (w8_streams_batched) the matrix-core forms of the step stream the bytes
    bool w4 = false;         // fp4 mode: fast, with the six decoder matrices per layer quantised by blocks of 32 (MXFP4); the row forms w4_streams names and the matrix-core forms w4_streams_batched names stream the nibbles
    float *proj_w = nullptr, *proj_b = nullptr, *normc_w = nullptr, *normc_b = nullptr;
    PointEnc pe;             // point encoder (cond_mode POINT)
    WeightTable w;           // every checkpoint key (register_weights)
    std::unique_ptr<KvMem> kv = std::make_unique<KvMem>();   // KV cache + decode workspace + plan of the reserved shape (kv->plan.B == 0: none); never null, er_kv_reserve swaps in a new one
    int kv_esz = 4;
    int* h_pinned = nullptr;      // small pinned host buffer
    int base_pos = 0;             // prefill length of the current generation
    bool have_hidden = false;     // ypre holds a valid last-position state
    DecodeKnobs knobs;        // environment of er_create
    er_sampling samp{1.0f, 1.0f, 0, 0, 0};   // er_set_sampling: sticky, kept across er_kv_reserve
    bool copy_made[4][WSRC_COUNT] = {};   // LayerW::copy[proj][source] of every layer has been made of the weights as loaded now (any reload clears the table)
    void* zero_row = nullptr;  // hidden zeros (fp32 size): what the fused MLP reads in place of a dead neuron's row
    int prof_len = 0;         // > 0: attention kernels run at this fixed length (er_profile_decode_kernels_at)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_decode_ms = 0.f;
    // scratch for prefill / encoder: grow-only, freed with the context
    DevBuf<_Float16> p_hi, p_lo;   // fast-mode prefill: hi / lo fp16 halves of the activation a Linear is about to read (LDS-DMA GEMM, split form)
    DevBuf<float> p_h, p_q, p_a, p_y, p_f, p_qkv, p_ap, p_aml, p_kx, e_tmp;   // p_kx: er_prefill_extend's gathered K | V rows (flash route, fast mode)
    DevBuf<int> e_ids;             // er_embed_tokens: the ids on the device
    DevBuf<float> s_lg;            // er_score: logits of every position when the caller passes no buffer for them
    // queue mode (er_queue_*): the host's view of the rows, the staging of an admission and of a look at the rows
    erq::QueueHost q;
    DevBuf<int> q_stage, q_look;   // [2 n_rows] stream ids | budgets of an admission; [3 B + 1] ngen | unfinished | eos_step | error
    int* q_pinned = nullptr;       // host image of q_look
};

constexpr int ER_MAX_BATCH = 1023;   // h_pinned holds B ints + one flag

template <typename Ctx>      // er_ctx, er_dit_ctx
static hipStream_t pick(Ctx* c, void* s) { return s ? (hipStream_t)s : c->own_stream; }

static int env_int(const char* name, int dflt) { const char* v = getenv(name); return (v && v[0]) ? atoi(v) : dflt; }
static bool env_is(const char* name, char ch) { const char* v = getenv(name); return v && v[0] == ch; }

// the knobs a context keeps for its lifetime (er_create; er_plan_decode evaluates the same rules at call time)
static DecodeKnobs read_knobs(bool fast) {
    DecodeKnobs k;
    k.use_graph = !env_is("ER_NO_GRAPH", '1');
    // one fat workgroup per CU (qkv 9 waves x 2 rows, fc1 12 waves x 2 rows) pays with fp16 weights only: the LayerNorm prologue and
    // its 18 KB of x / affine reads are then once per CU instead of three times (profiles/r03_fat_workgroups.log: fp16 +2.7 %, fp32 +-0)
    k.nw_qkv = env_int("ER_NW_QKV", fast ? 9 : 6);
    if (k.nw_qkv != 4 && k.nw_qkv != 9) k.nw_qkv = 6;
    k.nw_fc1 = env_int("ER_NW_FC1", fast ? 12 : 4) == 12 ? 12 : 4;
    k.prefill_attn_f16s = env_int("ER_PREFILL_ATTN_F16S", -1);
    if (k.prefill_attn_f16s != 0 && k.prefill_attn_f16s != 1) k.prefill_attn_f16s = -1;
    k.attn_v_batched = env_int("ER_ATTN_V_BATCHED", 0);
    if (k.attn_v_batched != 1 && k.attn_v_batched != 3) k.attn_v_batched = 0;
    k.decode_v = env_int("ER_DECODE_V", 3) == 2 ? 2 : 3;
    const char* rw = getenv("ER_RW_FC2");
    k.rw_fc2 = rw ? atoi(rw) : 6;
    if (fast && k.rw_fc2 != 2 && k.rw_fc2 != 4 && k.rw_fc2 != 6) fprintf(stderr, "[edgerunner_hip] ER_RW_FC2=%s is not 2 / 4 / 6: using 2 rows per fc2 workgroup\n", rw);
    // exact mode: on (1076 -> 1102 tok/s, profiles/mlp_sparse_bench.log); fast mode: off - fewer bytes per neuron row, and the pair
    // of launches lost its A/B (1542 -> 1501 tok/s decode, profiles/mlp_sparse_ab_decode.log)
    k.mlp_v = env_int("ER_MLP_V", fast ? 0 : 1);
    if (k.mlp_v != 1) k.mlp_v = 0;
    const char* pp = getenv("ER_PREFIX_PASS");      // valu | mfma; er_create keeps "mfma" for an fp16 cache only (er_set_prefix_pass)
    k.prefix_pass = (pp && !strcmp(pp, "mfma")) ? ER_PREFIX_PASS_MFMA : ER_PREFIX_PASS_VALU;
    k.w8_batched = env_is("ER_W8_BATCHED", '0') ? 0 : env_is("ER_W8_BATCHED", '1') ? 1 : -1;
    k.w4_rows = env_is("ER_W4_ROWS", '0') ? 0 : env_is("ER_W4_ROWS", '1') ? 1 : -1;
    k.w4_batched = env_is("ER_W4_BATCHED", '0') ? 0 : env_is("ER_W4_BATCHED", '1') ? 1 : -1;
    return k;
}

static ReserveKnobs read_reserve_knobs() { return {env_is("ER_FORCE_BATCHED", '1'), env_is("ER_BATCHED_VALU", '1'), !env_is("ER_XT", '0')}; }

extern "C" int er_abi_version(void) { return ER_ABI_VERSION; }
extern "C" const char* er_last_error(void) { return g_err; }

static const char* kKindNames[ER_NUM_KERNEL_KINDS] = {"qkv_gemv", "attn_decode", "attn_combine", "out_proj_gemv",
                                                      "fc1_gemv", "fc2_gemv", "lm_head_gemv", "sample_head"};
extern "C" const char* er_kernel_kind_name(int k) { return (k >= 0 && k < ER_NUM_KERNEL_KINDS) ? kKindNames[k] : "?"; }

// The encoder's point_encoder.* keys for `mode` (downsample checkpoints have no query_embed) into t, plain fp32 in every precision:
// at er_create / er_dit_attach_point_encoder and on a mode change, which must come before the first tensor whose key starts with
// `before` ("" = any key).
static int pe_attach(WeightTable& t, PointEnc& p, int mode, const char* who, const char* before) {
    if (mode != ER_PE_EMBED && mode != ER_PE_DOWNSAMPLE)
        return fail(ER_ERR_INVALID, "%s: %d is neither ER_PE_EMBED nor ER_PE_DOWNSAMPLE", who, mode);
    for (auto& kv : t.keys)
        if (kv.second.loaded && kv.first.rfind(before, 0) == 0)
            return fail(ER_ERR_INVALID, "%s: call it before any '%s*' tensor is loaded", who, before);
    const size_t PH = p.PH, kin = 2 * p.freq + 3;
    p.mode = mode;
    p.kpad = (int)((kin + 15) / 16 * 16);   // so that the point_embed.mlp GEMM's K is a multiple of 16
    const std::string pe = "point_encoder.";
    if (mode == ER_PE_EMBED) t.add(pe + "query_embed", &p.query, (size_t)p.Lq * PH);
    else t.keys.erase(pe + "query_embed");
    t.add(pe + "point_embed.basis", &p.basis, (size_t)3 * p.freq);
    t.lin(pe + "point_embed.mlp", &p.mlp_w, &p.mlp_b, PH, kin).pad(kin, p.kpad);
    t.lin(pe + "ln", &p.ln_w, &p.ln_b, PH, 1);
    t.lin(pe + "cross_att.ln1", &p.ca_ln1_w, &p.ca_ln1_b, PH, 1);
    t.lin(pe + "cross_att.ln2", &p.ca_ln2_w, &p.ca_ln2_b, PH, 1);
    t.lin(pe + "cross_att.att.q_proj", &p.ca_q_w, &p.ca_q_b, PH, PH);
    t.lin(pe + "cross_att.att.k_proj", &p.ca_k_w, &p.ca_k_b, PH, PH);
    t.lin(pe + "cross_att.att.v_proj", &p.ca_v_w, &p.ca_v_b, PH, PH);
    t.lin(pe + "cross_att.att.out_proj", &p.ca_o_w, &p.ca_o_b, PH, PH);
    t.lin(pe + "cross_att.mlp.net.0", &p.ff0_w, &p.ff0_b, 8 * PH, PH);
    t.lin(pe + "cross_att.mlp.net.2", &p.ff2_w, &p.ff2_b, PH, 4 * PH);
    t.lin(pe + "linear", &p.lin_w, &p.lin_b, p.LD, PH);
    return 0;
}

// every checkpoint key of the decoder context; fp16 mode keeps an fp16 copy of the streamed matrices
static void register_weights(er_ctx* c) {
    WeightTable& t = c->w;
    const er_config& g = c->cfg;
    const size_t H = g.hidden_dim, I = g.intermediate_dim, V = g.vocab_size;
    t.fp16 = c->fast;
    t.w8 = c->w8;
    t.w4 = c->w4;
    if (g.cond_mode == ER_COND_POINT) pe_attach(t, c->pe, ER_PE_EMBED, "er_create", "");
    if (g.cond_mode != ER_COND_NONE) {
        t.lin("proj_cond", &c->proj_w, &c->proj_b, H, g.point_latent_dim);
        t.lin("norm_cond", &c->normc_w, &c->normc_b, H, 1);
    }
    if (g.num_face_buckets > 0) t.add("embed_num_face.weight", &c->embed_num_face, (size_t)g.num_face_buckets * H);
    t.add("mesh_decoder.model.embd.weight", &c->embd, V * H);
    t.add("mesh_decoder.model.embed_positions.weight", &c->posemb, (size_t)g.max_positions * H);
    for (int i = 0; i < g.num_layers; ++i) {
        LayerW& L = c->layers[i];
        const std::string p = "mesh_decoder.model.layers." + std::to_string(i) + ".";
        const char* qkv[3] = {"q_proj", "k_proj", "v_proj"};     // fused [3 H][H] (+ bias [3 H]) in q, k, v order
        for (size_t j = 0; j < 3; ++j) {
            const std::string q = p + "self_attn." + qkv[j];
            t.add(q + ".weight", &L.wqkv, H * H).slice(3 * H * H, j * H * H).half(&L.wqkv_h).rows8(&L.wqkv_q, H).blocks4(&L.wqkv_q4, H);
            t.add(q + ".bias", &L.bqkv, H).slice(3 * H, j * H);
        }
        t.lin(p + "self_attn.out_proj", &L.wo, &L.bo, H, H).half(&L.wo_h).rows8(&L.wo_q, H).blocks4(&L.wo_q4, H);
        t.lin(p + "self_attn_layer_norm", &L.ln1w, &L.ln1b, H, 1);
        t.lin(p + "fc1", &L.w1, &L.b1, I, H).half(&L.w1_h).rows8(&L.w1_q, H).blocks4(&L.w1_q4, H);
        t.lin(p + "fc2", &L.w2, &L.b2, H, I).half(&L.w2_h).rows8(&L.w2_q, I).blocks4(&L.w2_q4, I);
        t.lin(p + "final_layer_norm", &L.ln2w, &L.ln2b, H, 1);
    }
    t.add("mesh_decoder.lm_head.weight", &c->lm_head, V * H).half(&c->lm_head_h);
}

extern "C" int er_create(const er_config* cfg, int device, er_ctx** out) {
    if (!cfg || !out) return fail(ER_ERR_INVALID, "er_create: null argument");
    if (cfg->hidden_dim != 1536 || cfg->intermediate_dim != 6144)
        return fail(ER_ERR_UNSUPPORTED, "this build streams hidden_dim=1536 / intermediate_dim=6144 (ArAE, DiT presets); got %d/%d",
                    cfg->hidden_dim, cfg->intermediate_dim);
    if (cfg->num_heads <= 0 || cfg->hidden_dim % cfg->num_heads) return fail(ER_ERR_INVALID, "hidden_dim %% num_heads != 0");
    const int D = cfg->hidden_dim / cfg->num_heads;
    if (D != 96 && D != 64) return fail(ER_ERR_UNSUPPORTED, "head_dim %d not built (96, 64)", D);
    const bool exact = cfg->weight_dtype == ER_F32 && cfg->kv_dtype == ER_F32;
    const bool kv8 = cfg->kv_dtype == ER_F8E4M3 && (cfg->weight_dtype == ER_F16 || cfg->weight_dtype == ER_F8E4M3 || cfg->weight_dtype == ER_F4E2M1);
    const bool w8 = cfg->weight_dtype == ER_F8E4M3 && (cfg->kv_dtype == ER_F16 || kv8);
    const bool w4 = cfg->weight_dtype == ER_F4E2M1 && (cfg->kv_dtype == ER_F16 || kv8);
    const bool fast = w8 || w4 || kv8 || (cfg->weight_dtype == ER_F16 && cfg->kv_dtype == ER_F16);
    if (!exact && !fast)
        return fail(ER_ERR_UNSUPPORTED, "built modes: fp32 weights + fp32 KV (exact), fp16 weights + fp16 KV (fast), e4m3 row-scaled weights + fp16 KV (fp8) or "
                                        "e2m1 block-scaled weights + fp16 KV (fp4); the fast, fp8 and fp4 weights also run on an e4m3 byte KV cache (kv8)");
    if (kv8 && D != 96) return fail(ER_ERR_UNSUPPORTED, "the e4m3 KV cache (kv8) is built for head_dim 96; got %d", D);
    if (cfg->vocab_size > ER_HEAD_MAX_VOCAB) return fail(ER_ERR_UNSUPPORTED, "vocab_size > %d", ER_HEAD_MAX_VOCAB);
    if (cfg->cond_mode == ER_COND_POINT && (cfg->point_hidden_dim != 1024 || cfg->point_hidden_dim % cfg->point_num_heads))
        return fail(ER_ERR_UNSUPPORTED, "point encoder width %d not built (1024)", cfg->point_hidden_dim);
    HIPCHK(hipSetDevice(device));
    er_ctx* c = new er_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->D = D;
    c->fast = fast;
    c->w8 = w8;
    c->w4 = w4;
    c->kv8 = kv8;
    c->kv_type = kv8 ? 2 : fast ? 1 : 0;
    c->kv_esz = kv8 ? 1 : fast ? 2 : 4;
    c->layers.resize(cfg->num_layers);
    c->pe.PH = cfg->point_hidden_dim; c->pe.heads = cfg->point_num_heads; c->pe.Lq = cfg->point_latent_size;
    c->pe.LD = cfg->point_latent_dim; c->pe.freq = cfg->point_freq_dim; c->pe.eps = cfg->ln_eps;
    c->knobs = read_knobs(fast);
    if (c->kv_type != 1) c->knobs.prefix_pass = ER_PREFIX_PASS_VALU;      // the matrix-core prefix pass reads fp16 caches only
    HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    HIPCHK(hipHostMalloc((void**)&c->h_pinned, 4096, hipHostMallocDefault));
    register_weights(c);
    *out = c;
    return ER_OK;
}

// The context's buffers, weight blocks and captured step are members: deleting the context frees them, once the device is idle.
extern "C" int er_destroy(er_ctx* c) {
    if (!c) return ER_OK;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    if (c->h_pinned) hipHostFree(c->h_pinned);
    if (c->q_pinned) hipHostFree(c->q_pinned);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
    return ER_OK;
}

// ------------------------------------------------------------------------------------ weights
extern "C" int er_load_tensor(er_ctx* c, const char* key, const void* data, int dtype, int ndim, const int64_t* shape,
                              int on_device) {
    if (!c || !key) return fail(ER_ERR_INVALID, "er_load_tensor: bad argument");
    HIPCHK(hipSetDevice(c->device));
    const int rc = weights_load(c->w, c->own_stream, "er_load_tensor", key, data, dtype, ndim, shape, on_device);
    if (rc != 1) memset(c->copy_made, 0, sizeof(c->copy_made));      // any reload invalidates every derived copy
    return rc;
}

extern "C" int er_finalize_weights(er_ctx* c) {
    if (!c) return fail(ER_ERR_INVALID, "null ctx");
    return weights_finalize(c->w);
}

// the tiled copy of a matrix (k_gemv_mfma.h); src: the row-major matrix, the byte block (w8_t) or the canonical MXFP4 block (w4_t: w4_tile_kernel)
template <typename WT>
static hipError_t launch_tile_weights(const void* src, void* dst, int N, int K, hipStream_t st) {
    if constexpr (WTraits<WT>::NIBBLES) {
        if (!w4t::shape_ok(N, K)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(w4_tile_kernel, dim3(2048), dim3(ER_WG), 0, st, reinterpret_cast<const unsigned char*>(src), reinterpret_cast<unsigned int*>(dst), (long long)N, K);
    } else {
        hipLaunchKernelGGL((tile_weights_kernel<WT>), dim3(2048), dim3(ER_WG), 0, st, reinterpret_cast<const WT*>(src), reinterpret_cast<f32x4*>(dst), N, K);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------ the weight copies
static WMode ctx_mode(const er_ctx* c) { return c->w4 ? W_FP4 : c->w8 ? W_FP8 : c->fast ? W_FAST : W_EXACT; }

// Where copy `s` of `proj` in layer L is: the loaded matrix or byte block, or a derived copy while it matches the loaded weights - else
// null, and the launch that wants it fails (run_proj)
static const void* weight_ptr(const er_ctx* c, const LayerW& L, Proj proj, WSrc s) {
    if (proj == PROJ_HEAD) return s != WSRC_PLAIN ? nullptr : c->fast ? (const void*)c->lm_head_h : (const void*)c->lm_head;
    const void* const w32[4] = {L.wqkv, L.wo, L.w1, L.w2};
    const void* const w16[4] = {L.wqkv_h, L.wo_h, L.w1_h, L.w2_h};
    const void* const w8[4] = {L.wqkv_q, L.wo_q, L.w1_q, L.w2_q};
    if (s == WSRC_PLAIN) return c->fast ? w16[proj] : w32[proj];
    if (s == WSRC_BYTES) return w8[proj];
    return c->copy_made[proj][s] ? L.copy[proj][s] : nullptr;
}
// ... and what a derived copy is made of: the plain matrix, the byte block or the canonical MXFP4 block
static const void* weight_origin(const er_ctx* c, const LayerW& L, Proj proj, WSrc s) {
    const void* const w4[4] = {L.wqkv_q4, L.wo_q4, L.w1_q4, L.w2_q4};
    return wsrc_nibbles(s) ? w4[proj] : weight_ptr(c, L, proj, s == WSRC_TILED_BYTES ? WSRC_BYTES : WSRC_PLAIN);
}

// Derived copy `s` of an [N][K] matrix (half: fp16 plain weights): its size, and the launch that makes it of `src` (weight_origin).
// The tiled copies are a second copy of the matrix in the layout the matrix-core batched kernels stream (2.5 GB fp32 / 1.3 GB fp16 of
// the 288 GB at 24 layers, 1.36 GB as bytes); the quad-interleaved copies are 15.4 MB per layer, fc2 k-major 0.9 GB fp32 / 0.45 GB fp16.
static size_t weight_copy_bytes(WSrc s, bool half, int N, int K) {
    switch (s) {
        case WSRC_TILED: return half ? tiled_weight_bytes<_Float16>(N, K) : tiled_weight_bytes<float>(N, K);
        case WSRC_TILED_BYTES: return tiled_weight_bytes<w8_t>(N, K);
        case WSRC_TILED_NIBBLES: return tiled_weight_bytes<w4_t>(N, K);
        case WSRC_QUADS: return (size_t)w4map::stream_bytes(N, K);
        case WSRC_KMAJOR: return (size_t)N * K * (half ? 2 : 4);
        default: return 0;
    }
}
static hipError_t launch_weight_copy(WSrc s, bool half, const void* src, void* dst, int N, int K, hipStream_t st) {
    if (!src || !dst) return hipErrorInvalidValue;
    switch (s) {
        case WSRC_TILED: return half ? launch_tile_weights<_Float16>(src, dst, N, K, st) : launch_tile_weights<float>(src, dst, N, K, st);
        case WSRC_TILED_BYTES: return launch_tile_weights<w8_t>(src, dst, N, K, st);
        case WSRC_TILED_NIBBLES: return launch_tile_weights<w4_t>(src, dst, N, K, st);
        case WSRC_QUADS:
            if (!w4map::shape_ok(N, K)) return hipErrorInvalidValue;
            hipLaunchKernelGGL(w4_interleave_kernel, dim3(2048), dim3(ER_WG), 0, st, (const unsigned char*)src, (unsigned char*)dst, (long long)N, K);
            return hipGetLastError();
        case WSRC_KMAJOR:
            if (N != MLP_HIDDEN || K != MLP_INTER) return hipErrorInvalidValue;
            return half ? launch_transpose_w2<_Float16>(src, dst, st) : launch_transpose_w2<float>(src, dst, st);
        default: return hipErrorInvalidValue;
    }
}

// The ONE owner of the derived copies: for each of qkv / out_proj / fc1 / fc2, and for the plan as stored and as a row class runs it
// (er_decode: fc1 and fc2 as row GEMVs on the same reserved shape), the copy weight_source names is made unless it has been, in every
// layer, in blocks of the weight table.  An fp8 or fp4 context so gets the tiled byte or nibble copy of a projection its plan streams
// packed and NO fp16 tiled copy of it; a later reserve whose plan names another copy makes it then.  The zero row goes with fc2 k-major.
static int ensure_weight_copies(er_ctx* c, const DecodePlan& plan) {
    if (weights_missing(c->w)) return 0;   // weights still loading: er_prefill comes back here
    const int H = c->cfg.hidden_dim, I = c->cfg.intermediate_dim;
    bool made = false;
    for (int row_class = 0; row_class < 2; ++row_class)
        for (int pj = 0; pj < 4; ++pj) {
            const WSrc s = weight_source(plan, c->knobs, ctx_mode(c), row_class != 0, (Proj)pj, 0);
            if (!wsrc_derived(s) || c->copy_made[pj][s]) continue;
            const int N = pj == PROJ_QKV ? 3 * H : pj == PROJ_FC1 ? I : H, K = pj == PROJ_FC2 ? I : H;
            if (s == WSRC_QUADS && !w4map::shape_ok(N, K)) return fail(ER_ERR_UNSUPPORTED, "fp4: a %d x %d matrix has no quad-interleaved copy", N, K);
            if (s == WSRC_KMAJOR && !c->zero_row) {
                char* z = nullptr;
                ERCHK(weights_alloc(c->w, &z, (size_t)H * 4));
                c->zero_row = z;
            }
            for (LayerW& L : c->layers) {
                if (!L.copy[pj][s]) {
                    char* blk = nullptr;
                    ERCHK(c->w.alloc(&blk, weight_copy_bytes(s, c->fast, N, K)));
                    L.copy[pj][s] = blk;
                }
                HIPCHK(launch_weight_copy(s, c->fast, weight_origin(c, L, (Proj)pj, s), L.copy[pj][s], N, K, c->own_stream));
            }
            c->copy_made[pj][s] = made = true;
        }
    if (made) HIPCHK(hipStreamSynchronize(c->own_stream));
    return 0;
}

// ------------------------------------------------------------------------------------ which decode kernels a cache shape gets
// The selection rules are host-only code in er_decode_plan.h (plan_decode, make_decode_plan, proj_form); the attention kernels' chunking
// enters them as numbers.
static AttnChunking attn_chunking(int heads) {
    return {attn3_num_chunks(heads), attn3_num_chunks(heads) * ATTN3_CAP, attn_chunk(ATTN_STEPS_DEFAULT)};
}

extern "C" int er_plan_decode(int batch, int heads, int head_dim, int hidden, int l_cap, er_decode_plan* out) {
    if (!out || batch <= 0 || heads <= 0 || head_dim <= 0 || l_cap <= 0) return fail(ER_ERR_INVALID, "er_plan_decode: bad argument");
    const DecodeKnobs k = read_knobs(false);
    plan_decode(k.decode_v, k.attn_v_batched, read_reserve_knobs().force_batched, batch, heads, head_dim, hidden, (l_cap + 31) / 32 * 32, attn_chunking(heads), out);
    return ER_OK;
}

// the plan of a LIVE context, as the last er_kv_reserve stored it: knobs of er_create, switches of that reserve (er_plan_decode above
// evaluates the same rules for hypothetical shapes with the environment as it is at call time)
extern "C" int er_ctx_plan(er_ctx* c, er_decode_plan* out) {
    if (!c || !out) return fail(ER_ERR_INVALID, "er_ctx_plan: null argument");
    if (c->kv->plan.B <= 0) return fail(ER_ERR_INVALID, "er_ctx_plan: no cache reserved (call er_kv_reserve)");
    *out = c->kv->plan.sel;
    return ER_OK;
}

// The reporters project the step's own rule (weight_source, with the context's row class) onto their question.
static int report_sources(er_ctx* c, const char* who, int32_t out[4], bool (*asks)(WSrc)) {
    if (!c || !out) return fail(ER_ERR_INVALID, "%s: null argument", who);
    const DecodePlan& p = c->kv->plan;
    if (p.B <= 0) return fail(ER_ERR_INVALID, "%s: no cache reserved (call er_kv_reserve)", who);
    for (int pj = 0; pj < 4; ++pj) out[pj] = asks(weight_source(p, c->knobs, ctx_mode(c), c->kv->row_class, (Proj)pj, 0)) ? 1 : 0;
    return ER_OK;
}
// which of qkv / out_proj / fc1 / fc2 the stored plan of a live context streams as e4m3 bytes (fp8 mode; all zero in every other mode)
extern "C" int er_ctx_w8_streams(er_ctx* c, int32_t out[4]) { return report_sources(c, "er_ctx_w8_streams", out, wsrc_bytes); }
// ... as e2m1 nibbles in their row forms (fp4 mode; all zero in every other mode)
extern "C" int er_ctx_w4_streams(er_ctx* c, int32_t out[4]) {
    return report_sources(c, "er_ctx_w4_streams", out, [](WSrc s) { return s == WSRC_QUADS; });
}
// ... and as nibbles in their matrix-core batched forms (fp4 mode; all zero in every other mode, and for a plan that is not batched):
// er_ctx_w4_streams keeps reporting the row forms only
extern "C" int er_ctx_w4_streams_batched(er_ctx* c, int32_t out[4]) {
    return report_sources(c, "er_ctx_w4_streams_batched", out, [](WSrc s) { return s == WSRC_TILED_NIBBLES; });
}

extern "C" int er_plan_gemm_tile(int m, int n, int batch) {
    if (m <= 0 || n <= 0 || batch <= 0) return fail(ER_ERR_INVALID, "er_plan_gemm_tile: bad argument");
    return gemm_pick_tile(m, n, batch);
}

// ------------------------------------------------------------------------------------ KV cache / workspace
static int kv_alloc(er_ctx* c, KvMem& m, int batch, int Lcap);

extern "C" int er_kv_reserve(er_ctx* c, int batch, int max_len) {
    if (!c || batch <= 0 || max_len <= 0) return fail(ER_ERR_INVALID, "er_kv_reserve: bad argument");
    if (batch > ER_MAX_BATCH) return fail(ER_ERR_UNSUPPORTED, "er_kv_reserve: batch %d > %d (host staging buffers are sized for %d rows)", batch, ER_MAX_BATCH, ER_MAX_BATCH);
    HIPCHK(hipSetDevice(c->device));
    const er_config& g = c->cfg;
    if (max_len > g.max_positions)
        return fail(ER_ERR_CAPACITY, "max_len %d exceeds the position table (%d)", max_len, g.max_positions);
    const int Lcap = (max_len + 31) / 32 * 32;
    if (c->kv->plan.B == batch && c->kv->plan.Lcap == Lcap) {
        c->kv->valid_prefix = 0;                 // a reserve starts over: nothing of the rows' earlier content is promised
        return c->kv->prefix_len ? er_set_prefix_groups(c, nullptr, 0, 0) : ER_OK;
    }
    HIPCHK(hipDeviceSynchronize());
    c->kv = std::make_unique<KvMem>();           // first: the old shape's memory makes room for the new one (this plan says: no cache)
    c->have_hidden = false;
    c->q.end();                                  // a queue lives on the rows of one reserved shape
    auto m = std::make_unique<KvMem>();
    ERCHK(kv_alloc(c, *m, batch, Lcap));         // a failed hipMalloc half way leaves nothing behind: m and its plan die here
    c->kv = std::move(m);                        // buffers and plan of the new shape, in one step
    return ER_OK;
}

// the buffers of the new shape and the decode plan that goes with them, both into m (of c, only the tiled weight copies may change)
static int kv_alloc(er_ctx* c, KvMem& m, int batch, int Lcap) {
    const er_config& g = c->cfg;
    const int H = g.num_heads, D = c->D, hid = g.hidden_dim;
    m.plan = make_decode_plan(c->knobs, read_reserve_knobs(), c->fast, batch, Lcap, g.num_layers, H, D, hid, attn_chunking(H), false, c->kv8);
    const DecodePlan& p = m.plan;
    const size_t kv_bytes = (size_t)p.kv_lstride * g.num_layers * c->kv_esz;
    ERCHK(m.kc.ensure(kv_bytes));
    ERCHK(m.vc.ensure(kv_bytes));
    const size_t b = (size_t)batch;
    for (DevBuf<float>* w : {&m.ypre, &m.hbuf, &m.ypre1, &m.h1buf, &m.qbuf, &m.abuf}) ERCHK(w->ensure(b * hid));
    ERCHK(m.fbuf.ensure(b * g.intermediate_dim));
    ERCHK(m.logits.ensure(b * g.vocab_size));
    ERCHK(m.part.ensure(b * H * (size_t)std::max(p.S_splits * (D + 2), p.nch3 * D)));
    ERCHK(m.part_ml.ensure(b * H * (size_t)p.nch3 * 2));
    ERCHK(m.state_block.ensure(gen_state_ints(b)));
    m.st = gen_state_carve(m.state_block.p, b);
    ERCHK(m.d_params.ensure(1));
    ERCHK(m.d_ctl.ensure(1));
    ERCHK(m.d_ids_tmp.ensure(b));
    ERCHK(m.d_row_stream.ensure(b));
    {
        std::vector<unsigned int> ident(b);
        for (size_t i = 0; i < b; ++i) ident[i] = (unsigned int)i;
        HIPCHK(hipMemcpy(m.d_row_stream.p, ident.data(), b * sizeof(unsigned int), hipMemcpyHostToDevice));
    }
    m.st.row_stream = m.d_row_stream.p;
    ERCHK(m.d_row_budget.ensure(b));
    {
        const std::vector<int> open(b, 0x7fffffff);
        HIPCHK(hipMemcpy(m.d_row_budget.p, open.data(), b * sizeof(int), hipMemcpyHostToDevice));
    }
    m.st.row_budget = m.d_row_budget.p;
    ERCHK(m.d_out_ids.ensure(b * (size_t)Lcap));
    ERCHK(ensure_weight_copies(c, p));
    if (p.mlp_fused) {
        ERCHK(m.mlp_part.ensure((size_t)MLP_WGS * hid));
        ERCHK(m.mlp_nnz.ensure((size_t)g.num_layers * MLP_WGS));
        HIPCHK(hipMemset(m.mlp_nnz.p, 0, m.mlp_nnz.n * sizeof(int)));
    }
    // split-K partials of the batched projections.  A finish launched right behind its producer re-uses ONE [4][32][N] block; only the
    // tiled path defers finishes to a later launch (prep_rows_kernel, sk_part) and keeps a [16][32][hidden] block per group of 32 rows
    const size_t groups = (b + NBM - 1) / NBM;
    ERCHK(m.skpart.ensure(p.xt ? groups * SK_SLICES_FC2 * NBM * (size_t)hid : (size_t)SK_SLICES_OUTPROJ * NBM * (size_t)std::max(hid, g.vocab_size)));
    // fast mode, matrix-core projections: the activations travel in the tiled hi | lo operand layout (k_gemv.h xt_entry).  One image
    // of K x 128 bytes per group of 32 rows; zeroed once so that the rows of a last, partial group never hold NaN patterns.
    if (p.xt) {
        const size_t b_h = groups * (size_t)hid * 128, b_f = groups * (size_t)g.intermediate_dim * 128;
        ERCHK(m.xt_h.ensure(b_h));
        ERCHK(m.xt_att.ensure(b_h));
        ERCHK(m.xt_f.ensure(b_f));
        HIPCHK(hipMemset(m.xt_h.p, 0, b_h));
        HIPCHK(hipMemset(m.xt_att.p, 0, b_h));
        HIPCHK(hipMemset(m.xt_f.p, 0, b_f));
    }
    return ER_OK;
}

// ------------------------------------------------------------------------------------ decode step
static AttnDecArgs attn_args(er_ctx* c, int layer) {
    const DecodePlan& p = c->kv->plan;
    AttnDecArgs a = attn_dec_args(c->cfg.num_heads, c->D, p.Lcap);
    a.q = c->kv->qbuf.p;
    a.kcache = c->kv->kc.p + (long long)layer * p.kv_lstride * c->kv_esz;
    a.vcache = c->kv->vc.p + (long long)layer * p.kv_lstride * c->kv_esz;
    a.chunk = attn_chunk(ATTN_STEPS_DEFAULT);
    a.pos = c->kv->st.pos;
    a.fixed_len = c->prof_len;
    a.part = c->kv->part.p;
    a.part_ml = c->kv->part_ml.p;
    a.out = c->kv->abuf.p;
    a.S = p.S_splits;
    a.out_xt = p.outproj_partials ? c->kv->xt_att.p : nullptr;      // out_proj then reads the tiled image
    return a;
}

// the two launches of a layer under prefix groups: the partials of the prefix chunks live in KvMem::part (ceil(P / 128) <= S_splits per (row, head))
static AttnSharedArgs attn_shared_args(er_ctx* c, int layer) {
    AttnSharedArgs s{};
    s.a = attn_args(c, layer);
    s.prefix_len = c->kv->prefix_len;
    s.a.S = attn_shared_chunks(s.prefix_len);
    s.grp_rows = c->kv->grp_rows.p; s.grp_off = c->kv->grp_off.p;
    return s;
}

static hipError_t launch_attn_partial(const AttnDecArgs& a, int D, int steps, int kv_half, int B, hipStream_t st, int ver = 2) {
    return D == 96 ? launch_attn_partial_d<96>(a, steps, kv_half, B, st, ver) : launch_attn_partial_d<64>(a, steps, kv_half, B, st, ver);
}
static hipError_t launch_attn_combine(const AttnDecArgs& a, int D, int B, hipStream_t st) {
    return D == 96 ? launch_attn_combine_d<96>(a, B, st) : launch_attn_combine_d<64>(a, B, st);
}

// The copy of its matrix the step streams for `proj` of `layer` (weight_source) and where it is (null: not made of the loaded weights)
struct StepWeight { WSrc src; const void* w; };
static StepWeight step_weight(const er_ctx* c, Proj proj, int layer) {
    const WSrc s = weight_source(c->kv->plan, c->knobs, ctx_mode(c), c->kv->row_class, proj, layer);
    return {s, weight_ptr(c, c->layers[proj == PROJ_HEAD ? 0 : layer], proj, s)};
}

// the fused single-row MLP of `layer` on the context's buffers (kinds 4 and 5 of a plan with mlp_fused): fc1 plain, fc2 k-major
static MlpArgs mlp_args(er_ctx* c, int layer) {
    const LayerW& L = c->layers[layer];
    const KvMem& kv = *c->kv;
    MlpArgs m{};
    m.W1 = step_weight(c, PROJ_FC1, layer).w; m.b1 = L.b1; m.W2T = step_weight(c, PROJ_FC2, layer).w; m.zero_row = c->zero_row;
    m.xin = kv.ypre1.p; m.ln_w = L.ln1w; m.ln_b = L.ln1b; m.eps = c->cfg.ln_eps; m.hout = kv.h1buf.p;
    m.part = kv.mlp_part.p; m.nnz = kv.mlp_nnz.p + (size_t)layer * MLP_WGS;
    m.b2 = L.b2; m.resid = kv.h1buf.p; m.out = kv.ypre.p;
    return m;
}

// A projection kind fills the operands from the context (row-major input, and in io what the other forms read instead); the form comes
// from proj_form, the weight copy from weight_source (weights_of: one lookup per projection) and the launches from run_proj (er_decode_proj.h).
template <typename WT>
static hipError_t launch_kind_t(er_ctx* c, int kind, int layer, hipStream_t st, long long* out_ids, int out_ld) {
    constexpr bool HALF = sizeof(WT) == 2;      // fp16 weights; the cache type is the context's own (c->kv_type: kv8 stores bytes under fp16 weights)
    const er_config& g = c->cfg;
    const DecodePlan& p = c->kv->plan;
    const KvMem& kv = *c->kv;
    const int H = g.hidden_dim, I = g.intermediate_dim, B = p.B;
    const SkPart sk{kv.skpart.p, kv.skpart.n};
    const auto form_of = [&](Proj proj, int l) { return proj_form(p, c->knobs, HALF, proj, l); };
    ProjIo io;
    const auto weights_of = [&](Proj proj) { const StepWeight w = step_weight(c, proj, layer); io.src = w.src; io.w = w.w; };
    const bool v3 = p.v3 && !kv.row_class, fused = p.mlp_fused && !kv.row_class;
    GemvArgs a{};
    a.eps = g.ln_eps;
    a.hidden = H; a.head_dim = c->D; a.l_cap = p.Lcap; a.kv_bstride = p.kv_bstride; a.kv_half = c->kv_type;
    switch (kind) {
        case 0: {   // qkv
            const LayerW& L = c->layers[layer];
            weights_of(PROJ_QKV); a.bias = L.bqkv; a.N = 3 * H;
            a.hout = kv.hbuf.p; a.pos = kv.st.pos;
            a.q = kv.qbuf.p;
            a.kcache = kv.kc.p + (long long)layer * p.kv_lstride * c->kv_esz;
            a.vcache = kv.vc.p + (long long)layer * p.kv_lstride * c->kv_esz;
            if (layer == 0) {
                io.pro = PRO_EMBED; a.embd = c->embd; a.posemb = c->posemb; a.tok = kv.st.tok;
            } else {
                io.pro = PRO_LN; a.xin = kv.ypre.p; a.ln_w = c->layers[layer - 1].ln2w; a.ln_b = c->layers[layer - 1].ln2b;
                // the previous layer's fc2 deferred its split-K finish to this LayerNorm
                if (form_of(PROJ_FC2, layer - 1).defer) io.rd = {sk.p, c->layers[layer - 1].b2, kv.h1buf.p, SK_SLICES_FC2};
            }
            io.x_image = kv.xt_h.p; io.pro_image = p.xt ? kv.xt_h.p : nullptr;
            return run_proj<WT>(PROJ_QKV, form_of(PROJ_QKV, layer), io, a, B, H, sk, st);
        }
        // v2 holds a wave's whole K/V slice in flight (latency-bound single rows); with hundreds of workgroups per CU's
        // worth of work (B > 4) the leaner v1 (66-74 VGPRs, 6-7 waves per SIMD) streams faster: 570 vs 636 us at B = 32, L = 18050
        case 1:
            if (v3) return launch_attn_partial3_d<96>(attn_args(c, layer), HALF, p.nch3, B, st);
            if (p.shared_mfma) return launch_attn_prefix_mfma_d<96>(attn_shared_args(c, layer), kv.n_groups, st);
            if (p.shared_attn) return launch_attn_prefix_d<96>(attn_shared_args(c, layer), HALF, kv.n_groups, st);
            if (p.stream_attn) return launch_attn_stream_d<96>(attn_args(c, layer), c->kv_type, B, st);
            return launch_attn_partial(attn_args(c, layer), c->D, ATTN_STEPS_DEFAULT, c->kv_type, B, st, p.batched ? 1 : 2);
        case 2:
            if (!p.sel.merge_launch && !(p.v3 && !v3)) return hipSuccess;      // the merge runs inside the out_proj kernel (version 3) / there are no partials (streaming)
            if (p.shared_attn) return launch_attn_suffix_merge_d<96>(attn_shared_args(c, layer), HALF, B, st);
            return launch_attn_combine(attn_args(c, layer), c->D, B, st);
        case 3: {   // out_proj + bias + residual(h) -> ypre1
            const LayerW& L = c->layers[layer];
            if (v3) {
                OutMergeArgs m{};
                weights_of(PROJ_OUT);      // the byte block or the plain copy
                m.W = io.w; m.bias = L.bo; m.resid = c->kv->hbuf.p; m.out = c->kv->ypre1.p;
                m.part_o = c->kv->part.p; m.part_ml = c->kv->part_ml.p; m.N = H;
                if (!m.W || (io.src != WSRC_BYTES && io.src != WSRC_PLAIN)) return hipErrorInvalidValue;
                return io.src == WSRC_BYTES ? launch_outproj_merge<w8_t, 96>(m, p.nch3, st) : launch_outproj_merge<WT, 96>(m, p.nch3, st);
            }
            weights_of(PROJ_OUT); a.bias = L.bo; a.N = H; a.xin = kv.abuf.p; a.out = kv.ypre1.p; a.resid = kv.hbuf.p;
            io.x_image = kv.xt_att.p;      // the streaming attention wrote the image (attn_args: out_xt)
            return run_proj<WT>(PROJ_OUT, form_of(PROJ_OUT, layer), io, a, B, H, sk, st);
        }
        case 4: {   // h1 = LN1(ypre1); f = relu(fc1 h1 + b)
            const LayerW& L = c->layers[layer];
            if (fused) {      // ... and the chain sums of fc2 over the live neurons; f stays in the workgroups
                const MlpArgs m = mlp_args(c, layer);
                if (!m.W1 || !m.W2T) return hipErrorInvalidValue;      // fc2 k-major does not match the loaded weights
                return launch_mlp_fused<WT>(m, st);
            }
            weights_of(PROJ_FC1); a.bias = L.b1; a.N = I; a.xin = kv.ypre1.p; a.ln_w = L.ln1w; a.ln_b = L.ln1b;
            a.hout = kv.h1buf.p; a.out = kv.fbuf.p;
            io.pro = PRO_LN;
            // out_proj (case 3) left four K-range partials: ypre1 = ((sum) + bo) + h
            if (form_of(PROJ_OUT, layer).defer) io.rd = {sk.p, L.bo, kv.hbuf.p, SK_SLICES_OUTPROJ};
            io.x_image = kv.xt_h.p; io.pro_image = p.xt ? kv.xt_h.p : nullptr; io.out_image = kv.xt_f.p;
            return run_proj<WT>(PROJ_FC1, form_of(PROJ_FC1, layer), io, a, B, H, sk, st);
        }
        case 5: {   // ypre = fc2 f + b + h1
            const LayerW& L = c->layers[layer];
            if (fused) return launch_mlp_finish(mlp_args(c, layer), st);
            weights_of(PROJ_FC2); a.bias = L.b2; a.N = H; a.xin = kv.fbuf.p; a.out = kv.ypre.p; a.resid = kv.h1buf.p;
            io.x_image = kv.xt_f.p;
            return run_proj<WT>(PROJ_FC2, form_of(PROJ_FC2, layer), io, a, B, I, sk, st);
        }
        case 6: {   // logits = lm_head LN2_last(ypre)
            weights_of(PROJ_HEAD); a.bias = nullptr; a.N = g.vocab_size; a.xin = kv.ypre.p;
            a.ln_w = c->layers[p.layers - 1].ln2w; a.ln_b = c->layers[p.layers - 1].ln2b; a.hout = p.batched ? kv.hbuf.p : nullptr; a.out = kv.logits.p;
            io.pro = PRO_LN;
            return run_proj<WT>(PROJ_HEAD, form_of(PROJ_HEAD, layer), io, a, B, H, sk, st);
        }
        case 7:
            if (kv.head_ctl) {
                const HeadCtlOut lp{kv.lp_on ? kv.d_lp_model.p : nullptr, kv.lp_on ? kv.d_lp_policy.p : nullptr, nullptr, p.Lcap};
                hipLaunchKernelGGL(sample_head_ctl_kernel, dim3(B), dim3(ER_WG), sample_head_lds(g.vocab_size), st, kv.logits.p,
                                   kv.d_params.p, kv.d_ctl.p, kv.st, out_ids, out_ld, lp);
                return hipGetLastError();
            }
            hipLaunchKernelGGL(sample_head_kernel, dim3(B), dim3(ER_WG), sample_head_lds(g.vocab_size), st, c->kv->logits.p,
                               c->kv->d_params.p, c->kv->st, out_ids, out_ld);
            return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_kind(er_ctx* c, int kind, int layer, hipStream_t st, long long* out_ids, int out_ld) {
    return c->fast ? launch_kind_t<_Float16>(c, kind, layer, st, out_ids, out_ld)
                   : launch_kind_t<float>(c, kind, layer, st, out_ids, out_ld);
}

static hipError_t enqueue_layers(er_ctx* c, hipStream_t st) {
    for (int l = 0; l < c->cfg.num_layers; ++l)
        for (int k = 0; k <= 5; ++k) {
            hipError_t e = launch_kind(c, k, l, st, nullptr, 0);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

static hipError_t enqueue_step(er_ctx* c, hipStream_t st, long long* out_ids, int out_ld) {
    hipError_t e = launch_kind(c, 6, 0, st, nullptr, 0);
    if (e != hipSuccess) return e;
    e = launch_kind(c, 7, 0, st, out_ids, out_ld);
    if (e != hipSuccess) return e;
    return enqueue_layers(c, st);
}

// ------------------------------------------------------------------------------------ GEMM helpers (prefill / encoder)
static hipError_t linear(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N, int K,
                         bool relu, const float* resid, int ldr, hipStream_t st) {
    return launch_gemm(gemm_args_linear(A, lda, W, bias, C, ldc, M, N, K, relu, resid, ldr), 1, st);
}

// fast mode: C = epilogue((A_hi + A_lo) . W_fp16^T) on the fp16 matrix cores (k_gemm.h, gemm_f16_mfma_kernel<SPLIT>)
static hipError_t linear_h(const float* A, int lda, const _Float16* W, const float* bias, float* C, int ldc, int M, int N, int K,
                           bool relu, const float* resid, int ldr, hipStream_t st) {
    return launch_gemm_f16s(gemm_args_linear(A, lda, W, bias, C, ldc, M, N, K, relu, resid, ldr), st);
}

// the same product through the LDS-DMA kernel (k_gemm.h, split form): the fp32 activation is split into hi / lo fp16 arrays by one
// streaming pass, then both A images and the weight tile reach LDS by DMA.  K % 64 == 0 (1536 / 6144 on the prefill path);
// same split and MFMA order as linear_h (fast-mode logits unchanged to the last digit); used for small M only (see the body)
static int linear_hs(er_ctx* c, const float* A, int lda, const _Float16* W, const float* bias, float* C, int ldc, int M, int N, int K,
                     bool relu, const float* resid, int ldr, hipStream_t st);

#define HIPRET(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ER_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)

static int linear_hs(er_ctx* c, const float* A, int lda, const _Float16* W, const float* bias, float* C, int ldc, int M, int N, int K,
                     bool relu, const float* resid, int ldr, hipStream_t st) {
    // measured (profiles/r03_prefill_fast_gemm.log): with its 64-row tiles (two A images per stage) and the extra split pass the
    // LDS-DMA form wins at 2050 rows (one prefix: encode + prefill 24.2 -> 23.1 ms) and loses to the register-staged 128 x 128 kernel
    // at 16400 rows and beyond (8 prefixes: 13.4 -> 13.8 ms per sample, 32: 12.65 -> 13.1).  The rule is on ROWS - what decides is how
    // many 64-row tiles a CU has to walk, whoever owns the rows - so one long resumed prefix (core/models.py:225-226; 14050 rows in the
    // long-context tests) takes the register-staged kernel exactly as seven short ones would.  Both forms give the same bits
    // (tests/test_gpu_kernels.py::test_gemm_f16s_forms_agree).
    constexpr int HS_MAX_ROWS = 4608;          // two 2050-token prefixes + slack
    if (K % XBK != 0 || M > HS_MAX_ROWS) { HIPRET(linear_h(A, lda, W, bias, C, ldc, M, N, K, relu, resid, ldr, st)); return 0; }
    ERCHK(c->p_hi.ensure((size_t)M * K + F16_TAIL));
    ERCHK(c->p_lo.ensure((size_t)M * K + F16_TAIL));
    _Float16 *hi = c->p_hi.p, *lo = c->p_lo.p;
    HIPRET(launch_split_rows_f16(A, hi, lo, (long long)M, K, lda, st));
    GemmArgs g = gemm_args_linear(hi, K, W, bias, C, ldc, M, N, K, relu, resid, ldr);
    g.a_lo = lo;
    HIPRET(launch_gemm_hh_split(g, st));
    return 0;
}

// softmax(Q K^T / sqrt(D)) V for one sample, all heads; scores live in `sc` ([H][N][ldS]).
static int attention_full(const float* Q, int ldq, const float* Kp, int ldk, long long k_hstride, const float* Vp, int ldv,
                          long long v_hstride, float* out, int ldo, float* sc, int H, int D, int N, int M, bool causal,
                          hipStream_t st) {
    const int ldS = (M + 15) / 16 * 16;
    GemmArgs g = gemm_args_default();
    g.A = Q; g.lda = ldq; g.sA2 = D;
    g.B = Kp; g.ldb = ldk; g.sB2 = k_hstride;
    g.C = sc; g.ldc = ldS; g.sC2 = (long long)N * ldS;
    g.Z2 = H; g.M = N; g.N = M; g.K = D; g.div = sqrtf((float)D);
    g.causal = causal ? 1 : 0; g.causal_off = M - N;
    HIPRET(launch_gemm(g, H, st));
    HIPRET(launch_softmax_rows(sc, N, M, (long long)ldS, ldS, (long long)N * ldS, H, causal ? 1 : 0, M - N, st));
    GemmArgs p = gemm_args_default();
    p.A = sc; p.lda = ldS; p.sA2 = (long long)N * ldS;
    p.B = Vp; p.ldb = ldv; p.sB2 = v_hstride; p.b_is_kn = 1; p.kb_valid = M;
    p.C = out; p.ldc = ldo; p.sC2 = D;
    p.Z2 = H; p.M = N; p.N = D; p.K = ldS;
    p.causal = causal ? 1 : 0; p.causal_off = M - N;
    HIPRET(launch_gemm(p, H, st));
    return 0;
}

// ------------------------------------------------------------------------------------ encode_cond
// PointEncoderEmbed (core/transformer/point.py:186-206) of nb samples of N points each: the latent mean (posterior.mode(), :201)
// into p.lat [nb][Lq][LD].  Shared by er_encode_cond (which projects it, core/models.py:124), er_point_latent and
// er_dit_point_latent.  Mode ER_PE_DOWNSAMPLE is PointEncoder (:143-169): the queries are point_embed (before ln) of the Lq points a
// farthest point sampling picks from each cloud (k_fps.h), one query table per sample.  Callers go through the samples in chunks of
// up to ENC_CHUNK (scratch for one chunk at N = 4096: ~5 GB); every GEMM / LayerNorm / attention launch of a chunk covers all of them.
constexpr int ENC_CHUNK = 32;
static int point_latent_chunk(PointEnc& p, const float* pts, int nb, int N, hipStream_t st) {
    const int PH = p.PH, Lq = p.Lq, LD = p.LD;
    const int PHh = p.heads > 0 ? p.heads : 1, PD = PH / PHh;
    const bool ds = p.mode == ER_PE_DOWNSAMPLE;
    if (N <= 0) return fail(ER_ERR_INVALID, "n_points must be > 0");
    if (ds && N < Lq)
        return fail(ER_ERR_INVALID, "point_encoder_mode downsample samples point_latent_size = %d points per cloud; the clouds have %d", Lq, N);
    const size_t R = (size_t)nb * N, RQ = (size_t)nb * Lq;
    const size_t QR = ds ? RQ : (size_t)Lq;   // rows of the query table: per sample (downsample) or one shared table (embed)
    ERCHK(p.a0.ensure(R * p.kpad));
    ERCHK(p.x.ensure(R * PH));
    ERCHK(p.k.ensure(R * PH));
    ERCHK(p.v.ensure(R * PH));
    ERCHK(p.qln.ensure(QR * PH));
    ERCHK(p.q.ensure(QR * PH));
    ERCHK(p.att.ensure(RQ * PH));
    ERCHK(p.l.ensure(RQ * PH));
    ERCHK(p.ln.ensure(RQ * PH));
    ERCHK(p.u.ensure(RQ * 8 * PH));
    ERCHK(p.g.ensure(RQ * 4 * PH));
    ERCHK(p.lat.ensure(RQ * LD));
    int32_t* fidx = nullptr;
    if (ds) {
        ERCHK(p.q0.ensure(RQ * PH));
        ERCHK(p.fidx.ensure(RQ));
        if (N > FPS_REG_MAX) ERCHK(p.fdist.ensure(R));
        fidx = p.fidx.p;
        // fps_indices = torch_cluster.fps(pc, batch, ratio = Lq / N)                  point.py:152-156
        HIPRET(launch_fps(pts, nb, N, Lq, fidx, p.fdist.p, st));
    }
    // x = ln(point_embed(pts))                                          point.py:194
    HIPRET(launch_point_embed(pts, p.basis, p.a0.p, (long long)R, p.freq, p.kpad, st));
    HIPRET(linear(p.a0.p, p.kpad, p.mlp_w, p.mlp_b, p.x.p, PH, (int)R, PH, p.kpad, false, nullptr, 0, st));
    if (ds) {   // q = point_embed(pc[fps_indices]): the sampled rows of the point_embed output, before ln      point.py:157-158
        hipLaunchKernelGGL(fps_gather_rows_kernel, dim3((unsigned)RQ), dim3(ER_WG), 0, st, p.x.p, fidx, N, Lq, PH, p.q0.p);
        HIPRET(hipGetLastError());
    }
    HIPRET(launch_layernorm(p.x.p, p.ln_w, p.ln_b, p.x.p, (int)R, PH, PH, PH, p.eps, st));
    // cross attention: l = q + out_proj(attn(q_proj(ln1(q)), k_proj(x), v_proj(x)))   point.py:123-124
    // (embed mode: the learned queries and their projection are the same for every sample: computed once)
    const float* qsrc = ds ? p.q0.p : p.query;
    HIPRET(launch_layernorm(qsrc, p.ca_ln1_w, p.ca_ln1_b, p.qln.p, (int)QR, PH, PH, PH, p.eps, st));
    HIPRET(linear(p.qln.p, PH, p.ca_q_w, p.ca_q_b, p.q.p, PH, (int)QR, PH, PH, false, nullptr, 0, st));
    HIPRET(linear(p.x.p, PH, p.ca_k_w, p.ca_k_b, p.k.p, PH, (int)R, PH, PH, false, nullptr, 0, st));
    HIPRET(linear(p.x.p, PH, p.ca_v_w, p.ca_v_b, p.v.p, PH, (int)R, PH, PH, false, nullptr, 0, st));
    if (PD == 64 || PD == 96) {
        Flash32Args f{};
        f.Q = p.q.p; f.ldq = PH; f.qs_b = ds ? (long long)Lq * PH : 0; f.qs_h = PD;   // embed: queries shared by the batch
        f.K = p.k.p; f.ldk = PH; f.ks_b = (long long)N * PH; f.ks_h = PD;
        f.V = p.v.p; f.ldv = PH; f.vs_b = (long long)N * PH; f.vs_h = PD;
        f.O = p.att.p; f.ldo = PH; f.os_b = (long long)Lq * PH; f.os_h = PD;
        f.N = Lq; f.M = N; f.sqrt_d = sqrtf((float)PD); f.causal_off = 0;
        HIPRET(launch_flash_attn_f32(f, PD, false, PHh, nb, st));
    } else {
        const int ldS = (N + 15) / 16 * 16;
        ERCHK(p.sc.ensure((size_t)PHh * Lq * ldS));
        for (int b = 0; b < nb; ++b)
            ERCHK(attention_full(p.q.p + (ds ? (size_t)b * Lq * PH : 0), PH, p.k.p + (size_t)b * N * PH, PH, PD,
                                 p.v.p + (size_t)b * N * PH, PH, PD, p.att.p + (size_t)b * Lq * PH, PH, p.sc.p, PHh, PD, Lq, N, false, st));
    }
    {   // l = q + out_proj(att): embed mode's residual table has Lq rows shared by every sample; downsample's has one per sample
        GemmArgs ga = gemm_args_default();
        ga.A = p.att.p; ga.B = p.ca_o_w; ga.C = p.l.p; ga.bias = p.ca_o_b; ga.resid = qsrc; ga.resid_mod = ds ? 0 : Lq;
        ga.M = (int)RQ; ga.N = PH; ga.K = PH; ga.lda = PH; ga.ldb = PH; ga.ldc = PH; ga.ldr = PH;
        HIPRET(launch_gemm(ga, 1, st));
    }
    // l = l + net2(GEGLU(net0(ln2(l))))                                   point.py:125, 68-84
    HIPRET(launch_layernorm(p.l.p, p.ca_ln2_w, p.ca_ln2_b, p.ln.p, (int)RQ, PH, PH, PH, p.eps, st));
    HIPRET(linear(p.ln.p, PH, p.ff0_w, p.ff0_b, p.u.p, 8 * PH, (int)RQ, 8 * PH, PH, false, nullptr, 0, st));
    HIPRET(launch_geglu(p.u.p, p.g.p, (long long)RQ, 4 * PH, st));
    HIPRET(linear(p.g.p, 4 * PH, p.ff2_w, p.ff2_b, p.l.p, PH, (int)RQ, PH, 4 * PH, false, p.l.p, PH, st));
    // latent mean = linear(l)                                              point.py:201
    HIPRET(linear(p.l.p, PH, p.lin_w, p.lin_b, p.lat.p, LD, (int)RQ, LD, PH, false, nullptr, 0, st));
    return 0;
}

// the latent means of B clouds of N points into latent_out [B][Lq][LD] (er_point_latent, er_dit_point_latent)
static int pe_latent(PointEnc& p, const float* pts, int B, int N, float* latent_out, hipStream_t st, const char* who) {
    const size_t per = (size_t)p.Lq * p.LD;
    if ((long long)B * (long long)per > 0x7fffffffLL) return fail(ER_ERR_CAPACITY, "%s: batch %d too large", who, B);
    for (int b0 = 0; b0 < B; b0 += ENC_CHUNK) {
        const int nb = std::min(ENC_CHUNK, B - b0);
        ERCHK(point_latent_chunk(p, pts + (size_t)b0 * N * 3, nb, N, st));
        HIPCHK(hipMemcpyAsync(latent_out + (size_t)b0 * per, p.lat.p, (size_t)nb * per * 4, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

extern "C" int er_encode_cond(er_ctx* c, const float* conds, int B, int n_points, const int32_t* face_bucket,
                              float* cond_out, void* stream) {
    if (!c || !cond_out || B <= 0) return fail(ER_ERR_INVALID, "er_encode_cond: bad argument");
    ERCHK(er_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const er_config& g = c->cfg;
    const int H = g.hidden_dim, C = g.num_cond_tokens, Lq = g.point_latent_size, LD = g.point_latent_dim;
    const int n_lat = (g.cond_mode == ER_COND_NONE) ? 0 : Lq;
    const int n_face = g.num_face_buckets > 0 ? 1 : 0;
    if (n_lat + n_face != C) return fail(ER_ERR_INVALID, "num_cond_tokens %d != latent tokens %d + face token %d", C, n_lat, n_face);
    if (g.cond_mode != ER_COND_NONE && !conds) return fail(ER_ERR_INVALID, "er_encode_cond: conds is null");
    if (LD % 16) return fail(ER_ERR_UNSUPPORTED, "point_latent_dim must be a multiple of 16");
    for (int b0 = 0; b0 < B; b0 += ENC_CHUNK) {
        const int nb = std::min(ENC_CHUNK, B - b0);
        const float* lat = nullptr;   // [nb][Lq][LD]
        if (g.cond_mode == ER_COND_POINT) {
            ERCHK(point_latent_chunk(c->pe, conds + (size_t)b0 * n_points * 3, nb, n_points, st));
            lat = c->pe.lat.p;
        } else if (g.cond_mode == ER_COND_POINT_LATENT) {
            lat = conds + (size_t)b0 * Lq * LD;
        }
        if (lat) {   // norm_cond(proj_cond(latent))                               core/models.py:124 / 128-129
            ERCHK(c->e_tmp.ensure((size_t)nb * Lq * H));
            HIPRET(linear(lat, LD, c->proj_w, c->proj_b, c->e_tmp.p, H, nb * Lq, H, LD, false, nullptr, 0, st));
        }
        for (int b = 0; b < nb; ++b) {
            float* out_b = cond_out + (size_t)(b0 + b) * C * H;
            if (lat) HIPRET(launch_layernorm(c->e_tmp.p + (size_t)b * Lq * H, c->normc_w, c->normc_b, out_b, Lq, H, H, H, g.ln_eps, st));
            if (n_face) {   // embed_num_face(quantize_num_faces(n))                     core/models.py:135-139
                const int bucket = face_bucket ? face_bucket[b0 + b] : 0;
                if (bucket < 0 || bucket >= g.num_face_buckets) return fail(ER_ERR_INVALID, "face bucket %d out of range", bucket);
                HIPCHK(hipMemcpyAsync(out_b + (size_t)n_lat * H, c->embed_num_face + (size_t)bucket * H, (size_t)H * 4,
                                      hipMemcpyDeviceToDevice, st));
            }
        }
    }
    return ER_OK;
}

extern "C" int er_embed_tokens(er_ctx* c, const int32_t* ids, int B, int R, float* out, void* stream) {
    if (!c || !ids || !out || B <= 0 || R <= 0) return fail(ER_ERR_INVALID, "er_embed_tokens: bad argument");
    ERCHK(er_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const int H = c->cfg.hidden_dim;
    const int n = B * R;
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= c->cfg.vocab_size) return fail(ER_ERR_INVALID, "token id %d out of range", ids[i]);
    // one gather launch (round 1 issued one hipMemcpyAsync per token: a 2000-token resume prefix was 2000 copies)
    ERCHK(c->e_ids.ensure((size_t)n));
    int* d_ids = c->e_ids.p;
    HIPCHK(hipMemcpyAsync(d_ids, ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPRET(launch_gather_rows(c->embd, d_ids, out, n, H, (long long)H, st));
    HIPCHK(hipStreamSynchronize(st));     // `ids` is caller-owned host memory
    return ER_OK;
}

// ------------------------------------------------------------------------------------ prefill
// Ragged last row tile of the exact prefill (ER_PREFILL_TAIL=0 switches it off): 2050 prefix rows are 32 row tiles of 64
// plus TWO rows, and those two rows cost out_proj / fc2 a fourth round of tiles on 24 CUs (792 tiles of 64 x 64 = 3.09 per CU) and
// fc1 a seventh half round (1584 tiles of 64 x 128 = 6.19 per CU): encode + prefill 42.2 -> 38.2 ms on the same box
// (profiles/r04_prefill_tail.log).  The out_proj / fc1 / fc2 Linears run on the
// first M - M % 64 rows and the 1..8 left-over rows go through the decode step's own fp32 GEMV kernels (one pass over the matrix,
// 5..6 us), whenever that saves a round of 64-row tiles.  Rows are independent in a Linear, so the split needs no sample boundary.
static int prefill_tail_rows(const er_ctx* c, int M) {
    const char* v = getenv("ER_PREFILL_TAIL");
    if ((v && atoi(v) == 0) || c->fast) return 0;
    if (c->cfg.hidden_dim != 1536 || c->cfg.intermediate_dim != 6144) return 0;      // the GEMV kernels are built for these K
    const int tail = M % 64;
    if (tail < 1 || tail > 8 || M < 1024) return 0;
    const long long nt = c->cfg.hidden_dim / 64;
    const long long r_all = ((long long)(M / 64 + 1) * nt + 255) / 256, r_main = ((long long)(M / 64) * nt + 255) / 256;
    return r_all > r_main ? tail : 0;
}
// C[tail rows] = epilogue(A . W^T): dense rows (lda == K, ldc == ldr == N) behind the GEMM's main part
template <int KS, int RW, int EPI>
static hipError_t linear_tail(const float* A, const float* W, const float* bias, float* C, const float* resid, int rows, int N, int K,
                              hipStream_t st) {
    GemvArgs t{};
    t.W = W; t.bias = bias; t.N = N; t.xin = A; t.out = C; t.resid = resid;
    return gemv_groups<float, KS, RW, PRO_NONE, EPI>(t, rows, K, st);
}

// Size checks of a full forward over B x S positions (er_prefill, er_score), before anything is launched.  The prefill kernels index
// their [B * S][width] scratch rows with 32-bit products up to B * S * max(intermediate_dim, 3 * hidden_dim) (fc1's output is the widest):
// such a product must stay below 2^31 (B = 8 at S = 43 011 and intermediate_dim 6144 is 2.11e9 - the edge).
// reserved >= 0 (er_prefill_fork): the pass runs B rows of a cache reserved for `reserved`.
static int forward_check(er_ctx* c, const char* who, const float* embeds, int B, int S, int reserved = -1) {
    if (!c || !embeds || B <= 0 || S <= 0) return fail(ER_ERR_INVALID, "%s: bad argument", who);
    if (c->q.active) return fail(ER_ERR_INVALID, "%s: a queue is open on this context (er_queue_end first)", who);
    ERCHK(er_finalize_weights(c));
    if (reserved < 0) reserved = B;
    if (c->kv->plan.B != reserved) return fail(ER_ERR_INVALID, "%s: batch %d but KV cache reserved for %d (call er_kv_reserve)", who, reserved, c->kv->plan.B);
    if (S >= c->kv->plan.Lcap) return fail(ER_ERR_CAPACITY, "prefix length %d does not fit the reserved KV cache (%d)", S, c->kv->plan.Lcap);
    const long long width = std::max({(long long)c->cfg.intermediate_dim, 3LL * c->cfg.hidden_dim, (long long)c->cfg.vocab_size});
    if ((long long)B * S * width > 0x7fffffffLL)
        return fail(ER_ERR_CAPACITY, "%s: %d x %d positions x %lld columns overflows the 32-bit row indexing of the prefill (split the batch)",
                    who, B, S, width);
    return 0;
}

// all layers over inputs_embeds [B, S, hidden]: K/V into cache positions [0, S), the last layer's pre-LN2 output of EVERY position in
// c->p_y [B * S][hidden], the last position's copy in ypre and the generation state at position S (what er_prefill promises).
// row0 >= 0 with in_queue: the B samples are cache rows [row0, row0 + B) of a larger reservation (er_queue_admit) - the cache base
// pointers move by row0 rows, ypre receives rows [row0, row0 + B), and the generation state is left to the caller, so that no other
// row is touched.
// pos0 > 0 (er_prefill_extend): the S inputs are positions [pos0, pos0 + S) behind a past the cache already holds - position embeddings
// from pos0 + t (modeling_opt.py:345-357 with past_key_values), K/V into cache positions [pos0, pos0 + S) (the cache-writing launches
// take the cache moved on by pos0 rows of a head), every query over keys [0, pos0 + t] (extend_attention), the state at position pos0 + S.
static int extend_attention(er_ctx* c, const float* q, int ldq, const char* kc, const char* vc, float* out, int B, int n_new, int past_len,
                            hipStream_t st);

static int prefill_run(er_ctx* c, const float* embeds, int B, int S, hipStream_t st, int row0 = 0, bool in_queue = false, int pos0 = 0) {
    HIPCHK(hipSetDevice(c->device));
    const DecodePlan& p = c->kv->plan;
    if (!in_queue) c->kv->valid_prefix = 0;      // until this pass has written its positions for every row
    ERCHK(ensure_weight_copies(c, p));
    const er_config& g = c->cfg;
    const int H = g.hidden_dim, I = g.intermediate_dim, NH = g.num_heads, D = c->D;
    const int M = B * S;
    ERCHK(c->p_h.ensure((size_t)M * H));
    ERCHK(c->p_q.ensure((size_t)M * H));
    ERCHK(c->p_a.ensure((size_t)M * H));
    ERCHK(c->p_y.ensure((size_t)M * H));
    ERCHK(c->p_f.ensure((size_t)M * I));
    float *h = c->p_h.p, *q = c->p_q.p, *a = c->p_a.p, *y = c->p_y.p, *f = c->p_f.p;
    // (under prefix groups every row takes the GEMM: the batch's last few positions through the GEMV kernels would give the last row other
    // bits than its group, and the groups rest on same-input rows getting the same bits)
    const int tail = c->kv->prefix_len ? 0 : prefill_tail_rows(c, M), Mm = M - tail;
    // the causal attention of a single prefix is split over two key ranges per query tile (k_flash_attn_f32.h, KSP; same rule as the launcher)
    bool attn_ksplit = false;
    if (!c->fast && !pos0 && flash32_ksplit(S, NH, B, D, true)) {
        ERCHK(c->p_ap.ensure(flash32_part_o_floats(B, NH, S, D)));
        ERCHK(c->p_aml.ensure(flash32_part_ml_floats(B, NH, S)));
        attn_ksplit = true;
    }

    // hidden = inputs_embeds + pos_embeds(pos0 .. pos0 + S)           modeling_opt.py:355-357
    HIPRET(launch_add_pos(embeds, c->posemb, h, B, S, H, pos0, st));
    for (int l = 0; l < g.num_layers; ++l) {
        const LayerW& L = c->layers[l];
        char* kc = c->kv->kc.p + ((long long)l * p.kv_lstride + (long long)row0 * p.kv_bstride) * c->kv_esz;
        char* vc = c->kv->vc.p + ((long long)l * p.kv_lstride + (long long)row0 * p.kv_bstride) * c->kv_esz;
        // where this pass's first position lies in a head's slice: the cache-writing launches index positions from here
        char *kc_new = kc + (long long)pos0 * D * c->kv_esz, *vc_new = vc + (long long)pos0 * D * c->kv_esz;
        if (!c->fast) {
            // q,k,v projections; k,v go straight into the cache layout      modeling_opt.py:185-196
            GemmArgs qa = gemm_args_default();
            qa.A = h; qa.lda = H; qa.B = L.wqkv; qa.ldb = H; qa.bias = L.bqkv; qa.C = q; qa.ldc = H;
            qa.M = M; qa.N = 3 * H; qa.K = H; qa.epi = GEPI_QKV;
            qa.q = q; qa.kcache = (float*)kc_new; qa.vcache = (float*)vc_new; qa.S = S; qa.hidden = H; qa.head_dim = D; qa.l_cap = p.Lcap;
            qa.kv_bstride = p.kv_bstride;
            HIPRET(launch_gemm(qa, 1, st));
            if (pos0) ERCHK(extend_attention(c, q, H, kc, vc, a, B, S, pos0, st));
            else {  // causal attention over the prefix, all samples and heads in one launch   modeling_opt.py:229
                Flash32Args f{};
                f.Q = q; f.ldq = H; f.qs_b = (long long)S * H; f.qs_h = D;
                f.K = (float*)kc; f.ldk = D; f.ks_b = p.kv_bstride; f.ks_h = (long long)p.Lcap * D;
                f.V = (float*)vc; f.ldv = D; f.vs_b = p.kv_bstride; f.vs_h = (long long)p.Lcap * D;
                f.O = a; f.ldo = H; f.os_b = (long long)S * H; f.os_h = D;
                f.N = S; f.M = S; f.sqrt_d = sqrtf((float)D); f.causal_off = 0;
                if (attn_ksplit) { f.part_o = c->p_ap.p; f.part_ml = c->p_aml.p; }
                HIPRET(launch_flash_attn_f32(f, D, true, NH, B, st));
            }
        } else {
            // fast mode: fused projection into fp32 scratch [M][3H]; K/V rounded to the cache dtype (fp16; kv8: e4m3) both in
            // the cache and in the scratch the prefix attention reads
            ERCHK(c->p_qkv.ensure((size_t)M * 3 * H));
            float* qkv = c->p_qkv.p;
            ERCHK(linear_hs(c, h, H, L.wqkv_h, L.bqkv, qkv, 3 * H, M, 3 * H, H, false, nullptr, 0, st));
            // (kv8: bytes into the cache, decode(encode(v)) back into the scratch)
            HIPRET(launch_kv_scatter(qkv, kc_new, vc_new, c->kv8, M, S, H, D, p.Lcap, p.kv_bstride, st));
            if (pos0) ERCHK(extend_attention(c, qkv, 3 * H, kc, vc, a, B, S, pos0, st));
            else {
                Flash32Args f{};
                f.Q = qkv; f.ldq = 3 * H; f.qs_b = (long long)S * 3 * H; f.qs_h = D;
                f.K = qkv + H; f.ldk = 3 * H; f.ks_b = f.qs_b; f.ks_h = D;
                f.V = qkv + 2 * H; f.ldv = 3 * H; f.vs_b = f.qs_b; f.vs_h = D;
                f.O = a; f.ldo = H; f.os_b = (long long)S * H; f.os_h = D;
                f.N = S; f.M = S; f.sqrt_d = sqrtf((float)D); f.causal_off = 0;
                const bool f16s = D == 96 && c->knobs.prefill_attn_f16s != 0;
                if (f16s) HIPRET(launch_flash_attn_f16s(f, D, true, NH, B, st));   // K / V in the scratch are fp16 values already
                else HIPRET(launch_flash_attn_f32(f, D, true, NH, B, st));
            }
        }
        // y = h + out_proj(a); h1 = LN1(y)                               modeling_opt.py:232, 272-274
        const bool hs = c->fast;
        if (hs) ERCHK(linear_hs(c, a, H, L.wo_h, L.bo, y, H, M, H, H, false, h, H, st));
        else {
            HIPRET(linear(a, H, L.wo, L.bo, y, H, Mm, H, H, false, h, H, st));
            if (tail) HIPRET((linear_tail<1, 1, EPI_RESID>(a + (size_t)Mm * H, L.wo, L.bo, y + (size_t)Mm * H, h + (size_t)Mm * H, tail, H, H, st)));
        }
        HIPRET(launch_layernorm(y, L.ln1w, L.ln1b, h, M, H, H, H, g.ln_eps, st));
        // y = h1 + fc2(relu(fc1(h1))); h = LN2(y)                        modeling_opt.py:281-288
        if (hs) {
            ERCHK(linear_hs(c, h, H, L.w1_h, L.b1, f, I, M, I, H, true, nullptr, 0, st));
            ERCHK(linear_hs(c, f, I, L.w2_h, L.b2, y, H, M, H, I, false, h, H, st));
        } else {
            HIPRET(linear(h, H, L.w1, L.b1, f, I, Mm, I, H, true, nullptr, 0, st));
            if (tail) HIPRET((linear_tail<1, 2, EPI_RELU>(h + (size_t)Mm * H, L.w1, L.b1, f + (size_t)Mm * I, nullptr, tail, I, H, st)));
            HIPRET(linear(f, I, L.w2, L.b2, y, H, Mm, H, I, false, h, H, st));
            if (tail) HIPRET((linear_tail<4, 2, EPI_RESID>(f + (size_t)Mm * I, L.w2, L.b2, y + (size_t)Mm * H, h + (size_t)Mm * H, tail, H, I, st)));
        }
        if (l + 1 < g.num_layers) HIPRET(launch_layernorm(y, L.ln2w, L.ln2b, h, M, H, H, H, g.ln_eps, st));
    }
    // keep the last position's pre-LN2 state: the decode head applies LN2 + lm_head to it
    for (int b = 0; b < B; ++b)
        HIPCHK(hipMemcpyAsync(c->kv->ypre.p + (size_t)(row0 + b) * H, y + ((size_t)b * S + S - 1) * H, (size_t)H * 4, hipMemcpyDeviceToDevice, st));
    if (in_queue) return ER_OK;
    hipLaunchKernelGGL(init_state_kernel, dim3((B + 63) / 64), dim3(64), 0, st, c->kv->st, B, pos0 + S);
    HIPRET(hipGetLastError());
    c->base_pos = pos0 + S;
    c->kv->valid_prefix = pos0 + S;
    c->have_hidden = true;
    return ER_OK;
}

// Behind a prefill with prefix groups: every follower's K/V [0, P) of all layers against its leader's, bit for bit, on the device.  Wrong
// groups must be loud: the step would read the leader's prefix for a row that never had it.
static int prefix_groups_check(er_ctx* c, hipStream_t st) {
    KvMem& kv = *c->kv;
    const DecodePlan& p = kv.plan;
    const int followers = (int)kv.grp_followers.n;
    if (!followers) return ER_OK;
    PrefixCheckArgs a{};
    a.kc = kv.kc.p; a.vc = kv.vc.p; a.followers = kv.grp_followers.p; a.leader = kv.grp_leader_dev.p;
    a.head_bytes = (long long)p.Lcap * c->D * c->kv_esz; a.row_bytes = p.kv_bstride * c->kv_esz; a.layer_bytes = p.kv_lstride * c->kv_esz;
    a.prefix_vecs = (long long)kv.prefix_len * c->D * c->kv_esz / 16;
    a.layers = p.layers; a.first = kv.grp_first.p;
    HIPCHK(hipMemsetAsync(kv.grp_first.p, 0x7f, sizeof(int), st));
    HIPRET(launch_prefix_check(a, c->cfg.num_heads, followers, st));
    int first = 0;
    HIPCHK(hipMemcpyAsync(&first, kv.grp_first.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (first != 0x7f7f7f7f) {
        c->have_hidden = false;
        const int row = first / p.layers, layer = first % p.layers;
        return fail(ER_ERR_INVALID, "er_prefill: prefix groups: the first %d cache positions of row %d differ from those of its leader, row %d, in layer %d "
                    "(rows of one group need the same prefix; prefill again)", kv.prefix_len, row, kv.grp_leader[row], layer);
    }
    return ER_OK;
}

extern "C" int er_prefill(er_ctx* c, const float* embeds, int B, int S, void* stream) {
    ERCHK(forward_check(c, "er_prefill", embeds, B, S));
    if (c->kv->prefix_len > S) return fail(ER_ERR_INVALID, "er_prefill: %d positions but the prefix groups share %d", S, c->kv->prefix_len);
    c->kv->row_class = false;                  // er_feed / er_logits after this prefill run the plan's own kinds; er_decode chooses again
    ERCHK(prefill_run(c, embeds, B, S, pick(c, stream)));
    return c->kv->prefix_len ? prefix_groups_check(c, pick(c, stream)) : ER_OK;
}

// ------------------------------------------------------------------------------------ prefill with a past
// One layer's attention of n_new new positions per row behind past_len cached ones: query (b, t) at q[(b * n_new + t) * ldq + h * D]
// over keys [0, past_len + t] of row b's cache slice (kc / vc: this layer's, at the pass's first row), out rows [B * n_new][hidden].
// The new positions' K/V are in the cache when this runs.  The route is extend_attn_route (er_extend_plan.h; ER_EXTEND_ATTN, read
// per call: the tests and the bench compare both routes in one process).
static int extend_attention(er_ctx* c, const float* q, int ldq, const char* kc, const char* vc, float* out, int B, int n_new, int past_len,
                            hipStream_t st) {
    const DecodePlan& p = c->kv->plan;
    const int H = c->cfg.hidden_dim, NH = c->cfg.num_heads, D = c->D, T = past_len + n_new;
    if (extend_attn_route(n_new, attn_extend_supported(D, c->kv_type), getenv("ER_EXTEND_ATTN")) == EXTEND_ROWS) {
        ERCHK(c->p_ap.ensure(attn_extend_part_floats(B, n_new, NH, T, D)));
        AttnExtendArgs a{};
        a.q = q; a.ldq = ldq; a.kcache = kc; a.vcache = vc; a.part = c->p_ap.p; a.out = out; a.ldo = H;
        a.H = NH; a.l_cap = p.Lcap; a.S = attn_extend_chunks(T); a.past_len = past_len; a.n_new = n_new;
        a.kv_bstride = p.kv_bstride; a.sqrt_d = sqrtf((float)D);
        HIPRET(launch_attn_extend(a, D, c->kv_type, B, st));
        return ER_OK;
    }
    Flash32Args f{};
    f.Q = q; f.ldq = ldq; f.qs_b = (long long)n_new * ldq; f.qs_h = D;
    f.O = out; f.ldo = H; f.os_b = (long long)n_new * H; f.os_h = D;
    f.N = n_new; f.M = T; f.sqrt_d = sqrtf((float)D); f.causal_off = past_len;
    if (!c->fast) {         // the fp32 cache in place
        f.K = (const float*)kc; f.ldk = D; f.ks_b = p.kv_bstride; f.ks_h = (long long)p.Lcap * D;
        f.V = (const float*)vc; f.ldv = D; f.vs_b = p.kv_bstride; f.vs_h = (long long)p.Lcap * D;
        HIPRET(launch_flash_attn_f32(f, D, true, NH, B, st));
        return ER_OK;
    }
    // fast / kv8 mode: the fast prefill's kernels read fp32 rows - positions [0, T) of the cache, exact in fp32, gathered into scratch
    ERCHK(c->p_kx.ensure((size_t)B * T * 2 * H));
    float* kx = c->p_kx.p;
    HIPRET(launch_kv_gather(kc, vc, kx, c->kv8, B * T, T, H, D, p.Lcap, p.kv_bstride, st));
    f.K = kx; f.ldk = 2 * H; f.ks_b = (long long)T * 2 * H; f.ks_h = D;
    f.V = kx + H; f.ldv = 2 * H; f.vs_b = f.ks_b; f.vs_h = D;
    const bool f16s = D == 96 && c->knobs.prefill_attn_f16s != 0;
    if (f16s) HIPRET(launch_flash_attn_f16s(f, D, true, NH, B, st));
    else HIPRET(launch_flash_attn_f32(f, D, true, NH, B, st));
    return ER_OK;
}

extern "C" int er_prefill_extend(er_ctx* c, const float* embeds, int B, int past_len, int n_new, void* stream) {
    if (!c || !embeds || B <= 0 || n_new <= 0 || past_len <= 0) return fail(ER_ERR_INVALID, "er_prefill_extend: bad argument");
    if (past_len > 0x3fffffff - n_new) return fail(ER_ERR_CAPACITY, "er_prefill_extend: past_len %d + n_new %d", past_len, n_new);
    // the forward pass's own checks at the length the cache will hold, and its 32-bit row rule over the rows this pass runs
    ERCHK(forward_check(c, "er_prefill_extend", embeds, B, past_len + n_new));
    KvMem& kv = *c->kv;
    if (past_len + n_new > c->cfg.max_positions) return fail(ER_ERR_CAPACITY, "er_prefill_extend: position table exhausted (%d)", c->cfg.max_positions);
    const int valid = c->have_hidden ? kv.valid_prefix : 0;
    switch (extend_past_check(past_len, valid, kv.prefix_len)) {
        case 1:
            return fail(ER_ERR_INVALID, "er_prefill_extend: past_len %d outside the prefix this reservation holds for all rows, [1, %d] (%s)", past_len, valid,
                        valid ? "positions behind it are rewritten, positions beyond it were never prefilled" : "call er_prefill first");
        case 2:
            return fail(ER_ERR_INVALID, "er_prefill_extend: past_len %d is below the %d positions the prefix groups share (keep the shared prefix, or clear the groups)",
                        past_len, kv.prefix_len);
    }
    if ((long long)B * (past_len + n_new) > 0x7fffffffLL)
        return fail(ER_ERR_CAPACITY, "er_prefill_extend: %d x %d positions overflow the 32-bit row indexing of the K/V gather (split the batch)", B, past_len + n_new);
    kv.row_class = false;                      // as er_prefill
    ERCHK(prefill_run(c, embeds, B, n_new, pick(c, stream), 0, false, past_len));
    return ER_OK;
}

// rows of the embed_num_face table (core/models.py:137): what encode_cond appends behind the cloud's tokens, without the point encoder
extern "C" int er_embed_num_face(er_ctx* c, const int32_t* face_bucket, int B, float* out, void* stream) {
    if (!c || !face_bucket || !out || B <= 0) return fail(ER_ERR_INVALID, "er_embed_num_face: bad argument");
    if (c->cfg.num_face_buckets == 0) return fail(ER_ERR_UNSUPPORTED, "er_embed_num_face: the model has no face-count condition (num_face_buckets == 0)");
    ERCHK(er_finalize_weights(c));
    for (int b = 0; b < B; ++b)
        if (face_bucket[b] < 0 || face_bucket[b] >= c->cfg.num_face_buckets)
            return fail(ER_ERR_INVALID, "er_embed_num_face: bucket %d outside [0, %d)", face_bucket[b], c->cfg.num_face_buckets);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    ERCHK(c->e_ids.ensure((size_t)B));
    HIPCHK(hipMemcpyAsync(c->e_ids.p, face_bucket, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    HIPRET(launch_gather_rows(c->embed_num_face, c->e_ids.p, out, B, c->cfg.hidden_dim, (long long)c->cfg.hidden_dim, st));
    HIPCHK(hipStreamSynchronize(st));     // `face_bucket` is caller-owned host memory
    return ER_OK;
}

// ------------------------------------------------------------------------------------ forked prefill
// What a fork launch needs of its arguments, before anything is launched: rows inside the batch, no destination that is also a source or
// named twice, len inside the cache, a slab of whole 16-byte pieces at 16-byte aligned bases.
static int kv_fork_check(const char* who, const void* kc, const void* vc, int esz, int layers, int B, int H, int Lcap, int D,
                         const int32_t* src, const int32_t* dst, int n_pairs, int len) {
    if (!kc || !vc || !src || !dst || layers < 1 || B < 1 || H < 1 || Lcap < 1 || D < 1 || n_pairs < 1) return fail(ER_ERR_INVALID, "%s: bad argument", who);
    if (esz != 1 && esz != 2 && esz != 4) return fail(ER_ERR_INVALID, "%s: element size %d is not 1, 2 or 4", who, esz);
    if (len < 1 || len > Lcap) return fail(ER_ERR_INVALID, "%s: len %d outside [1, %d]", who, len, Lcap);
    if (((long long)len * D * esz) % 16 || ((long long)Lcap * D * esz) % 16 || ((uintptr_t)kc | (uintptr_t)vc) % 16)
        return fail(ER_ERR_INVALID, "%s: a head's first %d positions (%lld bytes of %lld) are not whole 16-byte pieces at a 16-byte aligned base", who, len,
                    (long long)len * D * esz, (long long)Lcap * D * esz);
    std::vector<char> is_src((size_t)B, 0), is_dst((size_t)B, 0);
    for (int i = 0; i < n_pairs; ++i) {
        if (src[i] < 0 || src[i] >= B || dst[i] < 0 || dst[i] >= B) return fail(ER_ERR_INVALID, "%s: pair %d (%d -> %d) outside the %d rows", who, i, src[i], dst[i], B);
        is_src[(size_t)src[i]] = 1;
    }
    for (int i = 0; i < n_pairs; ++i) {
        if (is_src[(size_t)dst[i]]) return fail(ER_ERR_INVALID, "%s: row %d is a destination and a source", who, dst[i]);
        if (is_dst[(size_t)dst[i]]) return fail(ER_ERR_INVALID, "%s: row %d is a destination twice", who, dst[i]);
        is_dst[(size_t)dst[i]] = 1;
    }
    return ER_OK;
}

static KvForkArgs kv_fork_args(void* kc, void* vc, int esz, int B, int H, int Lcap, int D, int len) {
    KvForkArgs a{};
    a.kc = (char*)kc; a.vc = (char*)vc;
    a.head_bytes = (long long)Lcap * D * esz; a.row_bytes = a.head_bytes * H; a.layer_bytes = a.row_bytes * B;
    a.slab_vecs = (long long)len * D * esz / 16;
    return a;
}

// The launch on caller-owned caches.  It does not block and allocates nothing (the table travels in the kernel arguments), so it can be
// captured in a graph.
extern "C" int er_k_kv_fork(void* kc, void* vc, int esz, int layers, int B, int H, int Lcap, int D, const int32_t* src, const int32_t* dst,
                            int n_pairs, int len, void* stream) {
    ERCHK(kv_fork_check("er_k_kv_fork", kc, vc, esz, layers, B, H, Lcap, D, src, dst, n_pairs, len));
    HIPRET(launch_kv_fork(kv_fork_args(kc, vc, esz, B, H, Lcap, D, len), H, layers, src, dst, n_pairs, (hipStream_t)stream));
    return ER_OK;
}

// er_prefill for a batch whose rows [n_leaders, n) repeat rows [0, n_leaders): the forward pass runs over the leaders alone, every follower
// receives its leader's K/V [0, S) (kv_fork_kernel) and ypre row, and the generation state of all n rows starts at position S.  With prefix
// groups set to the same table prefix_groups_check is NOT run: it compares a follower's [0, P) with its leader's, which here are the
// bytes kv_fork_kernel has just copied from there.
extern "C" int er_prefill_fork(er_ctx* c, const float* embeds, int n_leaders, int S, const int32_t* leader, int n, void* stream) {
    if (!c || !leader || n <= 0) return fail(ER_ERR_INVALID, "er_prefill_fork: bad argument");
    ERCHK(forward_check(c, "er_prefill_fork", embeds, n_leaders, S, n));
    if (n_leaders > n) return fail(ER_ERR_INVALID, "er_prefill_fork: %d leaders for a batch of %d rows", n_leaders, n);
    for (int b = 0; b < n; ++b)
        if (b < n_leaders ? leader[b] != b : (leader[b] < 0 || leader[b] >= n_leaders))
            return fail(ER_ERR_INVALID, "er_prefill_fork: leader[%d] = %d (leaders first: leader[b] == b below %d, a row below %d behind them)", b, leader[b], n_leaders, n_leaders);
    KvMem& kv = *c->kv;
    if (kv.prefix_len > S) return fail(ER_ERR_INVALID, "er_prefill_fork: %d positions but the prefix groups share %d", S, kv.prefix_len);
    if (kv.prefix_len && !std::equal(kv.grp_leader.begin(), kv.grp_leader.end(), leader))
        return fail(ER_ERR_INVALID, "er_prefill_fork: prefix groups are set with another leader table (set the groups from the table of the fork)");
    const DecodePlan& p = kv.plan;
    std::vector<int32_t> src, dst;
    for (int b = n_leaders; b < n; ++b) { src.push_back(leader[b]); dst.push_back(b); }
    if (!src.empty()) ERCHK(kv_fork_check("er_prefill_fork", kv.kc.p, kv.vc.p, c->kv_esz, p.layers, n, c->cfg.num_heads, p.Lcap, c->D, src.data(), dst.data(), (int)src.size(), S));
    kv.row_class = false;                      // as er_prefill
    hipStream_t st = pick(c, stream);
    ERCHK(prefill_run(c, embeds, n_leaders, S, st));
    if (src.empty()) return ER_OK;
    c->have_hidden = false;                    // until the followers hold their state
    HIPRET(launch_kv_fork(kv_fork_args(kv.kc.p, kv.vc.p, c->kv_esz, n, c->cfg.num_heads, p.Lcap, c->D, S), c->cfg.num_heads, p.layers, src.data(), dst.data(), (int)src.size(), st));
    const size_t H = (size_t)c->cfg.hidden_dim;
    for (int b = n_leaders; b < n; ++b)
        HIPCHK(hipMemcpyAsync(kv.ypre.p + (size_t)b * H, kv.ypre.p + (size_t)leader[b] * H, H * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(init_state_kernel, dim3((n + 63) / 64), dim3(64), 0, st, kv.st, n, S);
    HIPRET(hipGetLastError());
    c->have_hidden = true;
    return ER_OK;
}

// ------------------------------------------------------------------------------------ prefix groups
extern "C" int er_set_prefix_groups(er_ctx* c, const int32_t* leader, int n, int prefix_len) {
    if (!c) return fail(ER_ERR_INVALID, "er_set_prefix_groups: null context");
    KvMem& kv = *c->kv;
    const int B = kv.plan.B;
    if (B <= 0) return fail(ER_ERR_INVALID, "er_set_prefix_groups: no cache reserved (call er_kv_reserve)");
    if (c->q.active) return fail(ER_ERR_INVALID, "er_set_prefix_groups: a queue is open on this context (er_queue_end first)");
    const bool clear = !leader || prefix_len == 0;
    if (clear && !kv.prefix_len) return ER_OK;
    if (!clear && c->kv8) return fail(ER_ERR_UNSUPPORTED, "er_set_prefix_groups: the shared-prefix kernels read fp32 and fp16 caches only; this context keeps an e4m3 cache (kv8)");
    std::vector<int> rows, off, followers;
    if (!clear) {
        if (n != B) return fail(ER_ERR_INVALID, "er_set_prefix_groups: %d leaders for a batch of %d rows", n, B);
        if (prefix_len < 1 || prefix_len >= kv.plan.Lcap) return fail(ER_ERR_INVALID, "er_set_prefix_groups: prefix_len %d outside [1, %d)", prefix_len, kv.plan.Lcap);
        for (int b = 0; b < B; ++b) {
            if (leader[b] < 0 || leader[b] > b) return fail(ER_ERR_INVALID, "er_set_prefix_groups: leader[%d] = %d outside [0, %d]", b, leader[b], b);
            if (leader[leader[b]] != leader[b]) return fail(ER_ERR_INVALID, "er_set_prefix_groups: leader[%d] = %d is itself led by row %d (name the group's lowest row)", b, leader[b], leader[leader[b]]);
        }
        if (!shared_attn_supported(kv.plan.sel, c->D))
            return fail(ER_ERR_UNSUPPORTED, "er_set_prefix_groups: prefix groups need the batched decode path (B > 4 or ER_FORCE_BATCHED=1) and head_dim 96; reserved: %d rows, head_dim %d", B, c->D);
        for (int b = 0; b < B; ++b) {
            if (leader[b] != b) { followers.push_back(b); continue; }
            off.push_back((int)rows.size());
            for (int r = b; r < B; ++r) if (leader[r] == b) rows.push_back(r);      // the leader first, then its followers in row order
        }
        off.push_back((int)rows.size());
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());           // a running step still reads the old tables
    kv.drop_steps();                          // the next step is captured with the new launches
    const er_config& g = c->cfg;
    kv.plan = make_decode_plan(c->knobs, kv.plan.rk, c->fast, B, kv.plan.Lcap, g.num_layers, g.num_heads, c->D, g.hidden_dim, attn_chunking(g.num_heads), !clear, c->kv8);
    c->have_hidden = false;                   // groups come before the prefill whose cache they describe
    kv.prefix_len = 0; kv.n_groups = 0; kv.grp_leader.clear();
    kv.grp_followers = DevBuf<int>();
    if (clear) return ER_OK;
    ERCHK(kv.grp_rows.ensure(rows.size()));
    ERCHK(kv.grp_off.ensure(off.size()));
    ERCHK(kv.grp_leader_dev.ensure((size_t)B));
    ERCHK(kv.grp_first.ensure(1));
    if (!followers.empty()) ERCHK(kv.grp_followers.ensure(followers.size()));
    HIPCHK(hipMemcpy(kv.grp_rows.p, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(kv.grp_off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(kv.grp_leader_dev.p, leader, (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    if (!followers.empty()) HIPCHK(hipMemcpy(kv.grp_followers.p, followers.data(), followers.size() * sizeof(int), hipMemcpyHostToDevice));
    kv.grp_leader.assign(leader, leader + B);
    kv.n_groups = (int)off.size() - 1;
    kv.prefix_len = prefix_len;
    return ER_OK;
}

// The prefix pass of the next grouping: a knob of the context, read by make_decode_plan when er_set_prefix_groups derives the plan again
// (the plan and the captured step of groups that are set now stay as they are until then).
extern "C" int er_set_prefix_pass(er_ctx* c, int pass) {
    if (!c) return fail(ER_ERR_INVALID, "er_set_prefix_pass: null context");
    if (pass != ER_PREFIX_PASS_VALU && pass != ER_PREFIX_PASS_MFMA) return fail(ER_ERR_INVALID, "er_set_prefix_pass: pass %d is neither ER_PREFIX_PASS_VALU nor ER_PREFIX_PASS_MFMA", pass);
    if (c->q.active) return fail(ER_ERR_INVALID, "er_set_prefix_pass: a queue is open on this context (er_queue_end first)");
    if (pass == ER_PREFIX_PASS_MFMA && (c->kv_type != 1 || c->D != 96))
        return fail(ER_ERR_UNSUPPORTED, "er_set_prefix_pass: the matrix-core prefix pass reads fp16 caches at head_dim 96 only; this context keeps %s at head_dim %d",
                    c->kv_type == 0 ? "an fp32 cache" : c->kv_type == 1 ? "an fp16 cache" : "an e4m3 cache (kv8)", c->D);
    c->knobs.prefix_pass = pass;
    return ER_OK;
}

// ------------------------------------------------------------------------------------ scoring (LMM.forward, eval mode)
extern "C" int er_score(er_ctx* c, const float* embeds, const int32_t* labels, int B, int S, float* nll_out, int32_t* pred_out,
                        float* logits_out, float* loss_out, void* stream) {
    ERCHK(forward_check(c, "er_score", embeds, B, S));
    if (c->kv->prefix_len) return fail(ER_ERR_INVALID, "er_score: prefix groups are set on this context (clear them with er_set_prefix_groups(ctx, NULL, 0, 0))");
    if (!labels || !nll_out || !loss_out) return fail(ER_ERR_INVALID, "er_score: labels, nll_out and loss_out are required");
    c->kv->row_class = false;                  // as er_prefill
    hipStream_t st = pick(c, stream);
    ERCHK(prefill_run(c, embeds, B, S, st));
    const er_config& g = c->cfg;
    const int H = g.hidden_dim, V = g.vocab_size, M = B * S;
    const LayerW& last = c->layers[g.num_layers - 1];
    // final LayerNorm of every position (the prefill leaves the last layer's LN2 to the head), into p_h: free once the layers ran
    HIPRET(launch_layernorm(c->p_y.p, last.ln2w, last.ln2b, c->p_h.p, M, H, H, H, g.ln_eps, st));
    float* lg = logits_out;
    if (!lg) {
        ERCHK(c->s_lg.ensure((size_t)M * V));
        lg = c->s_lg.p;
    }
    // lm_head over every position (modeling_opt.py:497): the prefill's own Linears, fp32 or fp16-stored weights (fp32-grade activations)
    if (c->fast) ERCHK(linear_hs(c, c->p_h.p, H, c->lm_head_h, nullptr, lg, V, M, V, H, false, nullptr, 0, st));
    else HIPRET(linear(c->p_h.p, H, c->lm_head, nullptr, lg, V, M, V, H, false, nullptr, 0, st));
    HIPRET(launch_score_rows(lg, labels, M, S, V, nll_out, pred_out, st));
    HIPRET(launch_score_reduce(nll_out, labels, M, S, loss_out, st));
    return ER_OK;
}

extern "C" int er_point_latent(er_ctx* c, const float* conds, int B, int n_points, float* latent_out, float* kl_out, void* stream) {
    if (!c || !conds || !latent_out || B <= 0) return fail(ER_ERR_INVALID, "er_point_latent: bad argument");
    if (c->cfg.cond_mode != ER_COND_POINT) return fail(ER_ERR_UNSUPPORTED, "er_point_latent: the context has no point encoder (cond_mode %d)", c->cfg.cond_mode);
    ERCHK(er_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    ERCHK(pe_latent(c->pe, conds, B, n_points, latent_out, st, "er_point_latent"));
    const size_t n = (size_t)B * c->pe.Lq * c->pe.LD;
    if (kl_out) HIPRET(launch_score_reduce(latent_out, nullptr, (int)n, 0, kl_out, st));
    return ER_OK;
}

extern "C" int er_set_point_encoder_mode(er_ctx* c, int mode) {
    if (!c) return fail(ER_ERR_INVALID, "null ctx");
    if (c->cfg.cond_mode != ER_COND_POINT)
        return fail(ER_ERR_UNSUPPORTED, "er_set_point_encoder_mode: the context has no point encoder (cond_mode %d)", c->cfg.cond_mode);
    return pe_attach(c->w, c->pe, mode, "er_set_point_encoder_mode", "");
}

extern "C" int er_logits(er_ctx* c, float* out, void* stream) {
    if (!c || !out) return fail(ER_ERR_INVALID, "er_logits: bad argument");
    if (!c->have_hidden) return fail(ER_ERR_INVALID, "er_logits: no forward pass has run (call er_prefill)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    HIPRET(launch_kind(c, 6, 0, st, nullptr, 0));
    HIPCHK(hipMemcpyAsync(out, c->kv->logits.p, (size_t)c->kv->plan.B * c->cfg.vocab_size * 4, hipMemcpyDeviceToDevice, st));
    return ER_OK;
}

static int check_room(er_ctx* c, int extra) {
    // generated token t is fed at position base_pos + t
    HIPCHK(hipMemcpy(c->h_pinned, c->kv->st.ngen, sizeof(int), hipMemcpyDeviceToHost));
    const int used = c->base_pos + c->h_pinned[0];
    if (used + extra > c->kv->plan.Lcap) return fail(ER_ERR_CAPACITY, "KV cache full: %d + %d > %d", used, extra, c->kv->plan.Lcap);
    if (used + extra > c->cfg.max_positions) return fail(ER_ERR_CAPACITY, "position table exhausted (%d)", c->cfg.max_positions);
    return 0;
}

extern "C" int er_feed(er_ctx* c, const int32_t* ids, void* stream) {
    if (!c || !ids) return fail(ER_ERR_INVALID, "er_feed: bad argument");
    if (!c->have_hidden) return fail(ER_ERR_INVALID, "er_feed: call er_prefill first");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    HIPCHK(hipStreamSynchronize(st));
    ERCHK(check_room(c, 1));
    const int B = c->kv->plan.B;
    for (int b = 0; b < B; ++b) {
        if (ids[b] < 0 || ids[b] >= c->cfg.vocab_size) return fail(ER_ERR_INVALID, "token id %d out of range", ids[b]);
        c->h_pinned[b] = ids[b];
    }
    HIPCHK(hipMemcpyAsync(c->kv->d_ids_tmp.p, c->h_pinned, B * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(force_token_kernel, dim3((B + 63) / 64), dim3(64), 0, st, c->kv->d_ids_tmp.p, c->kv->st, B);
    HIPRET(hipGetLastError());
    HIPRET(enqueue_layers(c, st));
    HIPCHK(hipStreamSynchronize(st));   // h_pinned may be reused by the next call
    return ER_OK;
}

// ------------------------------------------------------------------------------------ generation loop
__global__ void fill_i64_kernel(long long* p, long long n, long long v) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void reset_gen_kernel(GenState st, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) { *st.n_unfinished = B; *st.error = 0; }
    if (b >= B) return;
    st.counter[b] = 0; st.unfinished[b] = 1; st.eos_step[b] = -1;
}

// one step = lm_head -> sampling head -> 24 layers on the chosen token; captured once per reserved shape, replayed by er_decode and
// er_queue_run
static int ensure_step_graph(er_ctx* c) {
    KvMem& kv = *c->kv;
    if (!c->knobs.use_graph) return 0;
    // the step that ends in the head with controls is a capture of its own; one taken without the log-prob tables is taken again with them
    if (kv.head_ctl && kv.step_exec_ctl && kv.ctl_exec_lp != kv.lp_on) { hipGraphExecDestroy(kv.step_exec_ctl); kv.step_exec_ctl = nullptr; }
    hipGraphExec_t* slot = kv.head_ctl ? &kv.step_exec_ctl : &kv.step_exec;
    if (*slot) return 0;
    const int Lcap = c->kv->plan.Lcap;
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(c->own_stream, hipStreamCaptureModeRelaxed));
    hipError_t e = enqueue_step(c, c->own_stream, c->kv->d_out_ids.p, Lcap);
    hipError_t e2 = hipStreamEndCapture(c->own_stream, &graph);
    if (e != hipSuccess || e2 != hipSuccess) {
        if (graph) hipGraphDestroy(graph);
        return fail(ER_ERR_HIP, "graph capture failed: %s / %s", hipGetErrorString(e), hipGetErrorString(e2));
    }
    HIPCHK(hipGraphInstantiate(slot, graph, nullptr, nullptr, 0));
    hipGraphDestroy(graph);
    if (kv.head_ctl) kv.ctl_exec_lp = kv.lp_on;
    return 0;
}
static hipGraphExec_t step_graph(er_ctx* c) { return c->kv->head_ctl ? c->kv->step_exec_ctl : c->kv->step_exec; }

// What er_decode and er_queue_begin make of er_decode_params.top_k and the context's er_sampling: the top_k the head works with, which
// head ends the step, the device copy of the controls and the log-prob tables.
static int head_setup(er_ctx* c, const er_decode_params* p, int* top_k) {
    KvMem& kv = *c->kv;
    const er_sampling& s = c->samp;
    *top_k = s.top_k_set ? s.top_k : p->top_k;
    if (p->mode == ER_SAMPLE && !s.top_k_set && p->top_k <= 0) return fail(ER_ERR_INVALID, "top_k must be > 0 in sample mode");
    const bool sample = p->mode == ER_SAMPLE;
    kv.lp_on = s.logprobs != 0;
    kv.lp_valid = false;
    kv.row_class = kv.lp_on;
    kv.head_ctl = kv.lp_on || (sample && (s.temperature != 1.0f || s.top_p != 1.0f || *top_k <= 0));
    if (!kv.head_ctl) return 0;
    if (kv.lp_on) {
        const size_t n = (size_t)kv.plan.B * kv.plan.Lcap;
        ERCHK(kv.d_lp_model.ensure(n));
        ERCHK(kv.d_lp_policy.ensure(n));
    }
    const HeadCtlDev h{s.temperature, s.top_p};
    HIPCHK(hipMemcpy(kv.d_ctl.p, &h, sizeof(h), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int er_decode(er_ctx* c, const er_decode_params* p, int64_t* out_ids, int32_t* n_steps, void* stream) {
    if (!c || !p || !out_ids || !n_steps) return fail(ER_ERR_INVALID, "er_decode: bad argument");
    if (!c->have_hidden) return fail(ER_ERR_INVALID, "er_decode: call er_prefill first");
    if (p->max_new_tokens <= 0) return fail(ER_ERR_INVALID, "max_new_tokens must be > 0");
    if (p->mode != ER_GREEDY && p->mode != ER_SAMPLE) return fail(ER_ERR_INVALID, "bad mode");
    if (p->grammar < 0 || p->grammar > 2) return fail(ER_ERR_INVALID, "bad grammar");
    if (p->mode == ER_SAMPLE && !c->samp.top_k_set && p->top_k <= 0) return fail(ER_ERR_INVALID, "top_k must be > 0 in sample mode");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const int B = c->kv->plan.B, Lcap = c->kv->plan.Lcap, T = p->max_new_tokens;
    HIPCHK(hipStreamSynchronize(st));
    ERCHK(check_room(c, T));
    if (c->h_pinned[0] != 0) return fail(ER_ERR_INVALID, "er_decode must directly follow er_prefill (%d tokens already fed)", c->h_pinned[0]);
    int top_k = 0;
    ERCHK(head_setup(c, p, &top_k));

    const DecodeParamsDev dp = decode_params_dev(*p, top_k, T, c->cfg.eos_token_id, c->cfg.pad_token_id, c->cfg.vocab_size);
    HIPCHK(hipMemcpy(c->kv->d_params.p, &dp, sizeof(dp), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(reset_gen_kernel, dim3((B + 63) / 64), dim3(64), 0, st, c->kv->st, B);
    HIPRET(hipGetLastError());
    hipLaunchKernelGGL(fill_i64_kernel, dim3(ew_grid((long long)B * Lcap)), dim3(ER_WG), 0, st, c->kv->d_out_ids.p,
                       (long long)B * Lcap, (long long)dp.pad);
    HIPRET(hipGetLastError());

    ERCHK(ensure_step_graph(c));

    const int check_every = 32;
    int steps_run = 0;
    HIPCHK(hipEventRecord(c->ev0, st));
    for (int t = 0; t < T; ++t) {
        if (c->knobs.use_graph) HIPCHK(hipGraphLaunch(step_graph(c), st));
        else HIPRET(enqueue_step(c, st, c->kv->d_out_ids.p, Lcap));
        steps_run = t + 1;
        if (steps_run >= p->min_new_tokens && steps_run < T && (steps_run % check_every) == 0) {
            HIPCHK(hipMemcpyAsync(c->h_pinned, c->kv->st.n_unfinished, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (c->h_pinned[0] <= 0) break;
        }
    }
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipMemcpy2DAsync(out_ids, (size_t)T * sizeof(long long), c->kv->d_out_ids.p, (size_t)Lcap * sizeof(long long),
                            (size_t)T * sizeof(long long), B, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(c->h_pinned, c->kv->st.eos_step, B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c->h_pinned + B, c->kv->st.error, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&c->last_decode_ms, c->ev0, c->ev1));
    if (c->h_pinned[B] != 0)
        return fail(ER_ERR_INVALID, "er_decode: a row had no finite candidate score (non-finite logits); HF would raise in multinomial/argmax");
    // HF returns as many columns as steps it ran: it stops right after the step in which the last row emits EOS
    int last = -1;
    bool finished = true;
    for (int b = 0; b < B; ++b) {
        if (c->h_pinned[b] < 0) finished = false;
        else if (c->h_pinned[b] > last) last = c->h_pinned[b];
    }
    *n_steps = finished ? last + 1 : T;
    if (!finished && steps_run < T) return fail(ER_ERR_INVALID, "internal: stopped early with unfinished rows");
    c->kv->lp_valid = c->kv->lp_on;
    return ER_OK;
}

extern "C" int er_set_sampling(er_ctx* c, const er_sampling* s) {
    if (!c) return fail(ER_ERR_INVALID, "er_set_sampling: null context");
    const er_sampling dflt{1.0f, 1.0f, 0, 0, 0};
    if (!s) s = &dflt;
    if (!(s->temperature > 0.0f) || !(s->temperature <= 3.402823466e38f))
        return fail(ER_ERR_INVALID, "er_set_sampling: temperature %g is not a finite number > 0", (double)s->temperature);
    if (!(s->top_p > 0.0f) || !(s->top_p <= 1.0f)) return fail(ER_ERR_INVALID, "er_set_sampling: top_p %g outside (0, 1]", (double)s->top_p);
    if (s->top_k_set && s->top_k < 0) return fail(ER_ERR_INVALID, "er_set_sampling: top_k %d is negative", s->top_k);
    if (c->q.active) return fail(ER_ERR_INVALID, "er_set_sampling: a queue is open on this context (er_queue_begin read the controls; er_queue_end first)");
    c->samp = *s;
    c->samp.top_k_set = s->top_k_set ? 1 : 0;
    if (!c->samp.top_k_set) c->samp.top_k = 0;
    c->samp.logprobs = s->logprobs ? 1 : 0;
    return ER_OK;
}

extern "C" int er_get_logprobs(er_ctx* c, float* model_out, float* policy_out, int ld, int n_steps, void* stream) {
    if (!c) return fail(ER_ERR_INVALID, "er_get_logprobs: null context");
    const KvMem& kv = *c->kv;
    if (!kv.lp_valid) return fail(ER_ERR_INVALID, "er_get_logprobs: the last er_decode kept no log-probs (er_set_sampling with logprobs on, then er_decode)");
    if (n_steps <= 0 || n_steps > kv.plan.Lcap || ld < n_steps) return fail(ER_ERR_INVALID, "er_get_logprobs: n_steps %d, ld %d (reserved %d)", n_steps, ld, kv.plan.Lcap);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const size_t w = (size_t)n_steps * sizeof(float);
    if (model_out) HIPCHK(hipMemcpy2DAsync(model_out, (size_t)ld * sizeof(float), kv.d_lp_model.p, (size_t)kv.plan.Lcap * sizeof(float), w, kv.plan.B, hipMemcpyDeviceToDevice, st));
    if (policy_out) HIPCHK(hipMemcpy2DAsync(policy_out, (size_t)ld * sizeof(float), kv.d_lp_policy.p, (size_t)kv.plan.Lcap * sizeof(float), w, kv.plan.B, hipMemcpyDeviceToDevice, st));
    return ER_OK;
}

extern "C" int er_set_row_streams(er_ctx* c, const uint32_t* ids, int n) {
    if (!c) return fail(ER_ERR_INVALID, "er_set_row_streams: null context");
    const int B = c->kv->plan.B;
    if (B <= 0) return fail(ER_ERR_INVALID, "er_set_row_streams: no cache reserved (call er_kv_reserve)");
    if (ids && n != B) return fail(ER_ERR_INVALID, "er_set_row_streams: %d ids for a batch of %d rows", n, B);
    HIPCHK(hipSetDevice(c->device));
    std::vector<unsigned int> h((size_t)B);
    for (int i = 0; i < B; ++i) h[i] = ids ? ids[i] : (unsigned int)i;
    HIPCHK(hipDeviceSynchronize());           // a running decode still reads the old ids
    HIPCHK(hipMemcpy(c->kv->d_row_stream.p, h.data(), h.size() * sizeof(unsigned int), hipMemcpyHostToDevice));
    return ER_OK;
}

// ------------------------------------------------------------------------------------ queue mode (continuous batching)
// A free row: budget 0 (the sampling heads return before they write anything of the row) and position 0 (its forward writes
// K/V slot 0 of its own slice and attends that one key).  Nothing of it grows, and nothing reads what its forward leaves.
__global__ void queue_park_kernel(GenState st, int* budget, int row0, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = row0 + i;
    st.tok[b] = 0; st.pos[b] = 0; st.counter[b] = 0; st.ngen[b] = 0;
    st.unfinished[b] = 0; st.eos_step[b] = -1; st.base_pos[b] = 0;
    budget[b] = 0;
}
// The generation state of rows [row0, row0 + n) right after their prefill of S positions (init_state_kernel for a row range), with the
// rows' Philox stream ids and budgets from stage = {ids[n], budgets[n]}.  rows != nullptr (er_queue_admit_copy): row rows[i] in place of
// row0 + i.
__global__ void queue_admit_kernel(GenState st, unsigned int* row_stream, int* budget, const int* stage, int row0, int n, int S, const int* rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = rows ? rows[i] : row0 + i;
    st.tok[b] = 0; st.pos[b] = S; st.counter[b] = 0; st.ngen[b] = 0;
    st.unfinished[b] = 1; st.eos_step[b] = -1; st.base_pos[b] = S;
    row_stream[b] = (unsigned int)stage[i];
    budget[b] = stage[n + i];
}
// What the host looks at between two bursts, in one block: look = {ngen[B], unfinished[B], eos_step[B], error}.
__global__ void queue_look_kernel(GenState st, int B, int* look) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) look[3 * B] = *st.error;
    if (b >= B) return;
    look[b] = st.ngen[b]; look[B + b] = st.unfinished[b]; look[2 * B + b] = st.eos_step[b];
}
__global__ void fill_i32_kernel(int* p, int n, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

static int queue_open(er_ctx* c, const char* who) {
    if (!c) return fail(ER_ERR_INVALID, "%s: null context", who);
    if (!c->q.active) return fail(ER_ERR_INVALID, "%s: no queue is open (call er_queue_begin)", who);
    HIPCHK(hipSetDevice(c->device));
    return 0;
}

extern "C" int er_queue_begin(er_ctx* c, const er_decode_params* p, int check_every, void* stream) {
    if (!c || !p) return fail(ER_ERR_INVALID, "er_queue_begin: bad argument");
    if (c->q.active) return fail(ER_ERR_INVALID, "er_queue_begin: a queue is already open (er_queue_end first)");
    const int B = c->kv->plan.B, Lcap = c->kv->plan.Lcap;
    if (B <= 0) return fail(ER_ERR_INVALID, "er_queue_begin: no cache reserved (call er_kv_reserve)");
    if (c->kv->prefix_len) return fail(ER_ERR_INVALID, "er_queue_begin: prefix groups are set on this context (clear them with er_set_prefix_groups(ctx, NULL, 0, 0))");
    if (p->max_new_tokens <= 0) return fail(ER_ERR_INVALID, "max_new_tokens must be > 0");
    if (p->mode != ER_GREEDY && p->mode != ER_SAMPLE) return fail(ER_ERR_INVALID, "bad mode");
    if (p->grammar < 0 || p->grammar > 2) return fail(ER_ERR_INVALID, "bad grammar");
    if (p->mode == ER_SAMPLE && !c->samp.top_k_set && p->top_k <= 0) return fail(ER_ERR_INVALID, "top_k must be > 0 in sample mode");
    if (check_every < 0) return fail(ER_ERR_INVALID, "er_queue_begin: check_every %d", check_every);
    ERCHK(er_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    ERCHK(ensure_weight_copies(c, c->kv->plan));
    ERCHK(c->q_look.ensure((size_t)3 * B + 1));
    if (c->q_pinned) { hipHostFree(c->q_pinned); c->q_pinned = nullptr; }
    HIPCHK(hipHostMalloc((void**)&c->q_pinned, ((size_t)3 * B + 1) * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipStreamSynchronize(st));
    int top_k = 0;
    ERCHK(head_setup(c, p, &top_k));

    const DecodeParamsDev dp = decode_params_dev(*p, top_k, p->max_new_tokens, c->cfg.eos_token_id, c->cfg.pad_token_id, c->cfg.vocab_size);
    HIPCHK(hipMemcpy(c->kv->d_params.p, &dp, sizeof(dp), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(queue_park_kernel, dim3((B + 63) / 64), dim3(64), 0, st, c->kv->st, c->kv->d_row_budget.p, 0, B);
    HIPRET(hipGetLastError());
    HIPCHK(hipMemsetAsync(c->kv->st.n_unfinished, 0, 2 * sizeof(int), st));                          // n_unfinished (unused here), error
    HIPCHK(hipMemsetAsync(c->kv->ypre.p, 0, (size_t)B * c->cfg.hidden_dim * sizeof(float), st));   // a parked row's first forward reads its row
    ERCHK(ensure_step_graph(c));
    HIPCHK(hipStreamSynchronize(st));
    c->have_hidden = false;
    c->q.begin(B, Lcap, c->cfg.max_positions, p->max_new_tokens, check_every);
    return ER_OK;
}

extern "C" int er_queue_admit(er_ctx* c, int row0, int n_rows, const float* embeds, int S, const uint32_t* stream_ids,
                              const int32_t* max_new, void* stream) {
    ERCHK(queue_open(c, "er_queue_admit"));
    if (!embeds) return fail(ER_ERR_INVALID, "er_queue_admit: embeds is null");
    const long long width = std::max({(long long)c->cfg.intermediate_dim, 3LL * c->cfg.hidden_dim, (long long)c->cfg.vocab_size});
    const int rc = c->q.check_admit(row0, n_rows, S, max_new, width);
    if (rc < 0) return fail(rc, "%s", c->q.why);
    hipStream_t st = pick(c, stream);
    std::vector<int> stage((size_t)2 * n_rows);
    for (int i = 0; i < n_rows; ++i) {
        stage[(size_t)i] = (int)(stream_ids ? stream_ids[i] : (uint32_t)(row0 + i));
        stage[(size_t)n_rows + i] = c->q.budget_of(max_new, i);
    }
    ERCHK(c->q_stage.ensure(stage.size()));
    HIPCHK(hipMemcpyAsync(c->q_stage.p, stage.data(), stage.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->ev0, st));
    ERCHK(prefill_run(c, embeds, n_rows, S, st, row0, true));
    hipLaunchKernelGGL(queue_admit_kernel, dim3((n_rows + 63) / 64), dim3(64), 0, st, c->kv->st, c->kv->d_row_stream.p,
                       c->kv->d_row_budget.p, c->q_stage.p, row0, n_rows, S, (const int*)nullptr);
    HIPRET(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipStreamSynchronize(st));         // `stage` and the caller's arrays are host memory
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->q.stats.prefill_ms += ms;
    c->q.admit(row0, n_rows, S, max_new);
    return ER_OK;
}

extern "C" int er_queue_admit_copy(er_ctx* c, int src_row, const int32_t* dst_rows, int n, const uint32_t* stream_ids, const int32_t* max_new,
                                   void* stream) {
    ERCHK(queue_open(c, "er_queue_admit_copy"));
    const int rc = c->q.check_admit_copy(src_row, dst_rows, n, max_new);
    if (rc < 0) return fail(rc, "%s", c->q.why);
    KvMem& kv = *c->kv;
    const DecodePlan& p = kv.plan;
    const int S = c->q.rows[(size_t)src_row].S, NH = c->cfg.num_heads;
    std::vector<int32_t> src((size_t)n, src_row);
    ERCHK(kv_fork_check("er_queue_admit_copy", kv.kc.p, kv.vc.p, c->kv_esz, p.layers, p.B, NH, p.Lcap, c->D, src.data(), dst_rows, n, S));
    hipStream_t st = pick(c, stream);
    std::vector<int> stage((size_t)3 * n);      // ids | budgets | rows
    for (int i = 0; i < n; ++i) {
        stage[(size_t)i] = (int)(stream_ids ? stream_ids[i] : (uint32_t)dst_rows[i]);
        stage[(size_t)n + i] = c->q.budget_of(max_new, i);
        stage[(size_t)2 * n + i] = dst_rows[i];
    }
    ERCHK(c->q_stage.ensure(stage.size()));
    HIPCHK(hipMemcpyAsync(c->q_stage.p, stage.data(), stage.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->ev0, st));
    HIPRET(launch_kv_fork(kv_fork_args(kv.kc.p, kv.vc.p, c->kv_esz, p.B, NH, p.Lcap, c->D, S), NH, p.layers, src.data(), dst_rows, n, st));
    const size_t H = (size_t)c->cfg.hidden_dim;
    for (int i = 0; i < n; ++i)
        HIPCHK(hipMemcpyAsync(kv.ypre.p + (size_t)dst_rows[i] * H, kv.ypre.p + (size_t)src_row * H, H * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(queue_admit_kernel, dim3((n + 63) / 64), dim3(64), 0, st, kv.st, kv.d_row_stream.p, kv.d_row_budget.p, c->q_stage.p, 0, n, S,
                       (const int*)(c->q_stage.p + 2 * n));
    HIPRET(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipStreamSynchronize(st));         // `stage` and the caller's arrays are host memory
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->q.stats.prefill_ms += ms;              // the copy IS these rows' admission
    c->q.admit_copy(src_row, dst_rows, n, max_new);
    return ER_OK;
}

extern "C" int er_queue_run(er_ctx* c, int32_t* done_rows, int32_t* n_done, void* stream) {
    ERCHK(queue_open(c, "er_queue_run"));
    if (!done_rows || !n_done) return fail(ER_ERR_INVALID, "er_queue_run: bad argument");
    *n_done = c->q.list_done(done_rows);
    if (*n_done > 0 || c->q.occupied() == 0) return ER_OK;
    hipStream_t st = pick(c, stream);
    const int B = c->q.slots, Lcap = c->kv->plan.Lcap;
    HIPCHK(hipEventRecord(c->ev0, st));
    while (*n_done == 0) {
        const int burst = c->q.next_burst();
        if (burst <= 0) return fail(ER_ERR_INVALID, "internal: er_queue_run has occupied rows but none is running");
        for (int t = 0; t < burst; ++t) {
            if (c->knobs.use_graph) HIPCHK(hipGraphLaunch(step_graph(c), st));
            else HIPRET(enqueue_step(c, st, c->kv->d_out_ids.p, Lcap));
        }
        c->q.advance(burst);
        hipLaunchKernelGGL(queue_look_kernel, dim3((B + 63) / 64), dim3(64), 0, st, c->kv->st, B, c->q_look.p);
        HIPRET(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->q_pinned, c->q_look.p, ((size_t)3 * B + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (c->q_pinned[3 * B] != 0)
            return fail(ER_ERR_INVALID, "er_queue_run: a row had no finite candidate score (non-finite logits); HF would raise in multinomial/argmax");
        const int rc = c->q.collect(c->q_pinned, c->q_pinned + B, c->q_pinned + 2 * B, done_rows, n_done);
        if (rc < 0) return fail(rc, "%s", c->q.why);
    }
    HIPCHK(hipEventRecord(c->ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->q.stats.decode_ms += ms;
    return ER_OK;
}

extern "C" int er_queue_take(er_ctx* c, int row, int64_t* ids_out, int capacity, int32_t* n_tokens) {
    ERCHK(queue_open(c, "er_queue_take"));
    if (!ids_out || !n_tokens) return fail(ER_ERR_INVALID, "er_queue_take: bad argument");
    const int rc = c->q.check_take(row, capacity);
    if (rc < 0) return fail(rc, "%s", c->q.why);
    const int n = c->q.rows[(size_t)row].n_tokens;
    HIPCHK(hipMemcpy(ids_out, c->kv->d_out_ids.p + (size_t)row * c->kv->plan.Lcap, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost));
    hipLaunchKernelGGL(queue_park_kernel, dim3(1), dim3(64), 0, c->own_stream, c->kv->st, c->kv->d_row_budget.p, row, 1);
    HIPRET(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->own_stream));
    *n_tokens = n;
    c->q.release(row);
    return ER_OK;
}

extern "C" int er_queue_row_logprobs(er_ctx* c, int row, float* model_out, float* policy_out, int capacity) {
    ERCHK(queue_open(c, "er_queue_row_logprobs"));
    if (!c->kv->lp_on) return fail(ER_ERR_INVALID, "er_queue_row_logprobs: the queue keeps no log-probs (er_set_sampling with logprobs on before er_queue_begin)");
    const int rc = c->q.check_take(row, capacity);
    if (rc < 0) return fail(rc, "%s", c->q.why);
    const size_t n = (size_t)c->q.rows[(size_t)row].n_tokens, at = (size_t)row * c->kv->plan.Lcap;
    if (model_out) HIPCHK(hipMemcpy(model_out, c->kv->d_lp_model.p + at, n * sizeof(float), hipMemcpyDeviceToHost));
    if (policy_out) HIPCHK(hipMemcpy(policy_out, c->kv->d_lp_policy.p + at, n * sizeof(float), hipMemcpyDeviceToHost));
    return ER_OK;
}

extern "C" int er_queue_stats(er_ctx* c, er_queue_counters* out) {
    if (!c || !out) return fail(ER_ERR_INVALID, "er_queue_stats: bad argument");
    if (!c->q.active) return fail(ER_ERR_INVALID, "er_queue_stats: no queue is open");
    *out = c->q.stats;
    return ER_OK;
}

extern "C" int er_queue_end(er_ctx* c) {
    ERCHK(queue_open(c, "er_queue_end"));
    const int B = c->q.slots;
    HIPCHK(hipDeviceSynchronize());
    hipLaunchKernelGGL(fill_i32_kernel, dim3((B + 63) / 64), dim3(64), 0, c->own_stream, c->kv->d_row_budget.p, B, 0x7fffffff);
    HIPRET(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->own_stream));
    c->q.end();
    c->have_hidden = false;
    if (c->q_pinned) { hipHostFree(c->q_pinned); c->q_pinned = nullptr; }
    return er_set_row_streams(c, nullptr, B);
}

extern "C" int er_last_decode_ms(er_ctx* c, float* ms) {
    if (!c || !ms) return fail(ER_ERR_INVALID, "null");
    *ms = c->last_decode_ms;
    return ER_OK;
}

// ------------------------------------------------------------------------------------ per-kernel timing
static int profile_impl(er_ctx* c, int repeats, int use_graph, float* avg_us, double* bytes, void* stream);

extern "C" int er_profile_decode_kernels(er_ctx* c, int repeats, float* avg_us, double* bytes, void* stream) {
    return er_profile_decode_kernels_at(c, repeats, 0, 0, avg_us, bytes, stream);
}

extern "C" int er_profile_decode_kernels_at(er_ctx* c, int repeats, int context_len, int use_graph, float* avg_us, double* bytes,
                                            void* stream) {
    if (!c) return fail(ER_ERR_INVALID, "er_profile_decode_kernels: bad argument");
    if (context_len < 0 || context_len > c->kv->plan.Lcap) return fail(ER_ERR_CAPACITY, "profile: context_len %d outside the reserved cache (%d)", context_len, c->kv->plan.Lcap);
    c->prof_len = context_len;
    const int rc = profile_impl(c, repeats, use_graph, avg_us, bytes, stream);
    c->prof_len = 0;
    return rc;
}

static int profile_impl(er_ctx* c, int repeats, int use_graph, float* avg_us, double* bytes, void* stream) {
    if (!c || !avg_us || !bytes || repeats <= 0) return fail(ER_ERR_INVALID, "er_profile_decode_kernels: bad argument");
    if (!c->have_hidden) return fail(ER_ERR_INVALID, "profile: call er_prefill first");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const er_config& g = c->cfg;
    const DecodePlan& p = c->kv->plan;
    const int B = p.B, H = g.hidden_dim, I = g.intermediate_dim, nl = g.num_layers, V = g.vocab_size;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(c->h_pinned, c->kv->st.pos, sizeof(int), hipMemcpyDeviceToHost));
    const double len = c->prof_len > 0 ? (double)c->prof_len : (double)c->h_pinned[0] + 1.0;
    // save the state the sweep scribbles on
    std::vector<float> save_y((size_t)B * H);
    HIPCHK(hipMemcpy(save_y.data(), c->kv->ypre.p, save_y.size() * 4, hipMemcpyDeviceToHost));
    std::vector<int> save_state(gen_state_ints(B));
    HIPCHK(hipMemcpy(save_state.data(), c->kv->state_block.p, save_state.size() * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> head_state = save_state;          // the head sweep runs at step 0 so it writes dummy_ids[b][0]
    for (int b = 0; b < B; ++b) gen_state_carve(head_state.data(), B).ngen[b] = 0;
    er_decode_params greedy{};                         // greedy under the LR_ABSCO grammar, no budget in the way, seed 0
    greedy.mode = 0; greedy.grammar = 2;
    const DecodeParamsDev dp = decode_params_dev(greedy, 10, 1 << 30, g.eos_token_id, g.pad_token_id, V);
    HIPCHK(hipMemcpy(c->kv->d_params.p, &dp, sizeof(dp), hipMemcpyHostToDevice));
    c->kv->head_ctl = c->kv->row_class = false;   // the plan's own kinds 4, 5 and 7 here; er_decode / er_queue_begin choose again
    DevBuf<long long> dummy;             // freed on every return path; a failing one frees behind hipFree's own device synchronisation
    ERCHK(dummy.ensure((size_t)B * 8));
    long long* dummy_ids = dummy.p;

    const double w = c->fast ? 2.0 : 4.0;   // bytes per streamed weight / KV element
    bytes[0] = ((double)3 * H * H + 3 * H) * w + (double)B * (H + 3 * H) * w;
    bytes[1] = (double)B * 2.0 * len * H * (double)c->kv_esz;
    bytes[2] = (double)B * g.num_heads * p.S_splits * (c->D + 2) * w + (double)B * H * w;
    bytes[3] = ((double)H * H + H) * w + (double)B * 3 * H * w;
    bytes[4] = ((double)I * H + I) * w + (double)B * (H + I) * w;
    bytes[5] = ((double)I * H + H) * w + (double)B * (I + 2 * H) * w;
    bytes[6] = ((double)V * H) * w + (double)B * (H + V) * w;
    bytes[7] = (double)B * V * w;
    {   // what the step streams packed in place of 2 bytes per weight (weight_source; row_class was cleared above) - bytes: 1 per weight + 4 per
        // row scale; nibbles: half a byte per weight + a scale byte per 32 (the tiled copy: 4 bytes per 96).  The fused MLP's bytes are counted below.
        const auto less = [&](Proj proj, double n, double k) {
            switch (weight_source(p, c->knobs, ctx_mode(c), false, proj, 0)) {
                case WSRC_BYTES: case WSRC_TILED_BYTES: return n * k * (w - 1.0) - n * 4.0;
                case WSRC_TILED_NIBBLES: return n * k * w - (double)w4t::block_bytes((long long)n, (long long)k);
                case WSRC_QUADS: return n * k * (w - 0.5 - 1.0 / 32.0);
                default: return 0.0;
            }
        };
        bytes[0] -= less(PROJ_QKV, 3.0 * H, H);
        bytes[3] -= less(PROJ_OUT, H, H);
        bytes[4] -= less(PROJ_FC1, I, H);
        bytes[5] -= less(PROJ_FC2, H, I);
    }

    if (p.shared_attn) {   // kind 1 reads the prefix once per group and writes a partial per (row, head, chunk); kind 2 reads the suffixes and the partials
        const double P = c->kv->prefix_len, parts = (double)B * g.num_heads * attn_shared_chunks(c->kv->prefix_len) * (c->D + 2) * 4.0;
        bytes[1] = (double)c->kv->n_groups * 2.0 * P * H * w + parts;
        bytes[2] = (double)B * 2.0 * std::max(0.0, len - P) * H * w + parts + (double)B * H * 4.0;
    }
    if (p.v3) {   // the merge is part of the out_proj launch: its partial reads are charged there
        bytes[3] += (double)g.num_heads * p.nch3 * (c->D + 2) * 4.0;
        bytes[2] = 0.0;
    }
    for (int kind = 0; kind < ER_NUM_KERNEL_KINDS; ++kind) {
        const bool per_layer = kind <= 5;
        if (!p.sel.merge_launch && kind == 2) { avg_us[kind] = 0.f; continue; }
        // warm-up + timed sweeps
        hipGraphExec_t gexec = nullptr;
        if (use_graph && per_layer) {     // the nl launches of this kind as one replayable graph (what the generation loop replays)
            hipGraph_t graph = nullptr;
            HIPCHK(hipStreamBeginCapture(c->own_stream, hipStreamCaptureModeRelaxed));
            hipError_t e = hipSuccess;
            for (int l = 0; l < nl && e == hipSuccess; ++l) e = launch_kind(c, kind, l, c->own_stream, dummy_ids, 8);
            hipError_t e2 = hipStreamEndCapture(c->own_stream, &graph);
            if (e != hipSuccess || e2 != hipSuccess) { if (graph) hipGraphDestroy(graph); return fail(ER_ERR_HIP, "profile: graph capture failed"); }
            HIPCHK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
            hipGraphDestroy(graph);
        }
        for (int pass = 0; pass < 2; ++pass) {
            const int reps = pass == 0 ? 1 : repeats;
            if (pass == 1) HIPCHK(hipEventRecord(c->ev0, st));
            int launches = 0;
            for (int r = 0; r < reps; ++r) {
                if (gexec) {
                    HIPCHK(hipGraphLaunch(gexec, st));
                    launches += nl;
                } else if (per_layer) {
                    for (int l = 0; l < nl; ++l) { HIPRET(launch_kind(c, kind, l, st, dummy_ids, 8)); ++launches; }
                } else {
                    for (int l = 0; l < nl; ++l) {   // same number of back-to-back launches
                        if (kind == 7) {   // keep the head's step counter in range
                            HIPCHK(hipMemcpyAsync(c->kv->state_block.p, head_state.data(), head_state.size() * sizeof(int), hipMemcpyHostToDevice, st));
                        }
                        HIPRET(launch_kind(c, kind, 0, st, dummy_ids, 8));
                        ++launches;
                    }
                }
            }
            if (pass == 1) {
                HIPCHK(hipEventRecord(c->ev1, st));
                HIPCHK(hipStreamSynchronize(st));
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
                avg_us[kind] = ms * 1000.0f / (float)launches;
            }
        }
        if (gexec) hipGraphExecDestroy(gexec);
    }
    HIPCHK(hipStreamSynchronize(st));
    if (p.mlp_fused) {   // what the sweep's launches streamed: W1, the LIVE rows of W2T (counted by the kernel itself), the chain vectors
        std::vector<int> nnz((size_t)nl * MLP_WGS);
        HIPCHK(hipMemcpy(nnz.data(), c->kv->mlp_nnz.p, nnz.size() * sizeof(int), hipMemcpyDeviceToHost));
        double live = 0.0;
        for (int n : nnz) live += n;
        const double part = (double)MLP_WGS * H * 4.0;
        bytes[4] = ((double)I * H + live / nl * H) * w + ((double)I + 4 * H) * 4.0 + part;
        bytes[5] = part + (double)3 * H * 4.0;
    }
    HIPCHK(hipMemcpy(c->kv->ypre.p, save_y.data(), save_y.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->kv->state_block.p, save_state.data(), save_state.size() * sizeof(int), hipMemcpyHostToDevice));
    return ER_OK;
}

// ------------------------------------------------------------------------------------ single-kernel entry points
// Their temporaries are local DevBufs: allocated before the first launch, and freed by every return path - behind the explicit
// hipStreamSynchronize on the paths that launched something.
// One projection on caller-owned operands in a batched form, as er_k_gemv and er_k_gemv_form run it.  It first gets what a decode context
// keeps per reserved shape: rows for the prologue's output when the caller wants none back, the derived copy of the weights that io.src
// names (io.w comes in as what that copy is made of: launch_weight_copy), the split-K block (a deferred form leaves its partials in part_out instead) and, for the wide tiled form, one zeroed image of
// K * 128 bytes per group of 32 rows unless the caller passed one.  Then run_proj - or, for ER_FORM_PREP, the prologue launch alone.
template <typename WT>
static int proj_entry(Proj proj, const ProjForm& f, ProjIo io, GemvArgs a, int B, int K, float* part_out, hipStream_t st) {
    const int form = f.form, n = a.N;
    const size_t groups = (size_t)(B + NBM - 1) / NBM;
    const int slices = form == ER_FORM_NARROW || form == ER_FORM_NARROW_DEFER ? K / (4 * GM_KW) : K / (GM_WAVES * GM_KW);
    DevBuf<float> tmp, part;
    DevBuf<char> wcopy, img;
    SkPart sk{nullptr, 0};
    hipError_t e = hipSuccess;
    if (form != ER_FORM_ROW && form != ER_FORM_ROWS8) {
        if (io.pro != PRO_NONE && !a.hout) { ERCHK(tmp.ensure((size_t)B * K)); a.hout = tmp.p; }
        if (form_mfma(form)) {
            if (form != ER_FORM_NARROW_DEFER) ERCHK(part.ensure((size_t)slices * NBM * n));
            sk = form == ER_FORM_NARROW_DEFER ? SkPart{part_out, groups * slices * NBM * (size_t)n} : SkPart{part.p, part.n};
        }
        if (form == ER_FORM_MFMA_XT) {
            if (!io.pro_image) {
                ERCHK(img.ensure(groups * (size_t)K * 128));
                HIPCHK(hipMemsetAsync(img.p, 0, groups * (size_t)K * 128, st));
                io.pro_image = img.p;
            }
            io.x_image = io.pro_image;
        }
    }
    if (wsrc_derived(io.src) && form != ER_FORM_PREP) {
        ERCHK(wcopy.ensure(weight_copy_bytes(io.src, sizeof(WT) == 2, n, K)));
        e = launch_weight_copy(io.src, sizeof(WT) == 2, io.w, wcopy.p, n, K, st);
        io.w = wcopy.p;
    }
    if (e == hipSuccess) e = form == ER_FORM_PREP ? launch_prologue(io.pro, a, B, io.rd, io.pro_image, st) : run_proj<WT>(proj, f, io, a, B, K, sk, st);
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

// (k, relu, resid) name the projection: fc1, lm_head and out_proj at k = 1536, fc2 at 6144.  batch <= 4: its fp32 4-wave row kernel,
// which exists with the projection's own prologue only; batch > 4: the batched form (LayerNorm rows first when ln_w is given).
extern "C" int er_k_gemv(const float* w, const float* bias, const float* x, const float* ln_w, const float* ln_b,
                         const float* resid, float* y, float* xnorm_out, int B, int n, int k, int relu, float eps, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GemvArgs a{};
    a.bias = bias; a.N = n; a.xin = x; a.ln_w = ln_w; a.ln_b = ln_b; a.eps = eps; a.hout = xnorm_out;
    a.out = y; a.resid = resid;
    const bool batched = B > 4;
    if (batched && ln_w && k != 1536) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv: LayerNorm prologue needs k=1536");
    Proj proj = PROJ_FC2;
    bool built = k == 6144 && !relu && resid && !ln_w;
    if (k == 1536 && !(relu && resid)) {
        proj = relu ? PROJ_FC1 : resid ? PROJ_OUT : PROJ_HEAD;
        built = batched || (ln_w != nullptr) == (proj != PROJ_OUT);
    }
    if (!built) {
        if (batched) HIPRET(hipErrorInvalidValue);
        if (k != 1536 && k != 6144) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv: k must be 1536 or 6144");
        return fail(ER_ERR_UNSUPPORTED, "er_k_gemv: combination not instantiated for k=%d", k);
    }
    const bool wide = proj == PROJ_FC1 || proj == PROJ_FC2;
    ProjIo io;
    io.pro = ln_w ? PRO_LN : PRO_NONE; io.w = w;
    if (batched) {   // matrix cores for the fc1- and fc2-shaped cases unless ER_BATCHED_VALU=1, the VALU kernel for the narrow ones
        const ProjForm f{wide && !env_is("ER_BATCHED_VALU", '1') ? ER_FORM_MFMA : ER_FORM_VALU, 0, 0, false};
        io.src = form_mfma(f.form) ? WSRC_TILED : WSRC_PLAIN;
        return proj_entry<float>(proj, f, io, a, B, k, nullptr, st);
    }
    HIPRET(run_proj<float>(proj, ProjForm{ER_FORM_ROW, ER_NWAVES, wide ? 2 : 1, false}, io, a, B, k, SkPart{nullptr, 0}, st));
    return ER_OK;
}

extern "C" int er_k_attn_decode(const float* q, const void* k, const void* v, const int32_t* len_host, float* out, int B,
                                int heads, int head_dim, int l_cap, int steps, int kv_half, int variant, void* stream) {
    if (variant != ER_ATTN_SPLIT1 && variant != ER_ATTN_SPLIT2 && variant != ER_ATTN_STREAM)
        return fail(ER_ERR_INVALID, "er_k_attn_decode: variant must be ER_ATTN_SPLIT1, ER_ATTN_SPLIT2 or ER_ATTN_STREAM");
    if (variant == ER_ATTN_STREAM && head_dim != 96) return fail(ER_ERR_UNSUPPORTED, "the streaming kernel is built for head_dim 96");
    if (head_dim != 96 && head_dim != 64) return fail(ER_ERR_UNSUPPORTED, "head_dim %d", head_dim);
    if (steps != 2 && steps != 4 && steps != 8) return fail(ER_ERR_INVALID, "steps must be 2, 4 or 8 (chunk = 32*steps keys)");
    if (kv_half < 0 || kv_half > 2) return fail(ER_ERR_INVALID, "er_k_attn_decode: kv_half %d (0 = fp32, 1 = fp16, 2 = e4m3 bytes)", kv_half);
    if (kv_half == 2 && (head_dim != 96 || variant == ER_ATTN_SPLIT1 || (variant == ER_ATTN_SPLIT2 && steps != ATTN_STEPS_DEFAULT)))
        return fail(ER_ERR_UNSUPPORTED, "er_k_attn_decode: the byte cache runs ER_ATTN_SPLIT2 (steps 4) and ER_ATTN_STREAM at head_dim 96");
    hipStream_t st = (hipStream_t)stream;
    const int S = attn_num_chunks(l_cap, attn_chunk(steps));
    DevBuf<int> len_dev;
    DevBuf<float> part;
    ERCHK(len_dev.ensure(B));
    ERCHK(part.ensure((size_t)B * heads * S * (head_dim + 2)));
    HIPCHK(hipMemcpy(len_dev.p, len_host, B * sizeof(int), hipMemcpyHostToDevice));
    AttnDecArgs a = attn_dec_args(heads, head_dim, l_cap);
    a.q = q; a.kcache = k; a.vcache = v; a.len_dev = len_dev.p; a.part = part.p; a.out = out;
    a.S = S; a.chunk = attn_chunk(steps);
    hipError_t e;
    if (variant == ER_ATTN_STREAM) {       // the streaming kernel of the batched decode step (no partials)
        e = launch_attn_stream_d<96>(a, kv_half, B, st);
    } else {
        e = launch_attn_partial(a, head_dim, steps, kv_half, B, st, variant == ER_ATTN_SPLIT1 ? 1 : 2);
        if (e == hipSuccess) e = launch_attn_combine(a, head_dim, B, st);
    }
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

extern "C" int er_k_attn_stream_xt(const float* q, const void* k, const void* v, const int32_t* len_host, float* out, void* out_xt, int B,
                                   int heads, int l_cap, int kv_half, void* stream) {
    constexpr int D = 96;
    if (!q || !k || !v || !len_host || !out || B < 1 || heads < 1 || l_cap < 1) return fail(ER_ERR_INVALID, "er_k_attn_stream_xt: bad argument");
    if (kv_half < 0 || kv_half > 2) return fail(ER_ERR_INVALID, "er_k_attn_stream_xt: kv_half %d (0 = fp32, 1 = fp16, 2 = e4m3 bytes)", kv_half);
    for (int b = 0; b < B; ++b)
        if (len_host[b] < 1 || len_host[b] > l_cap) return fail(ER_ERR_CAPACITY, "er_k_attn_stream_xt: len[%d] = %d / l_cap %d", b, len_host[b], l_cap);
    hipStream_t st = (hipStream_t)stream;
    DevBuf<int> len_dev;
    ERCHK(len_dev.ensure(B));
    HIPCHK(hipMemcpy(len_dev.p, len_host, B * sizeof(int), hipMemcpyHostToDevice));
    AttnDecArgs a = attn_dec_args(heads, D, l_cap);
    a.q = q; a.kcache = k; a.vcache = v; a.len_dev = len_dev.p; a.out = out; a.out_xt = out_xt;      // as attn_args: xt_att when out_proj reads the tiled image
    hipError_t e = launch_attn_stream_d<D>(a, kv_half, B, st);      // launch_kind_t case 1, stream_attn
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

static int k_attn_shared_run(const char* who, bool mfma, const float* q, const void* k, const void* v, const int32_t* len_host, const int32_t* leader,
                             int prefix_len, float* out, void* out_xt, int B, int heads, int l_cap, int kv_half, void* stream);

extern "C" int er_k_attn_shared(const float* q, const void* k, const void* v, const int32_t* len_host, const int32_t* leader, int prefix_len,
                                float* out, void* out_xt, int B, int heads, int l_cap, int kv_half, void* stream) {
    return k_attn_shared_run("er_k_attn_shared", false, q, k, v, len_host, leader, prefix_len, out, out_xt, B, heads, l_cap, kv_half, stream);
}

extern "C" int er_k_attn_shared_mfma(const float* q, const void* k, const void* v, const int32_t* len_host, const int32_t* leader, int prefix_len,
                                     float* out, void* out_xt, int B, int heads, int l_cap, int kv_half, void* stream) {
    if (kv_half != 1) return fail(ER_ERR_UNSUPPORTED, "er_k_attn_shared_mfma: the matrix-core prefix pass reads fp16 caches only (kv_half = 1; got %d)", kv_half);
    return k_attn_shared_run("er_k_attn_shared_mfma", true, q, k, v, len_host, leader, prefix_len, out, out_xt, B, heads, l_cap, kv_half, stream);
}

static int k_attn_shared_run(const char* who, bool mfma, const float* q, const void* k, const void* v, const int32_t* len_host, const int32_t* leader,
                             int prefix_len, float* out, void* out_xt, int B, int heads, int l_cap, int kv_half, void* stream) {
    constexpr int D = 96;
    if (!q || !k || !v || !len_host || !leader || !out || B < 1 || heads < 1 || l_cap < 1) return fail(ER_ERR_INVALID, "%s: bad argument", who);
    if (prefix_len < 1 || prefix_len > l_cap) return fail(ER_ERR_INVALID, "%s: prefix_len %d outside [1, %d]", who, prefix_len, l_cap);
    std::vector<int> rows, off;
    for (int b = 0; b < B; ++b) {
        if (leader[b] < 0 || leader[b] > b || leader[leader[b]] != leader[b]) return fail(ER_ERR_INVALID, "%s: leader[%d] = %d", who, b, leader[b]);
        if (len_host[b] < prefix_len || len_host[b] > l_cap) return fail(ER_ERR_CAPACITY, "%s: len[%d] = %d outside [%d, %d]", who, b, len_host[b], prefix_len, l_cap);
    }
    for (int b = 0; b < B; ++b) {
        if (leader[b] != b) continue;
        off.push_back((int)rows.size());
        for (int r = b; r < B; ++r) if (leader[r] == b) rows.push_back(r);
    }
    off.push_back((int)rows.size());
    hipStream_t st = (hipStream_t)stream;
    DevBuf<int> len_dev, rows_dev, off_dev;
    DevBuf<float> part;
    AttnSharedArgs s{};
    s.a = attn_dec_args(heads, D, l_cap);
    s.prefix_len = prefix_len;
    s.a.S = attn_shared_chunks(prefix_len);
    ERCHK(len_dev.ensure(B));
    ERCHK(rows_dev.ensure(rows.size()));
    ERCHK(off_dev.ensure(off.size()));
    ERCHK(part.ensure((size_t)B * heads * s.a.S * (D + 2)));
    HIPCHK(hipMemcpy(len_dev.p, len_host, B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rows_dev.p, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(off_dev.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice));
    s.a.q = q; s.a.kcache = k; s.a.vcache = v; s.a.len_dev = len_dev.p; s.a.part = part.p; s.a.out = out; s.a.out_xt = out_xt;
    s.grp_rows = rows_dev.p; s.grp_off = off_dev.p;
    const int groups = (int)off.size() - 1;
    hipError_t e = mfma ? launch_attn_prefix_mfma_d<D>(s, groups, st)                      // launch_kind_t kinds 1 and 2, shared_mfma / shared_attn
                        : launch_attn_prefix_d<D>(s, kv_half != 0, groups, st);
    if (e == hipSuccess) e = launch_attn_suffix_merge_d<D>(s, kv_half != 0, B, st);
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

// the rows route of extend_attention (attn_extend_kernel + attn_extend_merge_kernel) on caller-owned q and caches
extern "C" int er_k_attn_extend(const float* q, const void* k, const void* v, int past_len, int n_new, float* out, int B, int heads, int l_cap,
                                int head_dim, int kv_half, void* stream) {
    if (!q || !k || !v || !out || B < 1 || B > 65535 || heads < 1 || l_cap < 1) return fail(ER_ERR_INVALID, "er_k_attn_extend: bad argument");
    if (kv_half < 0 || kv_half > 2) return fail(ER_ERR_INVALID, "er_k_attn_extend: kv_half %d (0 = fp32, 1 = fp16, 2 = e4m3 bytes)", kv_half);
    if (!attn_extend_supported(head_dim, kv_half))
        return fail(ER_ERR_UNSUPPORTED, "er_k_attn_extend: head_dim %d with cache type %d (96: every cache type; 64: fp32 and fp16)", head_dim, kv_half);
    if (past_len < 1 || n_new < 1 || n_new > 65535) return fail(ER_ERR_INVALID, "er_k_attn_extend: past_len %d, n_new %d", past_len, n_new);
    if (past_len > l_cap - n_new) return fail(ER_ERR_CAPACITY, "er_k_attn_extend: past_len %d + n_new %d > l_cap %d", past_len, n_new, l_cap);
    hipStream_t st = (hipStream_t)stream;
    DevBuf<float> part;
    ERCHK(part.ensure(attn_extend_part_floats(B, n_new, heads, past_len + n_new, head_dim)));
    AttnExtendArgs a{};
    a.q = q; a.ldq = heads * head_dim; a.kcache = k; a.vcache = v; a.part = part.p; a.out = out; a.ldo = heads * head_dim;
    a.H = heads; a.l_cap = l_cap; a.S = attn_extend_chunks(past_len + n_new); a.past_len = past_len; a.n_new = n_new;
    a.kv_bstride = (long long)heads * l_cap * head_dim; a.sqrt_d = sqrtf((float)head_dim);
    hipError_t e = launch_attn_extend(a, head_dim, kv_half, B, st);       // extend_attention, rows route
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

// ---- er_k_gemv_form: one decode projection in one of the forms the decode step launches it in.  The entry goes through the step's own
// launch table (run_proj / launch_proj) and takes "the step can launch this" from the step's own rule (proj_form_legal); what the step never
// launches is refused by gemv_form_check before anything is allocated or launched.
static int gemv_form_check(const er_k_gemv_form_args& f, Proj* proj_out) {
    const int B = f.batch, n = f.n, k = f.k, pro = f.prologue, epi = f.epilogue, form = f.form;
    const bool half = f.w_half != 0;
    if (B < 1 || B > ER_MAX_BATCH || n < 1) return fail(ER_ERR_INVALID, "er_k_gemv_form: batch %d, n %d", B, n);
    if (k != 1536 && k != 6144) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: k must be 1536 or 6144");
    Proj proj = PROJ_QKV;      // (unused by ER_FORM_PREP)
    const bool prep = form == ER_FORM_PREP;
    if (prep) {
        if (k != 1536 || pro == ER_PRO_NONE) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: the prologue launch is built for k=1536 and LN / EMBED");
        if (!f.xnorm_out) return fail(ER_ERR_INVALID, "er_k_gemv_form: ER_FORM_PREP needs xnorm_out");
    } else {
        if (!f.w) return fail(ER_ERR_INVALID, "er_k_gemv_form: null weights");
        if (epi == ER_EPI_QKV && k == 1536 && pro != ER_PRO_NONE) proj = PROJ_QKV;
        else if (epi == ER_EPI_RELU && k == 1536 && (pro == ER_PRO_LN || pro == ER_PRO_LN_SK)) proj = PROJ_FC1;
        else if (epi == ER_EPI_RESID && pro == ER_PRO_NONE) proj = k == 1536 ? PROJ_OUT : PROJ_FC2;
        else if (epi == ER_EPI_STORE && k == 1536 && pro == ER_PRO_LN) proj = PROJ_HEAD;
        else return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: no decode projection has k=%d, prologue %d, epilogue %d", k, pro, epi);
    }
    // operands of the prologue and the epilogue
    if (pro == ER_PRO_NONE && !f.x) return fail(ER_ERR_INVALID, "er_k_gemv_form: null x");
    if (pro == ER_PRO_LN && (!f.x || !f.ln_w || !f.ln_b)) return fail(ER_ERR_INVALID, "er_k_gemv_form: PRO_LN needs x, ln_w, ln_b");
    if (pro == ER_PRO_EMBED && (!f.embd || !f.posemb || !f.tok || !f.pos)) return fail(ER_ERR_INVALID, "er_k_gemv_form: PRO_EMBED needs embd, posemb, tok, pos");
    if (pro == ER_PRO_LN_SK) {
        if (!f.sk_part || !f.sk_bias || !f.sk_resid || !f.ln_w || !f.ln_b) return fail(ER_ERR_INVALID, "er_k_gemv_form: PRO_LN_SK needs sk_part, sk_bias, sk_resid, ln_w, ln_b");
        // only the tiled fast-mode path defers a finish: fc2's 16 partials to the next layer's qkv, out_proj's 4 to fc1
        if (!half || form == ER_FORM_ROW || form == ER_FORM_ROWS8) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: a deferred finish is read by the fast-mode batched prologue only");
        const int want = prep ? f.sk_slices : proj == PROJ_QKV ? SK_SLICES_FC2 : proj == PROJ_FC1 ? SK_SLICES_OUTPROJ : f.sk_slices;
        if ((f.sk_slices != SK_SLICES_OUTPROJ && f.sk_slices != SK_SLICES_FC2) || f.sk_slices != want)
            return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: sk_slices %d (qkv reads 16, fc1 reads 4)", f.sk_slices);
    }
    if (!prep && proj == PROJ_QKV) {
        if (!f.q_out || !f.kcache || !f.vcache || !f.pos) return fail(ER_ERR_INVALID, "er_k_gemv_form: EPI_QKV needs q_out, kcache, vcache, pos");
        if (f.heads < 1 || f.head_dim < 1 || f.l_cap < 1 || f.heads * f.head_dim != k || n != 3 * k)
            return fail(ER_ERR_INVALID, "er_k_gemv_form: EPI_QKV needs heads * head_dim == k and n == 3 k");
        if (f.kv_half == 2 && !half) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: the e4m3 byte cache (kv_half 2) goes with fp16 or byte weights");
    } else if (!prep) {
        if (!f.y && !(form == ER_FORM_MFMA_XT && proj == PROJ_FC1) && form != ER_FORM_NARROW_DEFER) return fail(ER_ERR_INVALID, "er_k_gemv_form: null y");
        if (epi == ER_EPI_RESID && !f.resid && form != ER_FORM_NARROW_DEFER) return fail(ER_ERR_INVALID, "er_k_gemv_form: EPI_RESID needs resid");
    }
    if (f.prep_xt_out && !(half && pro != ER_PRO_NONE && (form == ER_FORM_MFMA_XT || form == ER_FORM_PREP)))
        return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: prep_xt_out is written in front of the tiled fp16 forms only");
    // the form: the step's rule, and the batched forms at batch > 4 only (the step reaches them below that under ER_FORCE_BATCHED=1)
    if (form != ER_FORM_ROW && form != ER_FORM_ROWS8 && B <= 4) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: the batched forms run at batch > 4");
    if (form < ER_FORM_ROW || form > ER_FORM_PREP) return fail(ER_ERR_INVALID, "er_k_gemv_form: form %d", form);
    if (!prep && !proj_form_legal(proj, ProjForm{form, f.nw, f.rw, form == ER_FORM_NARROW_DEFER}, half, B))
        return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form: the decode step never launches projection %d in form %d (%d waves x %d rows) with %s weights at batch %d",
                    (int)proj, form, f.nw, f.rw, half ? "fp16" : "fp32", B);
    if (form == ER_FORM_MFMA_XT && proj == PROJ_FC1 && (!f.xt_out || n % 4)) return fail(ER_ERR_INVALID, "er_k_gemv_form: the tiled fc1 writes xt_out (n a multiple of 4)");
    if (form == ER_FORM_NARROW_DEFER && !f.part_out) return fail(ER_ERR_INVALID, "er_k_gemv_form: ER_FORM_NARROW_DEFER needs part_out");
    *proj_out = proj;
    return ER_OK;
}

// row / tiled: the source of f.w's family in a row form / a matrix-core form (f.w: the plain matrix, the byte block or the canonical MXFP4 block)
template <typename WT>
static int gemv_form_t(const er_k_gemv_form_args& f, Proj proj, hipStream_t st, WSrc row = WSRC_PLAIN, WSrc tiled = WSRC_TILED) {
    GemvArgs a{};
    a.bias = f.bias; a.N = f.n; a.xin = f.x; a.ln_w = f.ln_w; a.ln_b = f.ln_b; a.eps = f.eps; a.hout = f.xnorm_out;
    a.embd = f.embd; a.posemb = f.posemb; a.tok = f.tok; a.pos = f.pos;
    a.out = f.y; a.resid = f.resid; a.q = f.q_out; a.kcache = f.kcache; a.vcache = f.vcache; a.kv_half = f.kv_half == 2 ? 2 : f.kv_half ? 1 : 0;
    a.hidden = f.form != ER_FORM_PREP && proj == PROJ_QKV ? f.heads * f.head_dim : 1536; a.head_dim = f.head_dim; a.l_cap = f.l_cap;
    a.kv_bstride = (long long)f.heads * f.l_cap * f.head_dim;
    ProjIo io;
    io.pro = f.prologue == ER_PRO_NONE ? PRO_NONE : f.prologue == ER_PRO_EMBED ? PRO_EMBED : PRO_LN;
    if (f.prologue == ER_PRO_LN_SK) io.rd = {f.sk_part, f.sk_bias, f.sk_resid, f.sk_slices};
    io.pro_image = f.prep_xt_out; io.x_image = f.x; io.out_image = f.xt_out;      // the narrow forms' x IS the tiled image
    io.src = form_mfma(f.form) ? tiled : row; io.w = f.w;
    return proj_entry<WT>(proj, ProjForm{f.form, f.nw, f.rw, f.form == ER_FORM_NARROW_DEFER}, io, a, f.batch, f.k, f.part_out, st);
}

extern "C" int er_k_gemv_form(const er_k_gemv_form_args* f, void* stream) {
    if (!f) return fail(ER_ERR_INVALID, "er_k_gemv_form: null args");
    Proj proj = PROJ_QKV;
    ERCHK(gemv_form_check(*f, &proj));
    return f->w_half ? gemv_form_t<_Float16>(*f, proj, (hipStream_t)stream) : gemv_form_t<float>(*f, proj, (hipStream_t)stream);
}

// ---- kv8 mode: the device encoder the K/V producers store with (k_gemv.h gemv_epilogue, k_rowops.h kv_scatter_f8_kernel) on a flat array
extern "C" int er_k_kv8_encode(const float* src, void* dst, long long n, void* stream) {
    if (!src || !dst || n < 1) return fail(ER_ERR_INVALID, "er_k_kv8_encode: bad argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kv8_encode_kernel, dim3(ew_grid(n)), dim3(ER_WG), 0, st, src, (unsigned char*)dst, n);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

// ---- fp8 mode on caller-owned operands: the row quantiser of the weight loader, and the byte kernels behind the row forms.
extern "C" int er_k_w8_quantize(const void* src, int dtype, int on_device, int n, int k, void* q_dev, int32_t* e_dev, void* w16_dev,
                                float* wscale_dev, void* stream) {
    if (!src || n < 1 || k < 1) return fail(ER_ERR_INVALID, "er_k_w8_quantize: bad argument");
    if (dtype != ER_F32 && dtype != ER_F16 && dtype != ER_BF16) return fail(ER_ERR_INVALID, "er_k_w8_quantize: dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    DevBuf<char> stage;
    DevBuf<int> bad;
    ERCHK(bad.ensure(1));
    if (!on_device) {
        const size_t bytes = (size_t)n * k * (dtype == ER_F32 ? 4 : 2);
        ERCHK(stage.ensure((bytes + 3) / 4 * 4));
        HIPCHK(hipMemcpy(stage.p, src, bytes, hipMemcpyHostToDevice));
        src = stage.p;
    }
    HIPCHK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(quant_rows_kernel, dim3((unsigned)n), dim3(ER_WG), 0, st, src, dtype, (size_t)k, (float*)nullptr, (_Float16*)w16_dev,
                       (unsigned char*)q_dev, wscale_dev, (int*)e_dev, bad.p);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    int flag = 0;
    HIPCHK(hipMemcpy(&flag, bad.p, sizeof(int), hipMemcpyDeviceToHost));
    if (flag) return fail(ER_ERR_INVALID, "er_k_w8_quantize: the matrix holds a NaN or an infinity");
    return ER_OK;
}

// the byte block the kernels stream (k_gemv.h w8_scales) from a caller's separate bytes [n][k] and scales [n]
static int w8_block_of(DevBuf<char>& blk, const void* q_dev, const float* wscale_dev, int n, int k, hipStream_t st) {
    if ((size_t)n * k % 4) return fail(ER_ERR_INVALID, "w8: n * k must be a multiple of 4");
    ERCHK(blk.ensure(w8_block_bytes(n, k)));
    HIPCHK(hipMemcpyAsync(blk.p, q_dev, (size_t)n * k, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(blk.p + (size_t)n * k, wscale_dev, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

// er_k_gemv_form's checks and launch table on (bytes, wscale): the fp16 row shapes and the four matrix-core forms of qkv, out_proj, fc1
// and fc2.  args->w is not read.
extern "C" int er_k_gemv_form_w8(const er_k_gemv_form_args* f, const void* q_dev, const float* wscale_dev, void* stream) {
    if (!f || !q_dev || !wscale_dev) return fail(ER_ERR_INVALID, "er_k_gemv_form_w8: null argument");
    er_k_gemv_form_args g = *f;
    g.w = q_dev;
    if (!g.w_half) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w8: the bytes run the fp16 row shapes (set w_half)");
    if (g.form != ER_FORM_ROW && !form_mfma(g.form))
        return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w8: only the row forms and the matrix-core forms stream bytes (form %d)", g.form);
    Proj proj = PROJ_QKV;
    ERCHK(gemv_form_check(g, &proj));
    if (proj == PROJ_HEAD) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w8: the lm_head is not quantised");
    hipStream_t st = (hipStream_t)stream;
    DevBuf<char> blk;
    ERCHK(w8_block_of(blk, q_dev, wscale_dev, g.n, g.k, st));
    g.w = blk.p;      // proj_entry tiles the block for the matrix-core forms (tile_weights_kernel<w8_t>) and synchronises before blk goes
    return gemv_form_t<_Float16>(g, proj, st, WSRC_BYTES, WSRC_TILED_BYTES);
}

// ---- fp4 mode on caller-owned operands: the block quantiser of the weight loader, the hardware conversion the nibble kernels read
// with, and the nibble kernels behind the row forms.
extern "C" int er_k_w4_quantize(const void* src, int dtype, int on_device, int n, int k, void* block_dev, int32_t* e_dev, void* w16_dev, void* stream) {
    if (!src || n < 1 || k < 1) return fail(ER_ERR_INVALID, "er_k_w4_quantize: bad argument");
    if (k % W4_BLOCK) return fail(ER_ERR_INVALID, "er_k_w4_quantize: k must be a multiple of %d", W4_BLOCK);
    if (dtype != ER_F32 && dtype != ER_F16 && dtype != ER_BF16) return fail(ER_ERR_INVALID, "er_k_w4_quantize: dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    DevBuf<char> stage;
    DevBuf<int> bad;
    ERCHK(bad.ensure(1));
    if (!on_device) {
        const size_t bytes = (size_t)n * k * (dtype == ER_F32 ? 4 : 2);
        ERCHK(stage.ensure((bytes + 3) / 4 * 4));
        HIPCHK(hipMemcpy(stage.p, src, bytes, hipMemcpyHostToDevice));
        src = stage.p;
    }
    HIPCHK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
    unsigned char* nib = (unsigned char*)block_dev;
    hipLaunchKernelGGL(quant_blocks_kernel, dim3((unsigned)n), dim3(ER_WG), 0, st, src, dtype, (size_t)k, (float*)nullptr, (_Float16*)w16_dev, nib,
                       nib ? nib + w4_nibble_bytes(n, k) : nullptr, (int*)e_dev, bad.p);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    int flag = 0;
    HIPCHK(hipMemcpy(&flag, bad.p, sizeof(int), hipMemcpyDeviceToHost));
    if (flag) return fail(ER_ERR_INVALID, "er_k_w4_quantize: the matrix holds a NaN or an infinity");
    return ER_OK;
}

// out[((e - W4_E_MIN) * 256 + byte) * 4 + sel] = the two numbers v_cvt_scalef32_pk_f32_fp4 makes of byte `byte`, placed as byte `sel` of a
// dword whose other bytes hold other codes, under the scale 2^e
__global__ __launch_bounds__(256) void w4_cvt_probe_kernel(float* out) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const unsigned int byte = threadIdx.x, e = blockIdx.x;
    const float scale = w4_scale_f32(w4_scale_byte((int)e + W4_E_MIN));
    f32x2* o = reinterpret_cast<f32x2*>(out) + ((size_t)e * 256 + byte) * 4;
    const unsigned int fill = 0x5a3c96e1u;
    o[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((fill & ~0xffu) | byte, scale, 0);
    o[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((fill & ~0xff00u) | (byte << 8), scale, 1);
    o[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((fill & ~0xff0000u) | (byte << 16), scale, 2);
    o[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((fill & ~0xff000000u) | (byte << 24), scale, 3);
}
extern "C" int er_k_w4_cvt_probe(float* out_dev, void* stream) {
    if (!out_dev) return fail(ER_ERR_INVALID, "er_k_w4_cvt_probe: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(w4_cvt_probe_kernel, dim3(W4_E_MAX - W4_E_MIN + 1), dim3(256), 0, st, out_dev);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

// er_k_gemv_form's checks on a canonical MXFP4 block in place of args->w (not read): ER_FORM_ROW of qkv, fc1 and fc2 with fp16 or e4m3
// caches.  args names the fp16 row form the step would launch (w_half, nw, rw: checked like er_k_gemv_form's); the nibble kernel runs in
// the projection's own nibble shape (er_decode_proj.h launch_proj_w4).  Also the four matrix-core forms (ER_FORM_MFMA, _MFMA_XT, _NARROW,
// _NARROW_DEFER) of qkv, out_proj, fc1 and fc2.  Both go through er_k_gemv_form's own path: proj_entry builds the quad-interleaved or the
// tiled nibble copy (er_w4_map.h, er_w4_tile_map.h) and run_proj launches the nibble kernels.  Everything else - ER_FORM_VALU, ER_FORM_ROWS8,
// the lm_head - is refused before any launch.
extern "C" int er_k_gemv_form_w4(const er_k_gemv_form_args* f, const void* block_dev, void* stream) {
    if (!f || !block_dev) return fail(ER_ERR_INVALID, "er_k_gemv_form_w4: null argument");
    er_k_gemv_form_args g = *f;
    g.w = block_dev;
    if (!g.w_half) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w4: the nibbles stand in for fp16 row forms (set w_half)");
    if (g.form != ER_FORM_ROW && !form_mfma(g.form))
        return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w4: only the row forms and the matrix-core forms stream nibbles (form %d)", g.form);
    Proj proj = PROJ_QKV;
    ERCHK(gemv_form_check(g, &proj));
    if (form_mfma(g.form)) {
        if (proj == PROJ_HEAD) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w4: the lm_head has no nibble form");
        if (!w4t::shape_ok(g.n, g.k)) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w4: k %d must be a multiple of %d", g.k, w4t::KW);
    } else {
        if (!w4_has_row_form(proj)) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w4: %s has no nibble form", proj == PROJ_OUT ? "out_proj" : "the lm_head");
        if (!w4map::shape_ok(g.n, g.k)) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w4: n %d must be a multiple of 4 (rows are streamed in quads)", g.n);
    }
    if (proj == PROJ_QKV && !g.kv_half) return fail(ER_ERR_UNSUPPORTED, "er_k_gemv_form_w4: fp4 weights go with an fp16 or an e4m3 cache, not fp32");
    // proj_entry interleaves (w4_interleave_kernel) or tiles (w4_tile_kernel) the block and synchronises
    return gemv_form_t<_Float16>(g, proj, (hipStream_t)stream, WSRC_QUADS, WSRC_TILED_NIBBLES);
}

// ---- the fused single-row MLP on caller-owned operands.  er_k_mlp_transpose makes the k-major copy the decode context keeps per
// layer; er_k_mlp_sparse enqueues one layer's two launches and returns - it allocates nothing and does not synchronise, so a caller
// can capture it into a graph.
extern "C" int er_k_mlp_transpose(const void* w2, void* w2t, int w_half, void* stream) {
    if (!w2 || !w2t) return fail(ER_ERR_INVALID, "er_k_mlp_transpose: null argument");
    hipStream_t st = (hipStream_t)stream;
    HIPRET(w_half ? launch_transpose_w2<_Float16>(w2, w2t, st) : launch_transpose_w2<float>(w2, w2t, st));
    return ER_OK;
}

extern "C" int er_k_mlp_sparse(const er_k_mlp_sparse_args* f, void* stream) {
    if (!f) return fail(ER_ERR_INVALID, "er_k_mlp_sparse: null args");
    if (!f->w1 || !f->b1 || !f->w2t || !f->zero_row || !f->b2 || !f->x || !f->ln_w || !f->ln_b || !f->h1_out || !f->y || !f->part)
        return fail(ER_ERR_INVALID, "er_k_mlp_sparse: null operand");
    hipStream_t st = (hipStream_t)stream;
    MlpArgs m{};
    m.W1 = f->w1; m.b1 = f->b1; m.W2T = f->w2t; m.zero_row = f->zero_row; m.xin = f->x; m.ln_w = f->ln_w; m.ln_b = f->ln_b; m.eps = f->eps;
    m.hout = f->h1_out; m.part = f->part; m.nnz = f->nnz; m.b2 = f->b2; m.resid = f->h1_out; m.out = f->y;
    HIPRET(f->w_half ? launch_mlp_fused<_Float16>(m, st) : launch_mlp_fused<float>(m, st));
    HIPRET(launch_mlp_finish(m, st));
    return ER_OK;
}

// live fc1 neurons per (layer, workgroup) of the last decode step: layers * 256 counts of 0 .. 24
extern "C" int er_mlp_nnz(er_ctx* c, int32_t* out, int n) {
    if (!c || !out) return fail(ER_ERR_INVALID, "er_mlp_nnz: null argument");
    if (!c->kv->plan.mlp_fused) return fail(ER_ERR_INVALID, "er_mlp_nnz: the reserved shape does not run the fused MLP");
    if (n != (int)c->kv->mlp_nnz.n) return fail(ER_ERR_INVALID, "er_mlp_nnz: %d counts asked, the context holds %zu (layers * 256)", n, c->kv->mlp_nnz.n);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, c->kv->mlp_nnz.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return ER_OK;
}

// wscale: wo is e4m3 bytes with these row scales (er_k_attn_outproj3_w8); otherwise fp32 or (w_half) fp16
static int attn_outproj3_entry(const float* q, const void* k, const void* v, int len, const void* wo, const float* wscale, const float* bo,
                               const float* resid, float* y, int l_cap, int kv_half, int w_half, void* stream) {
    // version 3 of the single-row decode attention: balanced chunks (16 heads x 16 chunks) + the merge fused into out_proj
    constexpr int H = 16, D = 96;
    if (len <= 0 || len > l_cap || !attn3_fits(l_cap, H)) return fail(ER_ERR_CAPACITY, "er_k_attn_outproj3: len %d / l_cap %d (<= %d)", len, l_cap, attn3_num_chunks(H) * ATTN3_CAP);
    hipStream_t st = (hipStream_t)stream;
    const int nch = attn3_num_chunks(H);
    DevBuf<float> blk;                         // partial outputs, then their {m, l}
    ERCHK(blk.ensure((size_t)H * nch * (D + 2)));
    float *part = blk.p, *part_ml = part + (size_t)H * nch * D;
    DevBuf<char> wblk;                         // allocated and filled in front of the first launch
    if (wscale) {
        ERCHK(w8_block_of(wblk, wo, wscale, H * D, H * D, st));
        wo = wblk.p;
    }
    AttnDecArgs a = attn_dec_args(H, D, l_cap);
    a.q = q; a.kcache = k; a.vcache = v; a.fixed_len = len; a.part = part; a.part_ml = part_ml;
    hipError_t e = launch_attn_partial3_d<D>(a, kv_half != 0, nch, 1, st);
    OutMergeArgs m{};
    m.W = wo; m.bias = bo; m.resid = resid; m.out = y; m.part_o = part; m.part_ml = part_ml; m.N = H * D;
    if (e == hipSuccess)
        e = wscale ? launch_outproj_merge<w8_t, D>(m, nch, st)
                   : w_half ? launch_outproj_merge<_Float16, D>(m, nch, st) : launch_outproj_merge<float, D>(m, nch, st);
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

extern "C" int er_k_attn_outproj3(const float* q, const void* k, const void* v, int len, const void* wo, const float* bo,
                                  const float* resid, float* y, int l_cap, int kv_half, int w_half, void* stream) {
    return attn_outproj3_entry(q, k, v, len, wo, nullptr, bo, resid, y, l_cap, kv_half, w_half, stream);
}

extern "C" int er_k_attn_outproj3_w8(const float* q, const void* k, const void* v, int len, const void* wo_q, const float* wo_scale,
                                     const float* bo, const float* resid, float* y, int l_cap, int kv_half, void* stream) {
    if (!wo_q || !wo_scale) return fail(ER_ERR_INVALID, "er_k_attn_outproj3_w8: null weights");
    return attn_outproj3_entry(q, k, v, len, wo_q, wo_scale, bo, resid, y, l_cap, kv_half, 0, stream);
}

extern "C" int er_k_gemm(const float* a, const float* b, const float* bias, const float* resid, float* cc, int m, int n, int k,
                         int lda, int ldb, int ldc, int b_is_kn, int relu, float div, void* stream) {
    if (k % 16) return fail(ER_ERR_INVALID, "er_k_gemm: k must be a multiple of 16");
    GemmArgs g = gemm_args_linear(a, lda, b, bias, cc, ldc, m, n, k, relu != 0, resid, ldc);
    g.ldb = ldb; g.b_is_kn = b_is_kn; g.kb_valid = k; g.div = div;
    HIPRET(launch_gemm(g, 1, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_gemm_f16(const float* a, const void* w, const float* bias, const float* resid, float* cc, int m, int n, int k,
                             int lda, int ldb, int ldc, int relu, void* stream) {
    if (k % 32) return fail(ER_ERR_INVALID, "er_k_gemm_f16: k must be a multiple of 32");
    GemmArgs g = gemm_args_linear(a, lda, w, bias, cc, ldc, m, n, k, relu != 0, resid, ldc);
    g.ldb = ldb;
    HIPRET(launch_gemm_f16(g, (hipStream_t)stream));
    return ER_OK;
}

// tail of the test entries that launch and wait: both errors are reported, the launch's first
static int gemm_sync_report(hipError_t e, hipStream_t st) {
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}
// the er_k_gemm_hh* entries: fp32 a [M][lda] -> an fp16 copy [M][K] that becomes g.A (in the product the producer writes it), then
// launch(g) and the wait
template <typename L>
static int gemm_hh_entry(const float* a, int lda, GemmArgs& g, hipStream_t st, L&& launch) {
    DevBuf<_Float16> a16;
    ERCHK(a16.ensure((size_t)g.M * g.K));
    hipLaunchKernelGGL(cvt_rows_f16_kernel, dim3(ew_grid((long long)g.M * g.K)), dim3(ER_WG), 0, st, a, a16.p, (long long)g.M, g.K, lda, g.K);
    g.A = reinterpret_cast<const float*>(a16.p); g.lda = g.K;
    return gemm_sync_report(launch(g), st);
}

// fp16 x fp16 LDS-DMA GEMM (gemm_hh_mfma_kernel): a is converted to an fp16 copy first,
// c16_out (optional, device fp16 [m][n]) receives the epilogue's fp16 copy of the result
extern "C" int er_k_gemm_hh(const float* a, const void* w, const float* bias, const float* resid, float* cc, void* c16_out, int m,
                            int n, int k, int lda, int ldb, int ldc, int relu, void* stream) {
    if (k % 64 || (ldb & 7)) return fail(ER_ERR_INVALID, "er_k_gemm_hh: k must be a multiple of 64, ldb of 8");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g = gemm_args_linear(nullptr, k, w, bias, cc, ldc, m, n, k, relu != 0, resid, ldc);
    g.ldb = ldb; g.c16 = reinterpret_cast<_Float16*>(c16_out); g.ldc16 = n;
    return gemm_hh_entry(a, lda, g, st, [&](const GemmArgs& ga) { return launch_gemm_hh(ga, st); });
}

// ---- er_k_gemm_epi: one GEMM family with the WHOLE plain epilogue the product uses (bias, / div, relu, adaLN gate rows, a residual
// that may be one table shared by every batch, the fp16 copy).  It fills GemmArgs and calls the family's own launcher - no kernel of
// its own - so ER_GEMM_TILE / ER_GEMM_F32_DMA / ER_GEMM_STREAM / force_tile select the form exactly as they do for the product.
extern "C" int er_k_gemm_epi(const er_k_gemm_epi_args* f, void* stream) {
    if (!f) return fail(ER_ERR_INVALID, "er_k_gemm_epi: null args");
    const int fam = f->family;
    if (fam < ER_GEMM_F32 || fam > ER_GEMM_HH) return fail(ER_ERR_INVALID, "er_k_gemm_epi: family %d", fam);
    const bool hh = fam == ER_GEMM_HH;
    if (!f->a || !f->w || (!f->c && !(hh && f->c16))) return fail(ER_ERR_INVALID, "er_k_gemm_epi: a, w and an output are required");
    if (f->m <= 0 || f->n <= 0 || f->k <= 0 || f->ldc < f->n) return fail(ER_ERR_INVALID, "er_k_gemm_epi: m %d, n %d, k %d, ldc %d", f->m, f->n, f->k, f->ldc);
    if (fam == ER_GEMM_F32 && (f->k % 16 || (f->lda & 3) || (f->ldb & 3))) return fail(ER_ERR_INVALID, "er_k_gemm_epi: fp32 needs k a multiple of 16, lda and ldb of 4");
    if ((fam == ER_GEMM_F16 || fam == ER_GEMM_F16S) && (f->k % 32 || (f->lda & 3) || (f->ldb & 7)))
        return fail(ER_ERR_INVALID, "er_k_gemm_epi: the fp16-weight families need k a multiple of 32, lda of 4, ldb of 8");
    if (hh && (f->k % 64 || (f->ldb & 7))) return fail(ER_ERR_INVALID, "er_k_gemm_epi: the LDS-DMA fp16 family needs k a multiple of 64, ldb of 8");
    if (f->lda < f->k || f->ldb < f->k) return fail(ER_ERR_INVALID, "er_k_gemm_epi: lda %d / ldb %d below k %d", f->lda, f->ldb, f->k);
    if (f->c16 && !hh) return fail(ER_ERR_INVALID, "er_k_gemm_epi: c16 is written by the LDS-DMA fp16 family only");
    if (f->force_tile < 0 || f->force_tile > 4 || (f->force_tile && !hh)) return fail(ER_ERR_INVALID, "er_k_gemm_epi: force_tile 0..4, LDS-DMA fp16 family only (the others read ER_GEMM_TILE)");
    if (f->gate && (f->gate_rows <= 0 || f->gate_bstride < f->n)) return fail(ER_ERR_INVALID, "er_k_gemm_epi: a gate needs gate_rows > 0 and gate_bstride >= n");
    if (f->resid && f->ldr < f->n) return fail(ER_ERR_INVALID, "er_k_gemm_epi: ldr %d below n %d", f->ldr, f->n);
    if (f->resid_mod < 0 || (f->resid_mod && !f->resid)) return fail(ER_ERR_INVALID, "er_k_gemm_epi: resid_mod %d (>= 0, with a residual)", f->resid_mod);
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g = gemm_args_linear(f->a, f->lda, f->w, f->bias, f->c, f->ldc, f->m, f->n, f->k, false, f->resid, f->ldr);
    g.ldb = f->ldb; g.kb_valid = f->k; g.relu = f->relu; g.div = f->div; g.resid_mod = f->resid_mod;
    g.gate = f->gate; g.gate_rows = f->gate_rows; g.gate_bstride = f->gate_bstride;
    if (fam == ER_GEMM_F32) { HIPRET(launch_gemm(g, 1, st)); return ER_OK; }
    if (fam == ER_GEMM_F16) { HIPRET(launch_gemm_f16(g, st)); return ER_OK; }
    if (fam == ER_GEMM_F16S) { HIPRET(launch_gemm_f16s(g, st)); return ER_OK; }
    g.c16 = reinterpret_cast<_Float16*>(f->c16); g.ldc16 = f->ldc;
    return gemm_hh_entry(f->a, f->lda, g, st, [&](const GemmArgs& ga) { return launch_gemm_hh(ga, st, f->force_tile); });
}

extern "C" int er_k_gemm_hh_qkv(const float* a, const void* w, const float* bias, void* qk16_out, void* vt_out, int m, int n, int k,
                                int rows_per_batch, int force_tile, void* stream) {
    if (k % 64 || n % 192 || m % 64 || rows_per_batch <= 0 || rows_per_batch % 64 || m % rows_per_batch)
        return fail(ER_ERR_INVALID, "er_k_gemm_hh_qkv: k, m, rows_per_batch multiples of 64, n of 192");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g = gemm_args_linear(nullptr, k, w, bias, nullptr, n, m, n, k, false, nullptr, n);
    g.c16 = reinterpret_cast<_Float16*>(qk16_out); g.ldc16 = n;
    g.vt16 = reinterpret_cast<_Float16*>(vt_out); g.vt_col0 = 2 * (n / 3); g.vt_rows = rows_per_batch; g.vt_ld = rows_per_batch;
    return gemm_hh_entry(a, k, g, st, [&](const GemmArgs& ga) { return launch_gemm_hh(ga, st, force_tile); });
}

extern "C" int er_k_gemm_hh_geglu(const float* a, const void* w, const float* bias, void* out16, int m, int f, int k, int force_tile,
                                  void* stream) {
    // out16[m][f] = fp16(GEGLU(fp16(a) . w^T + bias)), w = the [2f][k] fp16 weight in the checkpoint's order (value rows, then gate rows):
    // the entry builds the permuted copy the product keeps per layer (geglu_permute_kernel) and runs the fused kernel
    if (!a || !w || !bias || !out16) return fail(ER_ERR_INVALID, "er_k_gemm_hh_geglu: a, w, bias and out16 are required (the permute pass reads the bias)");
    if (k % 64 || f % 64 || m <= 0) return fail(ER_ERR_INVALID, "er_k_gemm_hh_geglu: k and f must be multiples of 64");
    if (force_tile != 0 && force_tile != 1 && force_tile != 2 && force_tile != 4) return fail(ER_ERR_INVALID, "er_k_gemm_hh_geglu: force_tile 0 / 1 / 2 / 4");
    hipStream_t st = (hipStream_t)stream;
    DevBuf<_Float16> wpb;            // permuted weight
    DevBuf<float> bpb;               // permuted bias
    ERCHK(wpb.ensure((size_t)2 * f * k));
    ERCHK(bpb.ensure((size_t)2 * f));
    hipLaunchKernelGGL(geglu_permute_kernel, dim3(2 * f), dim3(ER_WG), 0, st, reinterpret_cast<const _Float16*>(w), bias, wpb.p, bpb.p, f, k);
    GemmArgs g = gemm_args_linear(nullptr, k, wpb.p, bpb.p, nullptr, 2 * f, m, 2 * f, k, false, nullptr, 2 * f);
    g.c16 = reinterpret_cast<_Float16*>(out16); g.ldc16 = f;
    return gemm_hh_entry(a, k, g, st, [&](const GemmArgs& ga) { return launch_gemm_hh_geglu(ga, st, force_tile); });
}

extern "C" int er_k_gemm_f16s(const float* a, const void* w, const float* bias, const float* resid, float* cc, int m, int n, int k,
                              int lda, int ldb, int ldc, int relu, void* stream) {
    if (k % 32) return fail(ER_ERR_INVALID, "er_k_gemm_f16s: k must be a multiple of 32");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g = gemm_args_linear(a, lda, w, bias, cc, ldc, m, n, k, relu != 0, resid, ldc);
    g.ldb = ldb;
    // ER_K_GEMM_F16S_FORM = reg / dma pins one of the two forms linear_hs chooses between (unit tests compare them bit for bit)
    const bool force_reg = env_is("ER_K_GEMM_F16S_FORM", 'r');
    if (k % XBK == 0 && !(ldb & 7) && !force_reg) {      // the product path of the fast-mode prefill: split pass + LDS-DMA kernel (linear_hs)
        DevBuf<_Float16> hi, lo;
        ERCHK(hi.ensure((size_t)m * k));
        ERCHK(lo.ensure((size_t)m * k));
        HIPRET(launch_split_rows_f16(a, hi.p, lo.p, (long long)m, k, lda, st));
        g.A = reinterpret_cast<const float*>(hi.p); g.a_lo = lo.p; g.lda = k;
        return gemm_sync_report(launch_gemm_hh_split(g, st), st);
    }
    HIPRET(launch_gemm_f16s(g, st));      // k % 64 != 0: the register-staged kernel
    return ER_OK;
}

extern "C" int er_k_flash_attn_f16(const float* q, const float* k, const float* v, float* o, int B, int H, int N, int M,
                                   void* stream) {
    // q/k/v/o: [B, rows, H*64] fp32, heads side by side in a row (the layout the projections produce)
    FlashArgs a{};
    a.Q = q; a.K = k; a.V = v; a.O = o; a.N = N; a.M = M;
    a.ldq = a.ldk = a.ldv = a.ldo = H * FA_D;
    a.qs_b = (long long)N * H * FA_D; a.os_b = a.qs_b; a.ks_b = (long long)M * H * FA_D; a.vs_b = a.ks_b;
    a.head_stride = FA_D; a.scale = 1.0f / sqrtf((float)FA_D);
    HIPRET(launch_flash_attn_f16(a, H, B, (hipStream_t)stream));
    return ER_OK;
}

// the LDS-DMA variant (q / k / v in fp16, V transposed per head): converts and transposes the fp32 inputs first - in the DiT
// path the qkv GEMM epilogue and transpose_v_f16_kernel produce these operands - and returns the fp16 output widened to fp32
extern "C" int er_k_flash_attn_hh(const float* q, const float* k, const float* v, float* o, int B, int H, int N, int M, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int C = H * FA_D, Mp = (M + 63) / 64 * 64;
    DevBuf<_Float16> q16b, k16b, v16b, vtb, o16b;
    ERCHK(q16b.ensure((size_t)B * N * C));
    ERCHK(k16b.ensure((size_t)B * M * C));
    ERCHK(v16b.ensure((size_t)B * M * C));
    ERCHK(vtb.ensure((size_t)B * H * 64 * Mp));
    ERCHK(o16b.ensure((size_t)B * N * C));
    _Float16 *q16 = q16b.p, *k16 = k16b.p, *v16 = v16b.p, *vt = vtb.p, *o16 = o16b.p;
    hipLaunchKernelGGL(cvt_rows_f16_kernel, dim3(ew_grid((long long)B * N * C)), dim3(ER_WG), 0, st, q, q16, (long long)B * N, C, C, C);
    hipLaunchKernelGGL(cvt_rows_f16_kernel, dim3(ew_grid((long long)B * M * C)), dim3(ER_WG), 0, st, k, k16, (long long)B * M, C, C, C);
    hipLaunchKernelGGL(cvt_rows_f16_kernel, dim3(ew_grid((long long)B * M * C)), dim3(ER_WG), 0, st, v, v16, (long long)B * M, C, C, C);
    hipLaunchKernelGGL(transpose_v_f16_kernel, dim3(Mp / 64, H, B), dim3(ER_WG), 0, st, v16, vt, M, Mp, C, (long long)M * C);
    FlashHArgs a{};
    a.Q = q16; a.K = k16; a.Vt = vt; a.O16 = o16; a.N = N; a.M = M; a.ldq = a.ldk = a.ldo = C; a.ldvt = Mp;
    a.qs_b = a.os_b = (long long)N * C; a.ks_b = (long long)M * C; a.vts_h = 64LL * Mp; a.vts_b = (long long)H * 64 * Mp;
    a.head_stride = FA_D; a.scale = 1.0f / sqrtf((float)FA_D);
    hipError_t e = launch_flash_attn_hh(a, H, B, st);
    hipLaunchKernelGGL(cvt_f16_rows_f32_kernel, dim3(ew_grid((long long)B * N * C)), dim3(ER_WG), 0, st, o16, o, (long long)B * N * C);
    hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

extern "C" int er_k_flash_attn_f32(const float* q, const float* k, const float* v, float* o, int B, int H, int N, int M, int D,
                                   int causal, void* stream) {
    // q/o: [B, N, H*D], k/v: [B, M, H*D] fp32, heads side by side in a row; causal: key j visible to query i iff j <= i + (M - N)
    if (D != 64 && D != 96) return fail(ER_ERR_UNSUPPORTED, "er_k_flash_attn_f32: head_dim %d (64, 96)", D);
    if (causal && M < N) return fail(ER_ERR_INVALID, "er_k_flash_attn_f32: causal needs M >= N");
    Flash32Args a = flash32_packed_args(q, k, v, o, H, N, M, D);
    DevBuf<float> po, pml;                                 // key-range split of the causal prefill shape (k_flash_attn_f32.h, KSP)
    if (flash32_ksplit(N, H, B, D, causal != 0)) {
        ERCHK(po.ensure(flash32_part_o_floats(B, H, N, D)));
        ERCHK(pml.ensure(flash32_part_ml_floats(B, H, N)));
        a.part_o = po.p; a.part_ml = pml.p;
    }
    hipError_t e = launch_flash_attn_f32(a, D, causal != 0, H, B, (hipStream_t)stream);
    if (po.p) hipStreamSynchronize((hipStream_t)stream);
    HIPRET(e);
    return ER_OK;
}

extern "C" int er_k_flash_attn_f16s(const float* q, const float* k, const float* v, float* o, int B, int H, int N, int M, int causal,
                                    void* stream) {
    // q/o [B, N, H*96], k/v [B, M, H*96] fp32 holding fp16-representable k / v values (the fast-mode prefill attention)
    if (causal && M < N) return fail(ER_ERR_INVALID, "er_k_flash_attn_f16s: causal needs M >= N");
    constexpr int D = 96;
    HIPRET(launch_flash_attn_f16s(flash32_packed_args(q, k, v, o, H, N, M, D), D, causal != 0, H, B, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_layernorm(const float* x, const float* w, const float* b, float* y, int rows, int cols, float eps, void* stream) {
    HIPRET(launch_layernorm(x, w, b, y, rows, cols, cols, cols, eps, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_softmax(float* s, int rows, int cols, int ld, int causal, void* stream) {
    HIPRET(launch_softmax_rows(s, rows, cols, (long long)ld, ld, 0LL, 1, causal, 0, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_softmax_batched(float* s, int rows, int cols, long long ld, int ld_pad, int batch, long long batch_stride, int causal,
                                    int causal_off, void* stream) {
    if (!s || rows < 1 || cols < 1 || ld_pad < cols || ld < ld_pad || batch < 1 || batch > 65535 || causal_off < 0 ||
        (batch > 1 && batch_stride < (long long)rows * ld))
        return fail(ER_ERR_INVALID, "er_k_softmax_batched: bad argument");
    HIPRET(launch_softmax_rows(s, rows, cols, ld, ld_pad, batch_stride, batch, causal ? 1 : 0, causal_off, (hipStream_t)stream));
    return ER_OK;
}

// ---- the once-per-sample row, element-wise and K/V scatter kernels (k_rowops.h, k_dit.h, k_gemm.h split_rows_f16_kernel) through the
// launchers the prefill, the point encoder, the CLIP front and the DiT sampler call.  Every entry refuses before it launches.
extern "C" int er_k_kv_scatter(float* qkv, void* kcache, void* vcache, int kv_half, int m, int s, int hidden, int head_dim, int l_cap,
                               long long kv_bstride, void* stream) {
    if (!qkv || !kcache || !vcache || (kv_half != 1 && kv_half != 2) || m < 1 || s < 1 || m % s || s > l_cap || hidden < 4 || hidden % 4 ||
        head_dim < 4 || head_dim % 4 || hidden % head_dim || kv_bstride % 4 || kv_bstride < (long long)hidden * l_cap)
        return fail(ER_ERR_INVALID, "er_k_kv_scatter: bad argument");
    HIPRET(launch_kv_scatter(qkv, kcache, vcache, kv_half == 2, m, s, hidden, head_dim, l_cap, kv_bstride, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_split_rows_f16(const float* x, void* hi, void* lo, long long rows, int cols, int ldx, void* stream) {
    if (!x || !hi || !lo || rows < 1 || cols < 4 || cols % 4 || ldx < cols || ldx % 4)
        return fail(ER_ERR_INVALID, "er_k_split_rows_f16: bad argument");
    HIPRET(launch_split_rows_f16(x, (_Float16*)hi, (_Float16*)lo, rows, cols, ldx, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_add_pos(const float* emb, const float* pos, float* out, int batch, int s, int c, int pos0, void* stream) {
    if (!emb || !pos || !out || batch < 1 || s < 1 || c < 4 || c % 4 || pos0 < 0) return fail(ER_ERR_INVALID, "er_k_add_pos: bad argument");
    HIPRET(launch_add_pos(emb, pos, out, batch, s, c, pos0, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_gather_rows(const float* table, int table_rows, const int32_t* ids_host, float* out, int rows, int c, long long ldo,
                                void* stream) {
    if (!table || !ids_host || !out || table_rows < 1 || rows < 1 || c < 1 || ldo < c) return fail(ER_ERR_INVALID, "er_k_gather_rows: bad argument");
    for (int i = 0; i < rows; ++i)
        if (ids_host[i] < 0 || ids_host[i] >= table_rows) return fail(ER_ERR_INVALID, "er_k_gather_rows: id %d out of range", ids_host[i]);
    hipStream_t st = (hipStream_t)stream;
    DevBuf<int> ids;
    ERCHK(ids.ensure((size_t)rows));
    HIPCHK(hipMemcpyAsync(ids.p, ids_host, (size_t)rows * sizeof(int), hipMemcpyHostToDevice, st));
    hipError_t e = launch_gather_rows(table, ids.p, out, rows, c, ldo, st);
    hipError_t e2 = hipStreamSynchronize(st);      // ids is freed on return
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

extern "C" int er_k_point_embed(const float* pts, const float* basis, float* out, long long m, int f, int ldo, void* stream) {
    if (!pts || !basis || !out || m < 1 || f < 1 || ldo < 2 * f + 3) return fail(ER_ERR_INVALID, "er_k_point_embed: bad argument");
    HIPRET(launch_point_embed(pts, basis, out, m, f, ldo, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_geglu(const float* u, float* out, long long rows, int f, void* stream) {
    if (!u || !out || rows < 1 || f < 1) return fail(ER_ERR_INVALID, "er_k_geglu: bad argument");
    HIPRET(launch_geglu(u, out, rows, f, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_gelu(const float* x, float* y, long long n, void* stream) {
    if (!x || !y || n < 1) return fail(ER_ERR_INVALID, "er_k_gelu: bad argument");
    HIPRET(launch_gelu(x, y, n, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_silu(const float* x, float* y, long long n, void* stream) {
    if (!x || !y || n < 1) return fail(ER_ERR_INVALID, "er_k_silu: bad argument");
    HIPRET(launch_silu(x, y, n, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_ln_modulate(const float* x, float* y, int rows, int rows_per_batch, int cols, const float* table, const float* tvec,
                                long long t_bstride, long long t_cstride, int shift_idx, int scale_idx, void* y16, void* stream) {
    if (!x || !y || !table || !tvec || rows < 1 || rows_per_batch < 1 || rows % rows_per_batch || t_bstride < 0 || t_bstride % 4 ||
        t_cstride < 0 || t_cstride % 4 || shift_idx < 0 || scale_idx < 0)
        return fail(ER_ERR_INVALID, "er_k_ln_modulate: bad argument");
    if (cols != 1024) return fail(ER_ERR_INVALID, "er_k_ln_modulate: width %d (1024)", cols);
    HIPRET(dit_ln_mod(x, y, rows, rows_per_batch, table, tvec, t_bstride, t_cstride, shift_idx, scale_idx, (hipStream_t)stream, (_Float16*)y16));
    return ER_OK;
}

extern "C" int er_k_adaln_gate(const float* table, const float* tada, float* out, int batch, int c, int idx, void* stream) {
    if (!table || !tada || !out || batch < 1 || c < 1 || idx < 0 || idx > 5) return fail(ER_ERR_INVALID, "er_k_adaln_gate: bad argument");
    HIPRET(launch_adaln_gate(table, tada, out, batch, c, idx, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_adaln_gate_all(const float* const* tables_host, const float* tada, float* out, int layers, int batch, int c, void* stream) {
    if (!tables_host || !tada || !out || layers < 1 || batch < 1 || c < 1) return fail(ER_ERR_INVALID, "er_k_adaln_gate_all: bad argument");
    for (int l = 0; l < layers; ++l)
        if (!tables_host[l]) return fail(ER_ERR_INVALID, "er_k_adaln_gate_all: null table %d", l);
    hipStream_t st = (hipStream_t)stream;
    DevBuf<const float*> tabs;
    ERCHK(tabs.ensure((size_t)layers));
    HIPCHK(hipMemcpyAsync(tabs.p, tables_host, (size_t)layers * sizeof(float*), hipMemcpyHostToDevice, st));
    hipError_t e = launch_adaln_gate_all(tabs.p, tada, out, layers, batch, c, st);
    hipError_t e2 = hipStreamSynchronize(st);      // tabs is freed on return
    HIPRET(e);
    HIPRET(e2);
    return ER_OK;
}

extern "C" int er_k_timestep_embed(const float* t, float* out, int batch, int half, void* stream) {
    if (!t || !out || batch < 1 || half < 1) return fail(ER_ERR_INVALID, "er_k_timestep_embed: bad argument");
    HIPRET(launch_timestep_embed(t, out, batch, half, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_ddim_cfg_step(float* latents, const float* pred, long long n, int prediction_type, float guidance, float sa_t,
                                  float sb_t, float sa_p, float sb_p, void* stream) {
    if (!latents || !pred || n < 1 || (prediction_type != ER_PRED_V_PREDICTION && prediction_type != ER_PRED_EPSILON))
        return fail(ER_ERR_INVALID, "er_k_ddim_cfg_step: bad argument");
    HIPRET(launch_ddim_cfg_step(prediction_type == ER_PRED_EPSILON, latents, pred, n, guidance, sa_t, sb_t, sa_p, sb_p, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_clip_preprocess(const float* img, float* out, int batch, int h, int w, int out_size, void* stream) {
    if (!img || !out || batch < 1 || h < 1 || w < 1 || out_size < 1) return fail(ER_ERR_INVALID, "er_k_clip_preprocess: bad argument");
    HIPRET(launch_clip_preprocess(img, out, batch, h, w, out_size, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_clip_im2col(const float* px, float* a, int batch, int s, int p, int lda, void* stream) {
    if (!px || !a || batch < 1 || p < 1 || s < p || s % p || lda < 3 * p * p) return fail(ER_ERR_INVALID, "er_k_clip_im2col: bad argument");
    HIPRET(launch_clip_im2col(px, a, batch, s, p, lda, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_clip_assemble(const float* patches, const float* cls, const float* pos, float* x, int batch, int np, int c, void* stream) {
    if (!patches || !cls || !pos || !x || batch < 1 || np < 1 || c < 1) return fail(ER_ERR_INVALID, "er_k_clip_assemble: bad argument");
    HIPRET(launch_clip_assemble(patches, cls, pos, x, batch, np, c, (hipStream_t)stream));
    return ER_OK;
}

extern "C" int er_k_score_rows(const float* logits, const int32_t* labels, int batch, int seq_len, int vocab, float* nll_out,
                               int32_t* pred_out, float* loss_out, void* stream) {
    if (!logits || !labels || !nll_out || batch <= 0 || seq_len <= 0 || vocab <= 0 || vocab > ER_HEAD_MAX_VOCAB ||
        (long long)batch * seq_len * vocab > 0x7fffffffLL)
        return fail(ER_ERR_INVALID, "er_k_score_rows: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int M = batch * seq_len;
    HIPRET(launch_score_rows(logits, labels, M, seq_len, vocab, nll_out, pred_out, st));
    if (loss_out) HIPRET(launch_score_reduce(nll_out, labels, M, seq_len, loss_out, st));
    return ER_OK;
}

// One step of a sampling head on row state the caller gives: what er_k_sample_head and er_k_sample_head_ctl share.  `who` names the
// entry in the error text; ctl null: sample_head_kernel, else sample_head_ctl_kernel with the controls ctl->s, leaving its log-probs
// and kept counts of this step in ctl's buffers for the entry to copy.  Returns after the stream has drained.
struct HeadUnitCtl {
    const er_sampling* s;
    DevBuf<HeadCtlDev> dev;
    DevBuf<float> lpm, lpp;            // [B][step + 1]
    DevBuf<int> nk;                    // [B]
};
static int head_unit_step(const char* who, const float* logits, const er_decode_params* p, int vocab, int eos, int pad, int B, int step,
                          const int32_t* last_tok, const int32_t* counter, const int32_t* unfinished, int32_t* next_tok,
                          int32_t* counter_out, int32_t* unfinished_out, HeadUnitCtl* ctl, hipStream_t st) {
    if (!logits || !p || B <= 0 || step < 0 || vocab <= 0 || vocab > ER_HEAD_MAX_VOCAB || !last_tok || !counter || !unfinished ||
        !next_tok || !counter_out || !unfinished_out)
        return fail(ER_ERR_INVALID, "%s: bad argument", who);
    const size_t b = (size_t)B, ld = (size_t)step + 1;
    DevBuf<int> sb;
    DevBuf<DecodeParamsDev> dpd;
    DevBuf<long long> ids;
    ERCHK(sb.ensure(gen_state_ints(b)));
    ERCHK(dpd.ensure(1));
    ERCHK(ids.ensure(b * ld));
    std::vector<int> h(gen_state_ints(b), 0);
    const GenState hs = gen_state_carve(h.data(), b);      // the same state on the host
    for (size_t i = 0; i < b; ++i) {
        hs.tok[i] = last_tok[i]; hs.counter[i] = counter[i]; hs.ngen[i] = step;
        hs.unfinished[i] = unfinished[i]; hs.eos_step[i] = -1;
    }
    *hs.n_unfinished = B;
    HIPCHK(hipMemcpy(sb.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
    const GenState gs = gen_state_carve(sb.p, b);
    const DecodeParamsDev dp = decode_params_dev(*p, ctl && ctl->s->top_k_set ? ctl->s->top_k : p->top_k, step + 1, eos, pad, vocab);
    HIPCHK(hipMemcpy(dpd.p, &dp, sizeof(dp), hipMemcpyHostToDevice));
    if (ctl) {
        ERCHK(ctl->dev.ensure(1));
        ERCHK(ctl->lpm.ensure(b * ld));
        ERCHK(ctl->lpp.ensure(b * ld));
        ERCHK(ctl->nk.ensure(b));
        const HeadCtlDev hc{ctl->s->temperature, ctl->s->top_p};
        HIPCHK(hipMemcpy(ctl->dev.p, &hc, sizeof(hc), hipMemcpyHostToDevice));
        const HeadCtlOut lp{ctl->lpm.p, ctl->lpp.p, ctl->nk.p, step + 1};
        hipLaunchKernelGGL(sample_head_ctl_kernel, dim3(B), dim3(ER_WG), sample_head_lds(vocab), st, logits, dpd.p, ctl->dev.p, gs, ids.p,
                           step + 1, lp);
    } else {
        hipLaunchKernelGGL(sample_head_kernel, dim3(B), dim3(ER_WG), sample_head_lds(vocab), st, logits, dpd.p, gs, ids.p, step + 1);
    }
    const hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(st);
    HIPRET(e);
    HIPRET(e2);
    HIPCHK(hipMemcpy(h.data(), sb.p, h.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < b; ++i) { next_tok[i] = hs.tok[i]; counter_out[i] = hs.counter[i]; unfinished_out[i] = hs.unfinished[i]; }
    return ER_OK;
}

extern "C" int er_k_sample_head(const float* logits, const er_decode_params* p, int vocab, int eos, int pad, int B, int step,
                                const int32_t* last_tok, const int32_t* counter, const int32_t* unfinished, int32_t* next_tok,
                                int32_t* counter_out, int32_t* unfinished_out, void* stream) {
    if (p && p->mode == ER_SAMPLE && p->top_k <= 0)        // as er_decode: only er_sampling can switch the top-k filter off
        return fail(ER_ERR_INVALID, "er_k_sample_head: top_k must be > 0 in sample mode");
    return head_unit_step("er_k_sample_head", logits, p, vocab, eos, pad, B, step, last_tok, counter, unfinished, next_tok, counter_out,
                          unfinished_out, nullptr, (hipStream_t)stream);
}

extern "C" int er_k_sample_head_ctl(const float* logits, const er_decode_params* p, const er_sampling* s, int vocab, int eos, int pad,
                                    int B, int step, const int32_t* last_tok, const int32_t* counter, const int32_t* unfinished,
                                    int32_t* next_tok, int32_t* counter_out, int32_t* unfinished_out, float* lp_model, float* lp_policy,
                                    int32_t* n_kept, void* stream) {
    const er_sampling dflt{1.0f, 1.0f, 0, 0, 0};
    if (!s) s = &dflt;
    if (!(s->temperature > 0.0f) || !(s->temperature <= 3.402823466e38f) || !(s->top_p > 0.0f) || !(s->top_p <= 1.0f) || (s->top_k_set && s->top_k < 0))
        return fail(ER_ERR_INVALID, "er_k_sample_head_ctl: temperature %g / top_p %g / top_k %d out of range", (double)s->temperature, (double)s->top_p, s->top_k);
    HeadUnitCtl ctl{s};
    ERCHK(head_unit_step("er_k_sample_head_ctl", logits, p, vocab, eos, pad, B, step, last_tok, counter, unfinished, next_tok, counter_out,
                         unfinished_out, &ctl, (hipStream_t)stream));
    const size_t pitch = (size_t)(step + 1) * sizeof(float);
    if (lp_model) HIPCHK(hipMemcpy2D(lp_model, sizeof(float), ctl.lpm.p + step, pitch, sizeof(float), (size_t)B, hipMemcpyDeviceToHost));
    if (lp_policy) HIPCHK(hipMemcpy2D(lp_policy, sizeof(float), ctl.lpp.p + step, pitch, sizeof(float), (size_t)B, hipMemcpyDeviceToHost));
    if (n_kept) HIPCHK(hipMemcpy(n_kept, ctl.nk.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    return ER_OK;
}

// ------------------------------------------------------------------------------------ detokenise (host)
extern "C" int er_k_fps(const float* pts, int B, int N, int S, int32_t* idx, void* stream) {
    if (!pts || !idx || B <= 0 || B > 65535 || N <= 0 || S <= 0 || S > N) return fail(ER_ERR_INVALID, "er_k_fps: bad argument");
    hipStream_t st = (hipStream_t)stream;
    DevBuf<float> dist;
    if (N > FPS_REG_MAX) ERCHK(dist.ensure((size_t)B * N));
    hipError_t e = launch_fps(pts, B, N, S, idx, dist.p, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e != hipSuccess || e2 != hipSuccess) return fail(ER_ERR_HIP, "er_k_fps: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return ER_OK;
}

// ------------------------------------------------------------------------------------ reconstruction fidelity (k_fidelity.h)
extern "C" int er_k_nn_dist2(const float* a, const float* b, int B, int Na, int Nb, float* d2, int32_t* idx, void* stream) {
    if (!a || !b || !d2 || B <= 0 || B > 65535 || Na <= 0 || Nb <= 0 || Na > FID_MAX_N || Nb > FID_MAX_N)
        return fail(ER_ERR_INVALID, "er_k_nn_dist2: bad argument");
    hipStream_t st = (hipStream_t)stream;
    DevBuf<unsigned long long> packed;
    ERCHK(packed.ensure((size_t)B * Na));
    const hipError_t e = launch_nn_dist2(a, b, B, Na, Nb, d2, idx, packed.p, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e != hipSuccess || e2 != hipSuccess) return fail(ER_ERR_HIP, "er_k_nn_dist2: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return ER_OK;
}

extern "C" int er_k_surface_sample(const float* vertices, const int32_t* faces, const int32_t* vert_offset, const int32_t* face_offset,
                                   int B, int n, uint64_t seed, const uint32_t* stream_ids, float* points, int32_t* face_out,
                                   void* stream) {
    if (!vertices || !faces || !vert_offset || !face_offset || !points || B <= 0 || B > 65535 || n <= 0 || n > FID_MAX_N)
        return fail(ER_ERR_INVALID, "er_k_surface_sample: bad argument");
    std::vector<FidMesh> hm((size_t)B);
    int max_faces = 0;
    for (int m = 0; m < B; ++m) {
        const int v0 = vert_offset[m], nv = vert_offset[m + 1] - v0, f0 = face_offset[m], nf = face_offset[m + 1] - f0;
        if (v0 < 0 || nv < 0 || f0 < 0 || nf < 0) return fail(ER_ERR_INVALID, "er_k_surface_sample: offsets of mesh %d are not ascending", m);
        if (nf == 0) return fail(ER_ERR_INVALID, "er_k_surface_sample: mesh %d has no faces", m);
        if (nf > FID_MAX_FACES) return fail(ER_ERR_INVALID, "er_k_surface_sample: mesh %d has %d faces (at most %d)", m, nf, FID_MAX_FACES);
        hm[m] = FidMesh{v0, nv, f0, nf, stream_ids ? stream_ids[m] : (unsigned)m};
        max_faces = std::max(max_faces, nf);
    }
    hipStream_t st = (hipStream_t)stream;
    DevBuf<FidMesh> meshes;
    DevBuf<unsigned long long> cum, total;
    DevBuf<int> bad;
    ERCHK(meshes.ensure((size_t)B));
    ERCHK(cum.ensure((size_t)face_offset[B]));
    ERCHK(total.ensure((size_t)B));
    ERCHK(bad.ensure((size_t)B));
    HIPCHK(hipMemcpyAsync(meshes.p, hm.data(), hm.size() * sizeof(FidMesh), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(bad.p, 0, (size_t)B * sizeof(int), st));
    const unsigned chunks = (unsigned)std::min((max_faces + ER_WG - 1) / ER_WG, 1024);
    hipLaunchKernelGGL(face_weight_kernel, dim3(chunks, B), dim3(ER_WG), 0, st, vertices, faces, meshes.p, cum.p, bad.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(face_scan_kernel, dim3(B), dim3(ER_WG), 0, st, cum.p, meshes.p, total.p);
    HIPCHK(hipGetLastError());
    // the one blocking point: no vertex is read through an unchecked index, and no sample is drawn from a mesh without area
    std::vector<unsigned long long> htotal((size_t)B);
    std::vector<int> hbad((size_t)B);
    HIPCHK(hipMemcpyAsync(htotal.data(), total.p, htotal.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hbad.data(), bad.p, hbad.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int m = 0; m < B; ++m) {
        if (hbad[m]) return fail(ER_ERR_INVALID, "er_k_surface_sample: mesh %d has a face index outside its %d vertices", m, hm[m].nv);
        if (htotal[m] == 0) return fail(ER_ERR_INVALID, "er_k_surface_sample: mesh %d has zero area", m);
    }
    hipLaunchKernelGGL(surface_sample_kernel, dim3((n + ER_WG - 1) / ER_WG, B), dim3(ER_WG), 0, st, vertices, faces, meshes.p, cum.p,
                       total.p, n, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), points, face_out);
    const hipError_t e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e != hipSuccess || e2 != hipSuccess) return fail(ER_ERR_HIP, "er_k_surface_sample: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return ER_OK;
}

extern "C" int er_k_fidelity_metrics(const float* d2_ab, const float* d2_ba, int B, int Na, int Nb, float tau, double* metrics,
                                     void* stream) {
    if (!d2_ab || !d2_ba || !metrics || B <= 0 || B > 65535 || Na <= 0 || Nb <= 0 || Na > FID_MAX_N || Nb > FID_MAX_N)
        return fail(ER_ERR_INVALID, "er_k_fidelity_metrics: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = launch_fidelity_metrics(d2_ab, d2_ba, B, Na, Nb, tau, metrics, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e != hipSuccess || e2 != hipSuccess) return fail(ER_ERR_HIP, "er_k_fidelity_metrics: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return ER_OK;
}

extern "C" int er_meto_decode(const int32_t* tokens, int n, int bins, int backend, float* v, int32_t* f, int32_t* t, int32_t* nv,
                              int32_t* nf, int32_t* nt) {
    if (n < 0 || bins <= 0 || (n > 0 && !tokens) || !v || !f || !t || !nv || !nf || !nt)
        return fail(ER_ERR_INVALID, "er_meto_decode: bad argument");
    if (backend != ER_METO_LR_ABSCO && backend != ER_METO_LR) return fail(ER_ERR_UNSUPPORTED, "meto backend %d (LR_ABSCO = 0, LR = 1)", backend);
    const MetoCounts c = backend == ER_METO_LR ? meto_decode_lr(tokens, n, bins, v, f, t) : meto_decode_lr_absco(tokens, n, bins, v, f, t);
    *nv = c.vertices; *nf = c.faces; *nt = c.face_types;
    return ER_OK;
}

extern "C" int er_meto_encode(const float* vertices, int nv, const int32_t* faces, int nf, int bins, int backend, int32_t* tokens,
                              int32_t* n_tokens, int32_t* face_order, int32_t* face_type, int32_t* n_faces_out) {
    if (backend != ER_METO_LR_ABSCO && backend != ER_METO_LR) return fail(ER_ERR_UNSUPPORTED, "meto backend %d (LR_ABSCO = 0, LR = 1)", backend);
    if (nv < 0 || nf < 0 || bins <= 0 || !tokens || !n_tokens || !face_order || !face_type || !n_faces_out ||
        (nv > 0 && !vertices) || (nf > 0 && !faces))
        return fail(ER_ERR_INVALID, "er_meto_encode: bad argument");
    for (int i = 0; i < 3 * nf; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return fail(ER_ERR_INVALID, "er_meto_encode: face index %d out of range", faces[i]);
    const MetoEncodeOut o = backend == ER_METO_LR ? meto_encode<true>(vertices, nv, faces, nf, bins) : meto_encode<false>(vertices, nv, faces, nf, bins);
    const long long per = backend == ER_METO_LR ? 2 : 1;      // LR may open a sub-mesh on an already covered face (see meto_encode.h)
    if ((long long)o.tokens.size() > 10LL * per * nf || (long long)o.face_order.size() > per * nf)
        return fail(ER_ERR_CAPACITY, "er_meto_encode: token bound exceeded");
    memcpy(tokens, o.tokens.data(), o.tokens.size() * sizeof(int32_t));
    memcpy(face_order, o.face_order.data(), o.face_order.size() * sizeof(int32_t));
    memcpy(face_type, o.face_type.data(), o.face_type.size() * sizeof(int32_t));
    *n_tokens = (int32_t)o.tokens.size();
    *n_faces_out = (int32_t)o.face_order.size();
    return ER_OK;
}

// ------------------------------------------------------------------------------------ DiT front-end (f3)
#include "er_dit.h"
