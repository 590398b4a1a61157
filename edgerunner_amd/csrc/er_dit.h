// DiT image-conditioned front-end behind the C ABI (er_dit_*): included at the end of er_api.hip so it can reuse the prefill
// building blocks (the GEMM launchers, attention_full, DevBuf, pick, fail, HIPCHK/HIPRET/ERCHK), the weight table and loader
// (er_weights.h) and the point encoder helpers.
// Reference: core/transformer/dit.py (DiT, DiTLayer, TimestepEmbedding) and core/models_dit.py::MDiT.run.
#pragma once
#include "k_dit.h"
#include "k_dit_loss.h"

struct DitLayerW {
    float *sst = nullptr;                                   // scale_shift_table [6][C]
    float *qkv_w = nullptr, *qkv_b = nullptr, *o_w = nullptr, *o_b = nullptr;                     // attn1 (self)
    float *q2_w = nullptr, *q2_b = nullptr, *k2_w = nullptr, *k2_b = nullptr, *v2_w = nullptr, *v2_b = nullptr,
          *o2_w = nullptr, *o2_b = nullptr;                                                      // attn2 (cross)
    float *ff0_w = nullptr, *ff0_b = nullptr, *ff2_w = nullptr, *ff2_b = nullptr;
    // fp16 mode: ff0 with its rows permuted so that the GEMM epilogue sees value and gate of an output in one wave (k_gemm.h,
    // HEPI_GEGLU); built on first use from the fp16 copy of ff0_w
    _Float16* ff0_p16 = nullptr;
    float* ff0_bp = nullptr;
};

struct ClipLayerW {
    float *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr;
    float *qw = nullptr, *qb = nullptr, *kw = nullptr, *kb = nullptr, *vw = nullptr, *vb = nullptr, *ow = nullptr, *ob = nullptr;
    float *f1w = nullptr, *f1b = nullptr, *f2w = nullptr, *f2b = nullptr;
};

struct er_dit_ctx {
    er_dit_config cfg{};
    int device = 0;
    hipStream_t own_stream = nullptr;
    std::vector<DitLayerW> layers;
    float *pos_embed = nullptr, *sst2 = nullptr, *proj_in_w = nullptr, *proj_in_b = nullptr, *tp1_w = nullptr, *tp1_b = nullptr,
          *tp2_w = nullptr, *tp2_b = nullptr, *adaln_w = nullptr, *adaln_b = nullptr, *proj_out_w = nullptr,
          *proj_out_b = nullptr, *projc_w = nullptr, *projc_b = nullptr, *normc_w = nullptr, *normc_b = nullptr;
    std::vector<ClipLayerW> clip;
    float *clip_cls = nullptr, *clip_patch_w = nullptr, *clip_pos = nullptr, *clip_prew = nullptr, *clip_preb = nullptr;
    int clip_kpad = 0;
    DevBuf<float> cpx, ccol, cpatch, cx, ch, cq, ck, cv, catt, cf;   // image encoder scratch
    WeightTable w;                                       // every checkpoint key (dit_weights); w.half_of: the fp16 copies of fast mode
    bool fast = false;                                   // fp16-input MFMA for every Linear (weights stored fp16 too)
    // scratch: grow-only, freed with the context
    DevBuf<float> x, qkv, att, q2, kv2, u, g, sc, tin, temb0, temb1, temb, tsil, tada, t_dev, xin, pred, czero, ctmp;
    // fp16 mode: fp16 copies of the activations that feed a Linear, written by their producers (k_gemm.h, gemm_hh_mfma_kernel)
    DevBuf<_Float16> x16, att16, g16;
    // ... and q / k / v in fp16 with V transposed, for the LDS-DMA attention (k_flash_attn.h, flash_attn_hh_kernel)
    DevBuf<_Float16> qkv16, vt16, q2_16, k2_16, v2tmp16, v2t16;
    DevBuf<float> gates;                   // [layer][2][B][C]: gate_msa / gate_mlp rows of every layer (one launch per forward)
    DevBuf<const float*> sst_ptrs;         // the layers' scale_shift_table pointers
    int kv2_mp = 0;                        // padded key count of the cross-attention V^T rows
    bool geglu_perm_valid = false;
    int pred_type = ER_PRED_V_PREDICTION;  // what the DiT predicts (er_dit_set_prediction_type): the sampler's DDIM update and the loss target
    // the reference's frozen point encoder (MDiT.point_encoder, core/models_dit.py:68-75), after er_dit_attach_point_encoder only
    bool has_pe = false;
    PointEnc pe;                           // its point_encoder.* keys join `w` when it is attached
    DevBuf<float> lcoef;                   // er_dit_loss: [sa | sb | w] per sample
    DevBuf<double> lpart;                  // ... and its partial sums
};

// every checkpoint key of the DiT (+ CLIP) context; fp16 mode keeps an fp16 copy of the Linear and patch-conv weights (GEMM operands)
static void dit_weights(er_dit_ctx* c) {
    WeightTable& t = c->w;
    const er_dit_config& g = c->cfg;
    const size_t C = g.hidden_dim;
    t.fp16 = c->fast;
    auto lin = [&](const std::string& k, float** w, float** b, size_t out, size_t in) { t.lin(k, w, b, out, in).half(); };
    auto norm = [&](const std::string& k, float** w, float** b, size_t n) { t.lin(k, w, b, n, 1); };
    t.add("dit.pos_embed", &c->pos_embed, (size_t)g.latent_size * C);
    t.add("dit.scale_shift_table", &c->sst2, 2 * C);
    lin("dit.proj_in", &c->proj_in_w, &c->proj_in_b, C, g.latent_dim);
    lin("dit.timestep_proj.linear_1", &c->tp1_w, &c->tp1_b, C, 256);
    lin("dit.timestep_proj.linear_2", &c->tp2_w, &c->tp2_b, C, C);
    lin("dit.adaln_linear", &c->adaln_w, &c->adaln_b, 6 * C, C);
    lin("dit.proj_out", &c->proj_out_w, &c->proj_out_b, g.latent_dim, C);
    lin("proj_cond", &c->projc_w, &c->projc_b, C, g.clip_dim);
    norm("norm_cond", &c->normc_w, &c->normc_b, C);
    if (g.clip_layers > 0) {
        const std::string p = "image_encoder.vision_model";
        const size_t W = g.clip_dim, P = g.clip_patch, NT = (size_t)(g.clip_image_size / g.clip_patch) * (g.clip_image_size / g.clip_patch) + 1;
        c->clip_kpad = (int)((3 * P * P + 31) / 32 * 32);
        t.add(p + ".embeddings.class_embedding", &c->clip_cls, W);
        t.add(p + ".embeddings.patch_embedding.weight", &c->clip_patch_w, W * 3 * P * P).pad(3 * P * P, c->clip_kpad).half();
        t.add(p + ".embeddings.position_embedding.weight", &c->clip_pos, NT * W);
        norm(p + ".pre_layrnorm", &c->clip_prew, &c->clip_preb, W);
        for (int i = 0; i < g.clip_layers; ++i) {
            ClipLayerW& L = c->clip[i];
            const std::string q = p + ".encoder.layers." + std::to_string(i);
            lin(q + ".self_attn.q_proj", &L.qw, &L.qb, W, W);
            lin(q + ".self_attn.k_proj", &L.kw, &L.kb, W, W);
            lin(q + ".self_attn.v_proj", &L.vw, &L.vb, W, W);
            lin(q + ".self_attn.out_proj", &L.ow, &L.ob, W, W);
            norm(q + ".layer_norm1", &L.ln1w, &L.ln1b, W);
            norm(q + ".layer_norm2", &L.ln2w, &L.ln2b, W);
            lin(q + ".mlp.fc1", &L.f1w, &L.f1b, g.clip_mlp_dim, W);
            lin(q + ".mlp.fc2", &L.f2w, &L.f2b, W, g.clip_mlp_dim);
        }
    }
    for (int i = 0; i < g.num_layers; ++i) {
        DitLayerW& L = c->layers[i];
        const std::string p = "dit.layers." + std::to_string(i);
        t.add(p + ".scale_shift_table", &L.sst, 6 * C);
        lin(p + ".attn1.qkv_proj", &L.qkv_w, &L.qkv_b, 3 * C, C);
        lin(p + ".attn1.out_proj", &L.o_w, &L.o_b, C, C);
        lin(p + ".attn2.q_proj", &L.q2_w, &L.q2_b, C, C);
        lin(p + ".attn2.k_proj", &L.k2_w, &L.k2_b, C, C);
        lin(p + ".attn2.v_proj", &L.v2_w, &L.v2_b, C, C);
        lin(p + ".attn2.out_proj", &L.o2_w, &L.o2_b, C, C);
        lin(p + ".ff.net.0", &L.ff0_w, &L.ff0_b, 8 * C, C);
        lin(p + ".ff.net.2", &L.ff2_w, &L.ff2_b, C, 4 * C);
    }
}

extern "C" int er_dit_create(const er_dit_config* cfg, int device, er_dit_ctx** out) {
    if (!cfg || !out) return fail(ER_ERR_INVALID, "er_dit_create: null argument");
    if (cfg->hidden_dim != 1024 || cfg->hidden_dim % cfg->num_heads || (cfg->hidden_dim / cfg->num_heads) % 16)
        return fail(ER_ERR_UNSUPPORTED, "DiT width %d / heads %d not built (1024, head_dim multiple of 16)", cfg->hidden_dim, cfg->num_heads);
    if (cfg->latent_dim % 16 || cfg->clip_dim % 16) return fail(ER_ERR_UNSUPPORTED, "latent_dim / clip_dim must be multiples of 16");
    HIPCHK(hipSetDevice(device));
    er_dit_ctx* c = new er_dit_ctx();
    c->cfg = *cfg;
    c->device = device;
    c->layers.resize(cfg->num_layers);
    if (cfg->weight_dtype != ER_F32 && cfg->weight_dtype != ER_F16) return fail(ER_ERR_UNSUPPORTED, "DiT weight_dtype must be fp32 or fp16");
    c->fast = cfg->weight_dtype == ER_F16;
    if (cfg->clip_layers > 0) {
        if (cfg->clip_dim != 1280 || cfg->clip_heads <= 0 || cfg->clip_dim % cfg->clip_heads || (cfg->clip_dim / cfg->clip_heads) % 16 ||
            cfg->clip_mlp_dim % 16 || cfg->clip_patch <= 0 || cfg->clip_image_size % cfg->clip_patch)
            return fail(ER_ERR_UNSUPPORTED, "CLIP encoder shape not built (width 1280, head_dim and mlp multiples of 16)");
        c->clip.resize(cfg->clip_layers);
    }
    HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault));
    dit_weights(c);
    *out = c;
    return ER_OK;
}

// the buffers and weight blocks are members: deleting the context frees them, once the device is idle
extern "C" int er_dit_destroy(er_dit_ctx* c) {
    if (!c) return ER_OK;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
    return ER_OK;
}

extern "C" int er_dit_load_tensor(er_dit_ctx* c, const char* key, const void* data, int dtype, int ndim, const int64_t* shape,
                                  int on_device) {
    if (!c || !key) return fail(ER_ERR_INVALID, "er_dit_load_tensor: bad argument");
    HIPCHK(hipSetDevice(c->device));
    std::string k(key);
    if (k.rfind("image_encoder.", 0) == 0 && k.find("image_encoder.vision_model.") != 0)
        k = "image_encoder.vision_model." + k.substr(strlen("image_encoder."));      // transformers >= 5 drops the prefix
    const int rc = weights_load(c->w, c->own_stream, "er_dit_load_tensor", k, data, dtype, ndim, shape, on_device);
    if (rc != 1) c->geglu_perm_valid = false;          // any reload invalidates the permuted feed-forward operands
    return rc;
}

extern "C" int er_dit_finalize_weights(er_dit_ctx* c) {
    if (!c) return fail(ER_ERR_INVALID, "null ctx");
    return weights_finalize(c->w);
}

extern "C" int er_dit_attach_point_encoder(er_dit_ctx* c, int point_hidden_dim, int point_num_heads, int point_freq_dim) {
    if (!c) return fail(ER_ERR_INVALID, "null ctx");
    if (c->has_pe) return fail(ER_ERR_INVALID, "er_dit_attach_point_encoder: a point encoder is already attached");
    if (point_hidden_dim != 1024 || point_num_heads <= 0 || point_hidden_dim % point_num_heads)   // as er_create (cond_mode POINT)
        return fail(ER_ERR_UNSUPPORTED, "point encoder width %d / heads %d not built (1024)", point_hidden_dim, point_num_heads);
    if (point_freq_dim <= 0 || point_freq_dim % 3) return fail(ER_ERR_INVALID, "point_freq_dim %d must be a positive multiple of 3", point_freq_dim);
    PointEnc& p = c->pe;
    p.PH = point_hidden_dim; p.heads = point_num_heads; p.freq = point_freq_dim;
    p.Lq = c->cfg.latent_size; p.LD = c->cfg.latent_dim; p.eps = 1e-5f;
    ERCHK(pe_attach(c->w, p, ER_PE_EMBED, "er_dit_attach_point_encoder", "point_encoder."));
    c->has_pe = true;
    return ER_OK;
}

extern "C" int er_dit_point_latent(er_dit_ctx* c, const float* points, int B, int n_points, float* latent_out, void* stream) {
    if (!c || !points || !latent_out || B <= 0 || n_points <= 0) return fail(ER_ERR_INVALID, "er_dit_point_latent: bad argument");
    if (!c->has_pe) return fail(ER_ERR_UNSUPPORTED, "er_dit_point_latent: no point encoder attached (er_dit_attach_point_encoder)");
    ERCHK(er_dit_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    return pe_latent(c->pe, points, B, n_points, latent_out, pick(c, stream), "er_dit_point_latent");
}

extern "C" int er_dit_set_point_encoder_mode(er_dit_ctx* c, int mode) {
    if (!c) return fail(ER_ERR_INVALID, "null ctx");
    if (!c->has_pe) return fail(ER_ERR_UNSUPPORTED, "er_dit_set_point_encoder_mode: no point encoder attached (er_dit_attach_point_encoder)");
    return pe_attach(c->w, c->pe, mode, "er_dit_set_point_encoder_mode", "point_encoder.");
}

extern "C" int er_dit_set_prediction_type(er_dit_ctx* c, int pred_type) {
    if (!c) return fail(ER_ERR_INVALID, "null ctx");
    if (pred_type != ER_PRED_V_PREDICTION && pred_type != ER_PRED_EPSILON)
        return fail(ER_ERR_INVALID, "er_dit_set_prediction_type: %d is neither ER_PRED_V_PREDICTION nor ER_PRED_EPSILON", pred_type);
    c->pred_type = pred_type;
    return ER_OK;
}

constexpr int DIT_TRAIN_STEPS = 1000;     // num_train_timesteps of both schedulers (core/models_dit.py:80-101)

// alphas_cumprod of the reference's DDPMScheduler / DDIMScheduler (scaled_linear betas 0.00085..0.012): the sampler's DDIM update and
// the loss coefficients read this one table.  torch.linspace(sqrt(b0), sqrt(b1), T, fp32) ** 2 -> cumprod(1 - betas), all in fp32
// like diffusers.
static std::vector<float> dit_alphas_cumprod() {
    const int T = DIT_TRAIN_STEPS;
    std::vector<float> ac(T);
    const float lo = (float)sqrt(0.00085), hi = (float)sqrt(0.012);
    const float step = (hi - lo) / (float)(T - 1);
    float prod = 1.0f;
    for (int i = 0; i < T; ++i) {
        const float r = (i < T / 2) ? lo + step * (float)i : hi - step * (float)(T - 1 - i);   // linspace is symmetric
        const float beta = r * r;
        prod *= (1.0f - beta);
        ac[i] = prod;
    }
    return ac;
}

// Per-sample loss coefficients in fp32, as diffusers computes them (add_noise / get_velocity / compute_snr) and models_dit.py:165-177
// weighs them: coef = [sa[B] | sb[B] | w[B]] with sa = sqrt(ac[t]), sb = sqrt(1 - ac[t]), snr = (sa / sb)^2 and
// w = min(snr, gamma) / (snr + 1) (v-prediction) or / snr (epsilon); w = 1 when gamma is None (<= 0 or NaN).
static int dit_loss_coefs(const int32_t* t, int B, int pred_type, float gamma, std::vector<float>& coef) {
    const std::vector<float> ac = dit_alphas_cumprod();
    coef.assign((size_t)3 * B, 0.f);
    const bool weighted = gamma > 0.f;        // false for NaN too
    for (int b = 0; b < B; ++b) {
        if (t[b] < 0 || t[b] >= DIT_TRAIN_STEPS)
            return fail(ER_ERR_INVALID, "timestep %d of sample %d is outside [0, %d)", t[b], b, DIT_TRAIN_STEPS);
        const float a = ac[t[b]], sa = sqrtf(a), sb = sqrtf(1.0f - a);
        float w = 1.0f;
        if (weighted) {
            const float r = sa / sb, snr = r * r, m = fminf(snr, gamma);
            w = pred_type == ER_PRED_EPSILON ? m / snr : m / (snr + 1.0f);
        }
        coef[b] = sa;
        coef[B + b] = sb;
        coef[2 * B + b] = w;
    }
    return 0;
}

// Linear layer: fp32 MFMA, or (fast mode) fp16-input MFMA with the activation rounded to fp16 on the way in
static hipError_t dlin(er_dit_ctx* c, const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N,
                       int K, const float* resid, int ldr, const float* gate, int gate_rows, hipStream_t st) {
    GemmArgs g = gemm_args_linear(A, lda, W, bias, C, ldc, M, N, K, false, resid, ldr);
    g.gate = gate; g.gate_rows = gate_rows; g.gate_bstride = N;
    if (c->fast && K % 32 == 0) {
        auto it = c->w.half_of.find(W);
        if (it != c->w.half_of.end()) {
            g.B = reinterpret_cast<const float*>(it->second);
            return launch_gemm_f16(g, st);
        }
    }
    return launch_gemm(g, 1, st);
}

extern "C" int er_dit_project_cond(er_dit_ctx* c, const float* clip_hidden, int B, int M, float* cond_out, void* stream) {
    if (!c || !clip_hidden || !cond_out || B <= 0 || M <= 0) return fail(ER_ERR_INVALID, "er_dit_project_cond: bad argument");
    ERCHK(er_dit_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const int C = c->cfg.hidden_dim;
    ERCHK(c->ctmp.ensure((size_t)B * M * C));
    HIPRET(dlin(c, clip_hidden, c->cfg.clip_dim, c->projc_w, c->projc_b, c->ctmp.p, C, B * M, C, c->cfg.clip_dim, nullptr, 0, nullptr, 1, st));
    HIPRET(launch_layernorm(c->ctmp.p, c->normc_w, c->normc_b, cond_out, B * M, C, C, C, 1e-5f, st));
    return ER_OK;
}

extern "C" int er_dit_encode_image(er_dit_ctx* c, const float* images, int B, int Himg, int Wimg, float* out, void* stream) {
    if (!c || !images || !out || B <= 0 || Himg <= 0 || Wimg <= 0) return fail(ER_ERR_INVALID, "er_dit_encode_image: bad argument");
    if (c->cfg.clip_layers <= 0) return fail(ER_ERR_UNSUPPORTED, "this context was created without the image encoder (clip_layers = 0)");
    ERCHK(er_dit_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const er_dit_config& g = c->cfg;
    const int W = g.clip_dim, S = g.clip_image_size, P = g.clip_patch, G = S / P, NP = G * G, NT = NP + 1, H = g.clip_heads,
              D = W / H, F = g.clip_mlp_dim, R = B * NT, ldS = (NT + 15) / 16 * 16;
    ERCHK(c->cpx.ensure((size_t)B * 3 * S * S));
    ERCHK(c->ccol.ensure((size_t)B * NP * c->clip_kpad));
    ERCHK(c->cpatch.ensure((size_t)B * NP * W));
    ERCHK(c->cx.ensure((size_t)R * W));
    ERCHK(c->ch.ensure((size_t)R * W));
    ERCHK(c->cq.ensure((size_t)R * W));
    ERCHK(c->ck.ensure((size_t)R * W));
    ERCHK(c->cv.ensure((size_t)R * W));
    ERCHK(c->catt.ensure((size_t)R * W));
    ERCHK(c->cf.ensure((size_t)R * F));
    ERCHK(c->sc.ensure((size_t)H * NT * ldS));
    HIPRET(launch_clip_preprocess(images, c->cpx.p, B, Himg, Wimg, S, st));
    HIPRET(launch_clip_im2col(c->cpx.p, c->ccol.p, B, S, P, c->clip_kpad, st));
    HIPRET(dlin(c, c->ccol.p, c->clip_kpad, c->clip_patch_w, nullptr, c->cpatch.p, W, B * NP, W, c->clip_kpad, nullptr, 0, nullptr, 1, st));
    float* x = c->cx.p;
    HIPRET(launch_clip_assemble(c->cpatch.p, c->clip_cls, c->clip_pos, x, B, NP, W, st));
    HIPRET(launch_layernorm(x, c->clip_prew, c->clip_preb, x, R, W, W, W, 1e-5f, st));
    for (int l = 0; l < g.clip_layers; ++l) {           // CLIPEncoderLayer: pre-LN attention + pre-LN MLP, both residual
        const ClipLayerW& L = c->clip[l];
        HIPRET(launch_layernorm(x, L.ln1w, L.ln1b, c->ch.p, R, W, W, W, 1e-5f, st));
        HIPRET(dlin(c, c->ch.p, W, L.qw, L.qb, c->cq.p, W, R, W, W, nullptr, 0, nullptr, 1, st));
        HIPRET(dlin(c, c->ch.p, W, L.kw, L.kb, c->ck.p, W, R, W, W, nullptr, 0, nullptr, 1, st));
        HIPRET(dlin(c, c->ch.p, W, L.vw, L.vb, c->cv.p, W, R, W, W, nullptr, 0, nullptr, 1, st));
        for (int b = 0; b < B; ++b) {
            const size_t o = (size_t)b * NT * W;
            ERCHK(attention_full(c->cq.p + o, W, c->ck.p + o, W, D, c->cv.p + o, W, D, c->catt.p + o, W, c->sc.p, H, D, NT, NT, false, st));
        }
        HIPRET(dlin(c, c->catt.p, W, L.ow, L.ob, x, W, R, W, W, x, W, nullptr, 1, st));
        HIPRET(launch_layernorm(x, L.ln2w, L.ln2b, c->ch.p, R, W, W, W, 1e-5f, st));
        HIPRET(dlin(c, c->ch.p, W, L.f1w, L.f1b, c->cf.p, F, R, F, W, nullptr, 0, nullptr, 1, st));
        HIPRET(launch_gelu(c->cf.p, c->cf.p, (long long)R * F, st));
        HIPRET(dlin(c, c->cf.p, F, L.f2w, L.f2b, x, W, R, W, F, x, W, nullptr, 1, st));
    }
    HIPCHK(hipMemcpyAsync(out, x, (size_t)R * W * 4, hipMemcpyDeviceToDevice, st));
    return ER_OK;
}

// fp16 mode: permuted ff0 operands of every layer (once per set of weights)
static int dit_build_geglu_perm(er_dit_ctx* c, hipStream_t st) {
    if (c->geglu_perm_valid) return 0;
    const int C = c->cfg.hidden_dim, F = 4 * C;
    for (auto& L : c->layers) {
        auto it = c->w.half_of.find(L.ff0_w);
        if (it == c->w.half_of.end()) return fail(ER_ERR_INVALID, "dit: no fp16 copy of ff.net.0.proj");
        if (!L.ff0_p16) {
            ERCHK(c->w.alloc(&L.ff0_p16, (size_t)2 * F * C));
            ERCHK(c->w.alloc(&L.ff0_bp, (size_t)2 * F));
        }
        hipLaunchKernelGGL(geglu_permute_kernel, dim3(2 * F), dim3(ER_WG), 0, st, it->second, L.ff0_b, L.ff0_p16, L.ff0_bp, F, C);
        HIPRET(hipGetLastError());
    }
    c->geglu_perm_valid = true;
    return 0;
}

// fp16 mode, A already in fp16 (written by its producer): both operands by LDS-DMA.  c16: optional fp16 copy of the output.
// vt16 / vt_rows: the V third of a fused q/k/v projection leaves as V^T per head (GemmArgs::vt16), vt_rows tokens per batch entry.
static hipError_t dlin16(er_dit_ctx* c, const _Float16* A16, int lda, const float* W, const float* bias, float* C, int ldc, int M,
                         int N, int K, const float* resid, int ldr, const float* gate, int gate_rows, _Float16* c16, hipStream_t st,
                         _Float16* vt16 = nullptr, int vt_rows = 0) {
    GemmArgs g = gemm_args_linear(A16, lda, nullptr, bias, C, ldc, M, N, K, false, resid, ldr);      // (B: the fp16 copy of W, below)
    g.gate = gate; g.gate_rows = gate_rows; g.gate_bstride = N;
    g.c16 = c16; g.ldc16 = N;
    if (vt16) { g.vt16 = vt16; g.vt_col0 = 2 * (N / 3); g.vt_rows = vt_rows; g.vt_ld = vt_rows; }
    auto it = c->w.half_of.find(W);
    if (it == c->w.half_of.end()) return hipErrorInvalidValue;
    g.B = reinterpret_cast<const float*>(it->second);
    return launch_gemm_hh(g, st);
}

// t_emb / t_adaln for B rows with timesteps already on the device (t_dev [B])
static int dit_time_embed(er_dit_ctx* c, int B, hipStream_t st) {
    const int C = c->cfg.hidden_dim;
    ERCHK(c->tin.ensure((size_t)B * 256));
    ERCHK(c->temb0.ensure((size_t)B * C));
    ERCHK(c->temb1.ensure((size_t)B * C));
    ERCHK(c->temb.ensure((size_t)B * C));
    ERCHK(c->tsil.ensure((size_t)B * C));
    ERCHK(c->tada.ensure((size_t)B * 6 * C));
    HIPRET(launch_timestep_embed(c->t_dev.p, c->tin.p, B, 128, st));
    HIPRET(dlin(c, c->tin.p, 256, c->tp1_w, c->tp1_b, c->temb0.p, C, B, C, 256, nullptr, 0, nullptr, 1, st));
    HIPRET(launch_silu(c->temb0.p, c->temb1.p, (long long)B * C, st));
    HIPRET(dlin(c, c->temb1.p, C, c->tp2_w, c->tp2_b, c->temb.p, C, B, C, C, nullptr, 0, nullptr, 1, st));
    HIPRET(launch_silu(c->temb.p, c->tsil.p, (long long)B * C, st));
    HIPRET(dlin(c, c->tsil.p, C, c->adaln_w, c->adaln_b, c->tada.p, 6 * C, B, 6 * C, C, nullptr, 0, nullptr, 1, st));
    return 0;
}

// cross-attention keys/values of every layer for a fixed condition (they do not depend on x or t):
// kv2 layout [layer][2][B*M][C]
static int dit_cross_kv(er_dit_ctx* c, const float* cond, int B, int M, hipStream_t st) {
    const int C = c->cfg.hidden_dim, nl = c->cfg.num_layers;
    ERCHK(c->kv2.ensure((size_t)nl * 2 * B * M * C));
    for (int l = 0; l < nl; ++l) {
        const DitLayerW& L = c->layers[l];
        float* k2 = c->kv2.p + ((size_t)l * 2) * B * M * C;
        float* v2 = k2 + (size_t)B * M * C;
        HIPRET(dlin(c, cond, C, L.k2_w, L.k2_b, k2, C, B * M, C, C, nullptr, 0, nullptr, 1, st));
        HIPRET(dlin(c, cond, C, L.v2_w, L.v2_b, v2, C, B * M, C, C, nullptr, 0, nullptr, 1, st));
    }
    if (c->fast && C / c->cfg.num_heads == FA_D) {      // fp16 K and V^T (zero-padded to a multiple of 64 keys) for flash_attn_hh_kernel
        const int H = c->cfg.num_heads, Mp = (M + 63) / 64 * 64;
        c->kv2_mp = Mp;
        ERCHK(c->k2_16.ensure((size_t)nl * B * M * C + F16_TAIL));
        ERCHK(c->v2tmp16.ensure((size_t)B * M * C + F16_TAIL));
        ERCHK(c->v2t16.ensure((size_t)nl * B * H * 64 * Mp + F16_TAIL));
        for (int l = 0; l < nl; ++l) {
            const float* k2 = c->kv2.p + ((size_t)l * 2) * B * M * C;
            const float* v2 = k2 + (size_t)B * M * C;
            _Float16* k16 = c->k2_16.p + (size_t)l * B * M * C;
            _Float16* vtmp = c->v2tmp16.p;
            _Float16* vt = c->v2t16.p + (size_t)l * B * H * 64 * Mp;
            hipLaunchKernelGGL(cvt_rows_f16_kernel, dim3(ew_grid((long long)B * M * C)), dim3(ER_WG), 0, st, k2, k16, (long long)B * M, C, C, C);
            hipLaunchKernelGGL(cvt_rows_f16_kernel, dim3(ew_grid((long long)B * M * C)), dim3(ER_WG), 0, st, v2, vtmp, (long long)B * M, C, C, C);
            hipLaunchKernelGGL(transpose_v_f16_kernel, dim3(Mp / 64, H, B), dim3(ER_WG), 0, st, vtmp, vt, M, Mp, C, (long long)M * C);
            HIPRET(hipGetLastError());
        }
    }
    return 0;
}

// Fused-attention arguments of a DiT layer: N latent queries per sample over M keys, H heads of D side by side in rows of C; q, k (and v)
// rows ldqkv apart (3 C inside the self-attention's fused qkv rows, C for the cross-attention's separate buffers), the output in rows of C.
// LDS-DMA form: fp16 operands, V^T per head in rows of Mp keys (M padded to a multiple of 64)
static FlashHArgs dit_flash_hh_args(const _Float16* q, const _Float16* k, const _Float16* vt, _Float16* o16, int N, int M, int Mp, int ldqkv,
                                    int C, int H, int D) {
    FlashHArgs fh{};
    fh.Q = q; fh.K = k; fh.Vt = vt; fh.O16 = o16; fh.N = N; fh.M = M;
    fh.ldq = fh.ldk = ldqkv; fh.ldvt = Mp; fh.ldo = C;
    fh.qs_b = (long long)N * ldqkv; fh.ks_b = (long long)M * ldqkv; fh.vts_h = 64LL * Mp; fh.vts_b = (long long)H * 64 * Mp; fh.os_b = (long long)N * C;
    fh.head_stride = D; fh.scale = 1.0f / sqrtf((float)D);
    return fh;
}
// register-staged form: fp32 operands; the output goes to o16 INSTEAD of o when o16 is not null
static FlashArgs dit_flash_args(const float* q, const float* k, const float* v, float* o, _Float16* o16, int N, int M, int ldqkv, int C, int D) {
    FlashArgs fa{};
    fa.Q = q; fa.K = k; fa.V = v; fa.O = o; fa.N = N; fa.M = M;
    fa.ldq = fa.ldk = fa.ldv = ldqkv; fa.ldo = C;
    fa.qs_b = (long long)N * ldqkv; fa.ks_b = fa.vs_b = (long long)M * ldqkv; fa.os_b = (long long)N * C;
    fa.head_stride = D; fa.scale = 1.0f / sqrtf((float)D);
    fa.O16 = o16;
    return fa;
}

// DiT.forward body for B rows; their time embeddings temb [B][C] / tada [B][6 C] (dit_time_embed), cross K/V in c->kv2 (dit_cross_kv)
static int dit_forward_impl(er_dit_ctx* c, const float* xin, int B, int M, float* out, const float* temb, const float* tada, hipStream_t st) {
    const er_dit_config& g = c->cfg;
    const int C = g.hidden_dim, N = g.latent_size, H = g.num_heads, D = C / H, LD = g.latent_dim;
    const int R = B * N;
    const int ldS = (N + 15) / 16 * 16;
    ERCHK(c->x.ensure((size_t)R * C));
    ERCHK(c->qkv.ensure((size_t)R * 3 * C));
    ERCHK(c->att.ensure((size_t)R * C));
    ERCHK(c->q2.ensure((size_t)R * C));
    ERCHK(c->u.ensure((size_t)R * 8 * C));
    ERCHK(c->g.ensure((size_t)R * 4 * C));
    // fp16 mode: fused attention on the fp16 matrix cores (no score matrix in HBM); ER_DIT_NO_FLASH=1 keeps the
    // materialised fp32 scores path for A/B measurements
    static const bool no_flash = getenv("ER_DIT_NO_FLASH") != nullptr;
    const bool flash = c->fast && D == FA_D && !no_flash;
    if (!flash) ERCHK(c->sc.ensure((size_t)H * N * ldS));
    ERCHK(c->gates.ensure((size_t)g.num_layers * 2 * B * C));
    if (!c->sst_ptrs.p) {
        std::vector<const float*> hp;
        for (auto& L : c->layers) hp.push_back(L.sst);
        DevBuf<const float*> d;
        ERCHK(d.ensure(hp.size()));
        HIPCHK(hipMemcpy(d.p, hp.data(), hp.size() * sizeof(float*), hipMemcpyHostToDevice));
        c->sst_ptrs = std::move(d);        // only a filled table is kept
    }
    // fp16 activations for the LDS-DMA GEMM (all K of this path are multiples of 64 except none: C = 1024, 4C = 4096)
    // ... and the LDS-DMA attention wants whole 64-row tiles of latent tokens and cross K / V^T prepared (zero-padded) for THIS
    // condition length; any other shape keeps the fp32-operand fused attention + register-staged GEMMs below (x16 / att16 null)
    const bool hh = flash && C % 64 == 0 && N % 64 == 0 && c->kv2_mp == (M + 63) / 64 * 64;
    if (hh) {
        ERCHK(c->x16.ensure((size_t)R * C + F16_TAIL));
        ERCHK(c->att16.ensure((size_t)R * C + F16_TAIL));
        ERCHK(c->g16.ensure((size_t)R * 4 * C + F16_TAIL));
    }
    _Float16* x16 = hh ? c->x16.p : nullptr;
    _Float16* att16 = hh ? c->att16.p : nullptr;
    _Float16* g16 = hh ? c->g16.p : nullptr;
    if (hh) ERCHK(dit_build_geglu_perm(c, st));
    if (hh) {
        ERCHK(c->qkv16.ensure((size_t)R * 3 * C + F16_TAIL));
        ERCHK(c->vt16.ensure((size_t)R * C + F16_TAIL));
        ERCHK(c->q2_16.ensure((size_t)R * C + F16_TAIL));
    }
    _Float16* qkv16 = hh ? c->qkv16.p : nullptr;
    _Float16* vt16 = hh ? c->vt16.p : nullptr;
    _Float16* q2_16 = hh ? c->q2_16.p : nullptr;
    HIPRET(launch_adaln_gate_all(c->sst_ptrs.p, tada, c->gates.p, g.num_layers, B, C, st));
    float* x = c->x.p;
    // x = proj_in(x) + pos_embed                                                  dit.py:177-180
    HIPRET(dlin(c, xin, LD, c->proj_in_w, c->proj_in_b, x, C, R, C, LD, nullptr, 0, nullptr, 1, st));
    HIPRET(launch_add_pos(x, c->pos_embed, x, B, N, C, 0, st));
    for (int l = 0; l < g.num_layers; ++l) {
        const DitLayerW& L = c->layers[l];
        // x = norm1(x) * (1 + scale_msa) + shift_msa   (chunks 0 = shift, 1 = scale, 2 = gate)     dit.py:129-132
        HIPRET(dit_ln_mod(x, x, R, N, L.sst, tada, 6LL * C, C, 0, 1, st, x16));
        // x = x + gate_msa * attn1(x)                                               dit.py:133
        if (hh) {     // q, k leave the GEMM in fp16 only and V as V^T per head (its epilogue); K and V^T tiles then reach LDS by DMA
            HIPRET(dlin16(c, x16, C, L.qkv_w, L.qkv_b, nullptr, 3 * C, R, 3 * C, C, nullptr, 0, nullptr, 1, qkv16, st, vt16, N));
            HIPRET(launch_flash_attn_hh(dit_flash_hh_args(qkv16, qkv16 + C, vt16, att16, N, N, N, 3 * C, C, H, D), H, B, st));
        } else {
        HIPRET(dlin(c, x, C, L.qkv_w, L.qkv_b, c->qkv.p, 3 * C, R, 3 * C, C, nullptr, 0, nullptr, 1, st));
        if (flash) {
            const float* qkv = c->qkv.p;
            HIPRET(launch_flash_attn_f16(dit_flash_args(qkv, qkv + C, qkv + 2 * C, c->att.p, att16, N, N, 3 * C, C, D), H, B, st));
        } else {
            for (int b = 0; b < B; ++b) {
                float* base = c->qkv.p + (size_t)b * N * 3 * C;
                ERCHK(attention_full(base, 3 * C, base + C, 3 * C, D, base + 2 * C, 3 * C, D, c->att.p + (size_t)b * N * C, C,
                                     c->sc.p, H, D, N, N, false, st));
            }
        }
        }
        const float* gate_msa = c->gates.p + ((size_t)l * 2) * B * C;
        const float* gate_mlp = gate_msa + (size_t)B * C;
        // (the fp16 copy of the new x is the A operand of the cross-attention query projection)
        if (hh) HIPRET(dlin16(c, att16, C, L.o_w, L.o_b, x, C, R, C, C, x, C, gate_msa, N, x16, st));
        else HIPRET(dlin(c, c->att.p, C, L.o_w, L.o_b, x, C, R, C, C, x, C, gate_msa, N, st));
        // x = x + attn2(x, c)                                                       dit.py:135
        if (hh) HIPRET(dlin16(c, x16, C, L.q2_w, L.q2_b, nullptr, C, R, C, C, nullptr, 0, nullptr, 1, q2_16, st));
        else HIPRET(dlin(c, x, C, L.q2_w, L.q2_b, c->q2.p, C, R, C, C, nullptr, 0, nullptr, 1, st));
        const float* k2 = c->kv2.p + ((size_t)l * 2) * B * M * C;
        const float* v2 = k2 + (size_t)B * M * C;
        if (hh) {
            const int Mp = c->kv2_mp;
            const _Float16* k16 = c->k2_16.p + (size_t)l * B * M * C;
            const _Float16* v16t = c->v2t16.p + (size_t)l * B * H * 64 * Mp;
            HIPRET(launch_flash_attn_hh(dit_flash_hh_args(q2_16, k16, v16t, att16, N, M, Mp, C, C, H, D), H, B, st));
        } else if (flash) {
            HIPRET(launch_flash_attn_f16(dit_flash_args(c->q2.p, k2, v2, c->att.p, att16, N, M, C, C, D), H, B, st));
        } else {
            for (int b = 0; b < B; ++b)
                ERCHK(attention_full(c->q2.p + (size_t)b * N * C, C, k2 + (size_t)b * M * C, C, D, v2 + (size_t)b * M * C, C, D,
                                     c->att.p + (size_t)b * N * C, C, c->sc.p, H, D, N, M, false, st));
        }
        if (hh) HIPRET(dlin16(c, att16, C, L.o2_w, L.o2_b, x, C, R, C, C, x, C, nullptr, 1, nullptr, st));
        else HIPRET(dlin(c, c->att.p, C, L.o2_w, L.o2_b, x, C, R, C, C, x, C, nullptr, 1, st));
        // x = norm2(x) * (1 + scale_mlp) + shift_mlp; x = x + gate_mlp * ff(x)     dit.py:137-139
        HIPRET(dit_ln_mod(x, x, R, N, L.sst, tada, 6LL * C, C, 3, 4, st, x16));
        if (hh) {     // feed-forward in + GEGLU in one launch: the [R][8C] pre-activation never reaches HBM (dit.py FeedForward)
            GemmArgs fg = gemm_args_default();
            fg.A = reinterpret_cast<const float*>(x16); fg.B = reinterpret_cast<const float*>(L.ff0_p16); fg.bias = L.ff0_bp;
            fg.M = R; fg.N = 8 * C; fg.K = C; fg.lda = C; fg.ldb = C; fg.c16 = g16; fg.ldc16 = 4 * C;
            HIPRET(launch_gemm_hh_geglu(fg, st));
        } else {
            HIPRET(dlin(c, x, C, L.ff0_w, L.ff0_b, c->u.p, 8 * C, R, 8 * C, C, nullptr, 0, nullptr, 1, st));
            HIPRET(launch_geglu(c->u.p, c->g.p, (long long)R, 4 * C, st));
        }
        if (hh) HIPRET(dlin16(c, g16, 4 * C, L.ff2_w, L.ff2_b, x, C, R, C, 4 * C, x, C, gate_mlp, N, nullptr, st));
        else HIPRET(dlin(c, c->g.p, 4 * C, L.ff2_w, L.ff2_b, x, C, R, C, 4 * C, x, C, gate_mlp, N, st));
    }
    // shift, scale = scale_shift_table + t_emb; x = norm_out(x) * (1 + scale) + shift; proj_out     dit.py:190-194
    HIPRET(dit_ln_mod(x, x, R, N, c->sst2, temb, (long long)C, 0, 0, 1, st, x16));
    if (hh) HIPRET(dlin16(c, x16, C, c->proj_out_w, c->proj_out_b, out, LD, R, LD, C, nullptr, 0, nullptr, 1, nullptr, st));
    else HIPRET(dlin(c, x, C, c->proj_out_w, c->proj_out_b, out, LD, R, LD, C, nullptr, 0, nullptr, 1, st));
    return 0;
}

extern "C" int er_dit_forward(er_dit_ctx* c, const float* x, const float* cond, const float* t_host, int B, int M, float* out,
                              void* stream) {
    if (!c || !x || !cond || !t_host || !out || B <= 0 || M <= 0) return fail(ER_ERR_INVALID, "er_dit_forward: bad argument");
    ERCHK(er_dit_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    ERCHK(c->t_dev.ensure((size_t)B));
    HIPCHK(hipMemcpyAsync(c->t_dev.p, t_host, B * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    ERCHK(dit_cross_kv(c, cond, B, M, st));
    ERCHK(dit_time_embed(c, B, st));
    return dit_forward_impl(c, x, B, M, out, c->temb.p, c->tada.p, st) < 0 ? -1 : ER_OK;
}

extern "C" int er_dit_sample(er_dit_ctx* c, const float* cond, int B, int M, float* latents, int steps, float guidance,
                             int init_step, void* stream) {
    if (!c || !cond || !latents || B <= 0 || M <= 0 || steps <= 0 || steps > 1000 || init_step < 0 || init_step >= steps)
        return fail(ER_ERR_INVALID, "er_dit_sample: bad argument");
    if ((steps - 1) * (1000 / steps) + 1 >= 1000)   // leading spacing + offset 1: the first timestep must index the 1000-entry table
        return fail(ER_ERR_INVALID, "er_dit_sample: %d steps put the first timestep at %d (>= 1000 training steps)", steps,
                    (steps - 1) * (1000 / steps) + 1);
    ERCHK(er_dit_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const er_dit_config& g = c->cfg;
    const int C = g.hidden_dim, N = g.latent_size, LD = g.latent_dim;
    const size_t nlat = (size_t)B * N * LD;
    // DDIM tables (diffusers DDIMScheduler: leading spacing + offset 1)
    const int T = DIT_TRAIN_STEPS;
    const std::vector<float> ac = dit_alphas_cumprod();
    const int ratio = T / steps;
    // CFG batch: rows [0,B) = zero condition, rows [B,2B) = cond                   models_dit.py:211
    ERCHK(c->czero.ensure((size_t)2 * B * M * C));
    HIPCHK(hipMemsetAsync(c->czero.p, 0, (size_t)B * M * C * 4, st));
    HIPCHK(hipMemcpyAsync(c->czero.p + (size_t)B * M * C, cond, (size_t)B * M * C * 4, hipMemcpyDeviceToDevice, st));
    ERCHK(dit_cross_kv(c, c->czero.p, 2 * B, M, st));
    ERCHK(c->xin.ensure(2 * nlat));
    ERCHK(c->pred.ensure(2 * nlat));
    // time embeddings of ALL the steps that will run, in one pass (round 6): the timesteps are known up front, so the three tiny Linears
    // (2 B rows each, ~13 us per launch on the 64 x 64-tile GEMM), the two SiLUs and the sinusoid run once over nrun x 2 B rows instead
    // of once per step, and the loop needs no host -> device copy and no stream synchronisation any more.  Rows are independent in every
    // one of these kernels: the embeddings are bit-identical to the per-step ones.
    const int nrun = steps - init_step, B2 = 2 * B;
    ERCHK(c->t_dev.ensure((size_t)nrun * B2));
    {
        std::vector<float> th((size_t)nrun * B2);
        for (int k = 0; k < nrun; ++k)
            for (int b = 0; b < B2; ++b) th[(size_t)k * B2 + b] = (float)((steps - 1 - init_step - k) * ratio + 1);   // scheduler.timesteps[init_step:]   models_dit.py:213
        HIPCHK(hipMemcpyAsync(c->t_dev.p, th.data(), th.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));      // th goes out of scope
    }
    ERCHK(dit_time_embed(c, nrun * B2, st));
    for (int k = 0; k < nrun; ++k) {
        const int t = (steps - 1 - init_step - k) * ratio + 1;
        HIPCHK(hipMemcpyAsync(c->xin.p, latents, nlat * 4, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(c->xin.p + nlat, latents, nlat * 4, hipMemcpyDeviceToDevice, st));
        if (dit_forward_impl(c, c->xin.p, B2, M, c->pred.p, c->temb.p + (size_t)k * B2 * C, c->tada.p + (size_t)k * B2 * 6 * C, st) < 0) return -1;
        const int prev = t - ratio;
        const float a_t = ac[t], a_p = prev >= 0 ? ac[prev] : ac[0];
        HIPRET(launch_ddim_cfg_step(c->pred_type == ER_PRED_EPSILON, latents, c->pred.p, (long long)nlat, guidance, sqrtf(a_t),
                                    sqrtf(1.0f - a_t), sqrtf(a_p), sqrtf(1.0f - a_p), st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return ER_OK;
}

// ------------------------------------------------------------------------------------ eval loss (MDiT.forward, core/models_dit.py:119-181)
extern "C" int er_dit_loss(er_dit_ctx* c, const float* latents, const float* noise, const float* cond, const int32_t* timesteps, int B,
                           int M, float snr_gamma, float* pred_out, float* mse_out, float* loss_out, void* stream) {
    if (!c || !latents || !noise || !cond || !timesteps || !mse_out || !loss_out || B <= 0 || M <= 0)
        return fail(ER_ERR_INVALID, "er_dit_loss: bad argument");
    if (B > 65535) return fail(ER_ERR_CAPACITY, "er_dit_loss: batch %d too large", B);
    std::vector<float> coef;
    ERCHK(dit_loss_coefs(timesteps, B, c->pred_type, snr_gamma, coef));
    ERCHK(er_dit_finalize_weights(c));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick(c, stream);
    const long long n = (long long)c->cfg.latent_size * c->cfg.latent_dim;
    if ((long long)B * c->cfg.latent_size * 8 * c->cfg.hidden_dim > 0x7fffffffLL)      // the widest DiT activation (ff.net.0: 8 C per row)
        return fail(ER_ERR_CAPACITY, "er_dit_loss: batch %d too large for 32-bit row indexing", B);
    const int chunks = dit_loss_chunks(n);
    ERCHK(c->lcoef.ensure((size_t)3 * B));
    ERCHK(c->lpart.ensure((size_t)B * chunks));
    ERCHK(c->t_dev.ensure((size_t)B));
    ERCHK(c->xin.ensure((size_t)B * n));
    std::vector<float> th(B);
    for (int b = 0; b < B; ++b) th[b] = (float)timesteps[b];
    HIPCHK(hipMemcpyAsync(c->lcoef.p, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->t_dev.p, th.data(), B * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));        // coef / th go out of scope
    const float *sa = c->lcoef.p, *sb = sa + B, *w = sb + B;
    float* pred = pred_out;
    if (!pred) {
        ERCHK(c->pred.ensure((size_t)B * n));
        pred = c->pred.p;
    }
    // noisy_latents = add_noise(nan_to_num(latents), noise, t); model_pred = dit(noisy_latents, cond, t)     models_dit.py:143-155
    HIPRET(launch_dit_add_noise(latents, noise, c->xin.p, sa, sb, B, n, st));
    ERCHK(dit_cross_kv(c, cond, B, M, st));
    ERCHK(dit_time_embed(c, B, st));
    if (dit_forward_impl(c, c->xin.p, B, M, pred, c->temb.p, c->tada.p, st) < 0) return -1;
    HIPRET(launch_dit_loss(pred, latents, noise, sa, sb, w, B, n, c->pred_type, c->lpart.p, mse_out, loss_out, st));
    return ER_OK;
}

extern "C" int er_k_dit_loss(const float* pred, const float* x0, const float* eps, const int32_t* timesteps, int B, int n, int pred_type,
                             float snr_gamma, float* mse_out, float* loss_out, void* stream) {
    if (!pred || !eps || !timesteps || !mse_out || !loss_out || B <= 0 || B > 65535 || n <= 0 || n % 4 ||
        (pred_type == ER_PRED_V_PREDICTION && !x0) || (pred_type != ER_PRED_V_PREDICTION && pred_type != ER_PRED_EPSILON))
        return fail(ER_ERR_INVALID, "er_k_dit_loss: bad argument");
    for (const void* p : {(const void*)pred, (const void*)x0, (const void*)eps})
        if ((uintptr_t)p % 16) return fail(ER_ERR_INVALID, "er_k_dit_loss: operands must be 16-byte aligned");
    std::vector<float> coef;
    ERCHK(dit_loss_coefs(timesteps, B, pred_type, snr_gamma, coef));
    hipStream_t st = (hipStream_t)stream;
    const int chunks = dit_loss_chunks(n);
    DevBuf<float> dcoef;
    DevBuf<double> part;
    ERCHK(dcoef.ensure(coef.size()));
    ERCHK(part.ensure((size_t)B * chunks));
    hipError_t e = hipMemcpyAsync(dcoef.p, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_dit_loss(pred, x0, eps, dcoef.p, dcoef.p + B, dcoef.p + 2 * B, B, n, pred_type, part.p, mse_out, loss_out, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e != hipSuccess || e2 != hipSuccess) return fail(ER_ERR_HIP, "er_k_dit_loss: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return ER_OK;
}
