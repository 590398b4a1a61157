/*
 * edgerunner_hip.h - C ABI of the MI355X-native (gfx950) ArAE decode path.
 *
 * The reference (NVlabs/EdgeRunner) has no plugin/FFI layer on this path; the
 * seam this library replaces is the call
 *     output_ids = self.mesh_decoder.generate(**kwargs)      core/models.py:303
 * (kwargs built at core/models.py:286-301) together with the arithmetic above
 * and below it inside LMM.generate:
 *     encode_cond          core/models.py:101-144  (+ core/transformer/point.py:172-206)
 *     embd(input_ids)      core/models.py:228      (core/transformer/modeling_opt.py:313)
 *     ShapeOPT.forward     core/transformer/modeling_opt.py:464-517 (prefill + cached steps)
 *     logits processors    core/utils.py:118-141, core/models.py:236-275 (grammar)
 *     greedy / top-k=10 sampling, EOS/pad bookkeeping  (transformers 4.46.2 _sample)
 *
 * Conventions
 *   - plain C types only; every "dev" pointer is a device (HBM) pointer owned by
 *     the caller (e.g. torch-ROCm tensor.data_ptr()), every "host" pointer is
 *     ordinary host memory;
 *   - every function returns 0 on success, a negative er_status otherwise; the
 *     message is retrievable with er_last_error() (thread-local);
 *   - no C++ exception crosses the ABI;
 *   - all device work is enqueued on the caller-supplied hipStream_t (passed as
 *     void*; NULL = the default stream).  A context is bound to one device and
 *     is not thread-safe; different contexts are independent;
 *   - weights, KV cache and workspaces are context-owned (hipMalloc).
 */
#ifndef EDGERUNNER_HIP_H
#define EDGERUNNER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ER_ABI_VERSION 1

typedef enum {
    ER_OK = 0,
    ER_ERR_INVALID = -1,      /* bad argument / shape / state        */
    ER_ERR_HIP = -2,          /* a HIP runtime call failed           */
    ER_ERR_MISSING = -3,      /* a required tensor was never loaded  */
    ER_ERR_CAPACITY = -4,     /* KV cache / position table too small */
    ER_ERR_UNSUPPORTED = -5   /* configuration not built             */
} er_status;

/* Element types.  As the dtype of a CHECKPOINT tensor handed to er_load_tensor / er_dit_load_tensor all three are accepted
 * (converted on the device).  As a context's STORAGE precision (er_config.weight_dtype / kv_dtype) five combinations are
 * built: ER_F32 + ER_F32 (exact mode), ER_F16 + ER_F16 (fast mode, the reference's GPU dtype) and ER_F8E4M3 + ER_F16 (fp8 mode:
 * fast mode with the q / k / v / out_proj / fc1 / fc2 matrices of every decoder layer stored as OCP e4m3fn bytes times 2^e per
 * output row, csrc/er_w8.h; it computes what fast mode computes on a checkpoint rounded that way), and ER_F16 + ER_F8E4M3 and
 * ER_F8E4M3 + ER_F8E4M3 (kv8: fast or fp8 mode with the KV cache stored as one OCP e4m3fn byte per element and no scale -
 * saturating at +-448, round to nearest even, NaN kept, csrc/er_w8.h kv8_encode; head_dim 96 only; single rows decode with version 2,
 * every batched shape with ER_ATTN_STREAM, er_set_prefix_groups is ER_ERR_UNSUPPORTED).  ER_F4E2M1 + ER_F16 and ER_F4E2M1 + ER_F8E4M3
 * are fp4 mode: fast mode (or kv8) with the same six matrices stored as OCP MXFP4 - e2m1 nibbles with one e8m0 scale byte per block of
 * 32 elements along a row, csrc/er_w4.h; it computes what fast mode computes on a checkpoint rounded that way, and the single-row
 * forms of qkv, fc1 and fc2 stream the nibbles where ER_W4_ROWS / the measured rule say so (er_ctx_w4_streams), the matrix-core
 * batched forms of qkv, out_proj, fc1 and fc2 where ER_W4_BATCHED / the measured rule say so (er_ctx_w4_streams_batched).  Every other
 * combination, ER_BF16 storage and ER_F4E2M1 with an fp32 cache included, is rejected by er_create with ER_ERR_UNSUPPORTED.
 * ER_F8E4M3 and ER_F4E2M1 are storage modes only, never checkpoint dtypes. */
typedef enum { ER_F32 = 0, ER_F16 = 1, ER_BF16 = 2, ER_F8E4M3 = 3, ER_F4E2M1 = 4 } er_dtype;
typedef enum { ER_COND_NONE = 0, ER_COND_POINT = 1, ER_COND_POINT_LATENT = 2 } er_cond_mode;
typedef enum { ER_GREEDY = 0, ER_SAMPLE = 1 } er_gen_mode;
/* prefix_allowed_tokens_fn variants LMM.generate can build (core/models.py:236-275) */
typedef enum {
    ER_GRAMMAR_NONE = 0,      /* prefix_allowed_tokens_fn = None                            */
    ER_GRAMMAR_NAIVE9 = 1,    /* tokenizer is None: ids >= 3, EOS iff len % 9 == 1  (:237-242) */
    ER_GRAMMAR_LR_ABSCO = 2   /* meto LR / LR_ABSCO counter automaton               (:246-271) */
} er_grammar;

/* Model description: mirrors ShapeOPTConfig (core/transformer/modeling_opt.py:86-134)
 * and the Options fields LMM.__init__ reads (core/models.py:32-99). */
typedef struct {
    int32_t hidden_dim, num_heads, num_layers, intermediate_dim;
    int32_t vocab_size, max_positions, num_cond_tokens;
    int32_t point_hidden_dim, point_num_heads, point_latent_size, point_latent_dim;
    int32_t point_freq_dim;      /* columns of point_embed.basis (24)          */
    int32_t num_face_buckets;    /* rows of embed_num_face (10); 0 = no face cond */
    int32_t cond_mode;           /* er_cond_mode                               */
    int32_t pad_token_id, bos_token_id, eos_token_id;
    int32_t weight_dtype;        /* er_dtype the decoder weights are streamed in */
    int32_t kv_dtype;            /* er_dtype of the KV cache                    */
    float   ln_eps;              /* 1e-5 (nn.LayerNorm default)                 */
} er_config;

/* kwargs of mesh_decoder.generate (core/models.py:286-301) that are not tensors. */
typedef struct {
    int32_t mode;                /* er_gen_mode: num_beams=1 | do_sample=True     */
    int32_t top_k;               /* 10 in the reference (sample mode only)         */
    int32_t grammar;             /* er_grammar                                    */
    int32_t max_new_tokens;
    int32_t min_new_tokens;      /* HF MinNewTokensLength semantics; 0 = off      */
    uint64_t seed;               /* Philox key of the device sampler              */
} er_decode_params;

typedef struct er_ctx er_ctx;

int         er_abi_version(void);
const char* er_last_error(void);

int er_create(const er_config* cfg, int device, er_ctx** out);
int er_destroy(er_ctx* ctx);

/* Checkpoint loading: one call per state_dict entry, keyed by the reference's own
 * key names (replaces model.load_state_dict, infer.py:44-50).
 * `data` is host (on_device=0) or device (on_device=1) memory, contiguous,
 * row-major.  Unknown keys are ignored (strict=False) and reported via return
 * value 1.  The tensor is converted to the context's storage dtype and repacked
 * (q/k/v fused per layer). */
int er_load_tensor(er_ctx* ctx, const char* key, const void* data, int dtype,
                   int ndim, const int64_t* shape, int on_device);
/* Verifies every required tensor was provided (ER_ERR_MISSING names the first gap). */
int er_finalize_weights(er_ctx* ctx);

/* Pre-allocates the context-owned KV cache for `batch` sequences of up to
 * `max_len` positions (prefix + generated).  Replaces the per-step torch.cat
 * growth of core/transformer/modeling_opt.py:191-192. */
int er_kv_reserve(er_ctx* ctx, int batch, int max_len);

/* encode_cond (core/models.py:101-144), eval mode.
 *   cond_mode POINT:        conds_dev = float[B, N, 3] point clouds
 *   cond_mode POINT_LATENT: conds_dev = float[B, point_latent_size, point_latent_dim], n_points ignored
 *   cond_mode NONE:         conds_dev ignored
 * face_bucket_host = int[B] = quantize_num_faces(num_faces) (core/utils.py:89-116), ignored when
 * num_face_buckets == 0.  cond_out_dev = float[B, num_cond_tokens, hidden_dim]. */
int er_encode_cond(er_ctx* ctx, const float* conds_dev, int batch, int n_points,
                   const int32_t* face_bucket_host, float* cond_out_dev, void* stream);

/* mesh_decoder.model.embd(input_ids) (core/models.py:228): ids_host int[B*R] -> float[B, R, hidden]. */
int er_embed_tokens(er_ctx* ctx, const int32_t* ids_host, int batch, int n_tokens,
                    float* out_dev, void* stream);

/* First generation step of ShapeOPT (prepare_inputs_for_generation step 0,
 * core/transformer/modeling_opt.py:536-538): runs all layers over
 * inputs_embeds float[B, S, hidden], fills KV positions [0, S) and leaves the
 * hidden state of the last position ready for er_logits / er_decode. */
int er_prefill(er_ctx* ctx, const float* embeds_dev, int batch, int seq_len, void* stream);

/* LMM.forward in eval mode (core/models.py:147-202 -> ShapeOPT.forward with labels, modeling_opt.py:464-497).
 * Runs all layers over inputs_embeds float[B,S,hidden] exactly as er_prefill does and leaves the context in the
 * state er_prefill leaves it in.  It then applies final LayerNorm + lm_head to EVERY position and the shifted cross entropy:
 * the target of position s is labels[b, s+1]; -100 and s = S-1 are ignored.
 *   labels_dev   int32[B,S]       (unshifted, as the reference's `labels`)
 *   nll_out_dev  float[B,S]       -log softmax(logits[b,s])[target]; 0 where ignored (NaN for a target outside [0, vocab))
 *   pred_out_dev int32[B,S]       argmax of logits[b,s], first index on ties (torch.argmax); nullable
 *   logits_out_dev float[B,S,V]   nullable (context scratch is used when null)
 *   loss_out_dev float[2]         {mean NLL over supervised positions (NaN if none, like F.cross_entropy), count}
 * ER_ERR_CAPACITY when S >= the reserved cache or B*S*max(intermediate_dim, 3*hidden_dim) >= 2^31 (er_prefill checks the same). */
int er_score(er_ctx* ctx, const float* embeds_dev, const int32_t* labels_dev, int batch, int seq_len,
             float* nll_out_dev, int32_t* pred_out_dev, float* logits_out_dev, float* loss_out_dev, void* stream);

/* posterior.mode() of PointEncoderEmbed (point.py:201) float[B, point_latent_size, point_latent_dim], and
 * kl_out_dev[0] = 0.5 * sum(mean^2) over the WHOLE batch tensor (DummyLatent.kl, point.py:32-34, then .mean() of a scalar);
 * kl_out_dev nullable.  cond_mode POINT only (ER_ERR_UNSUPPORTED otherwise); conds_dev = float[B, n_points, 3]. */
int er_point_latent(er_ctx* ctx, const float* conds_dev, int batch, int n_points, float* latent_out_dev,
                    float* kl_out_dev, void* stream);

/* Options.point_encoder_mode (core/options.py:49): ER_PE_EMBED = PointEncoderEmbed (learned query table, the default),
 * ER_PE_DOWNSAMPLE = PointEncoder (point.py:129-169: the queries are point_embed of point_latent_size points picked per cloud by
 * farthest point sampling, torch_cluster.fps with random_start=False: the first sample is point 0, then argmax of the running
 * min squared distance, lowest index on ties).  Downsample checkpoints have no point_encoder.query_embed: it is not required and
 * loading it returns 1 like any unknown key.  Downsample needs n_points >= point_latent_size (ER_ERR_INVALID otherwise).
 * er_set_point_encoder_mode: cond_mode POINT, before the first er_load_tensor. */
typedef enum { ER_PE_EMBED = 0, ER_PE_DOWNSAMPLE = 1 } er_point_encoder_mode;
int er_set_point_encoder_mode(er_ctx* ctx, int mode);

/* logits[:, -1, :].float() of the most recent forward (prefill or er_feed): float[B, vocab]. */
int er_logits(er_ctx* ctx, float* logits_out_dev, void* stream);

/* One cached decode step with caller-chosen ids (teacher forcing / host-side
 * logits processors): ShapeOPT(input_ids=ids[:, None], past_key_values=...). */
int er_feed(er_ctx* ctx, const int32_t* ids_host, void* stream);

/* The whole generation loop on device (no host round trip per token): replaces
 * GenerationMixin._sample for the reference's kwargs.  out_ids_dev = int64[B, max_new_tokens]
 * (rows padded with pad_token_id after EOS, as HF does); *n_steps_host = number of
 * columns HF would have returned (stops when every row has emitted EOS).
 * Blocks until the result is complete. */
int er_decode(er_ctx* ctx, const er_decode_params* p, int64_t* out_ids_dev,
              int32_t* n_steps_host, void* stream);
/* Sample mode draws are Philox4x32-10(key = seed, counter = (step, stream id of the row)).  The stream id of row b is b until this
 * call sets it (ids_host: n = reserved batch entries; NULL restores the identity).  A caller that shards or batches the reference's
 * serial loop (infer.py:99-101: file x test_repeat x test_num_face) passes the GLOBAL job index of every row, so a job's tokens do
 * not depend on the world size or on which jobs share its batch (torch.multinomial's global generator gives the reference the
 * same property for its serial loop). */
int er_set_row_streams(er_ctx* ctx, const uint32_t* ids_host, int n);

/* ---- sampling controls and per-token log-probs.  What HF's warpers add above the reference's TopK(10), in HF's order (temperature,
 * top-k, top-p), and the two log-probabilities of every chosen id:
 *   model  = logits[id] - logsumexp(logits) over the raw row of the step (-nll of er_score at that position);
 *   policy = log of the probability the id had in the distribution it was taken from: after mask, temperature, top-k and top-p in
 *            sample mode, log_softmax of the masked row in greedy mode.  A finished row's PAD carries 0 and 0.
 * temperature: s / temperature, finite and > 0.  top_k: used when top_k_set != 0, and then 0 means no top-k filter; otherwise
 * er_decode_params.top_k decides, as before.  top_p in (0, 1]: in the order (probability descending, lower id first) a candidate stays
 * iff the mass strictly ahead of it is < top_p (TopPLogitsWarper, min_tokens_to_keep = 1).  The draw stays the inverse CDF in ascending
 * token id from the Philox uniform of (seed, step, row stream).
 * Sticky until changed, like er_set_row_streams, and kept across er_kv_reserve; NULL restores the defaults {1, 1, unset, off}.  er_decode
 * and er_queue_begin read it.  While everything is at its default a call launches exactly the kernels and the captured step it launched
 * before this entry existed; otherwise the step ends in a second head kernel (captured separately, er_ctx_plan is unchanged) which, at
 * temperature 1, top_p 1 and top_k > 0, picks the ids of the first.  ER_ERR_INVALID names the field that is out of range; it is also
 * the answer while a queue is open (er_queue_begin has read the controls: er_queue_end first).
 * With logprobs on, a one-row context runs its step with the kernels that 2 .. 4 rows run (split attention + merge, row fc1 /
 * fc2) in place of its own (version 3, the fused MLP): in exact mode a job's log-probs are then the same bits alone and in a queue of up to 4 slots. */
typedef struct {
    float   temperature;
    float   top_p;
    int32_t top_k;
    int32_t top_k_set;           /* 0: er_decode_params.top_k decides */
    int32_t logprobs;            /* != 0: keep model / policy log-probs of every step (device buffers [B][l_cap], allocated at first use) */
} er_sampling;
int er_set_sampling(er_ctx* ctx, const er_sampling* s);
/* After an er_decode that ran with logprobs on: the first n_steps columns (n_steps <= what er_decode returned) of the two tables into
 * float[B, ld] device buffers (either may be NULL). */
int er_get_logprobs(er_ctx* ctx, float* model_out_dev, float* policy_out_dev, int ld, int n_steps, void* stream);

/* ---- queue mode (continuous batching): a list of independent jobs served from the fixed rows ("slots") of one reserved cache.
 * er_decode runs a batch until its LONGEST row ends; here a row is handed back as soon as its job emits EOS or spends its token
 * budget, and the next job is prefilled into that row while the other rows keep their state.  Between two steps a row's whole state
 * is its slice of the KV cache, its row of the last hidden state and its entries of the generation state, so a refill touches
 * nothing else and the captured step is replayed unchanged.  A free ("parked") row still rides through the step (the grid is
 * fixed): it has budget 0, so the sampling head leaves it alone, and sits at position 0, so its attention reads one key.
 * Contract: a job's tokens are those of the same job run alone through er_prefill + er_decode with the same er_decode_params
 * (max_new_tokens = its budget) and, in sample mode, the same stream id - whatever row it landed in and whatever shares the batch
 * (exact mode: for every slot count; fast mode: within one kernel class, slots <= 4 or slots > 4).
 * Call order: er_kv_reserve(slots, l_cap); er_queue_begin; { er_queue_admit ...; er_queue_run; er_queue_take ... }; er_queue_end.
 * All calls block until their device work is complete.  While a queue is open er_prefill / er_score / er_decode / er_feed fail. */
typedef struct {
    int64_t steps;               /* step replays so far                                                    */
    int64_t admissions;          /* rows admitted (er_queue_admit and er_queue_admit_copy)                 */
    int64_t occupied_row_steps;  /* sum over steps of the rows that held a job (running or waiting)        */
    int64_t wait_row_steps;      /* steps finished jobs spent in their row before er_queue_run listed them */
    int64_t parked_row_steps;    /* sum over steps of the free rows                                        */
    float prefill_ms, decode_ms; /* HIP events around the admissions' forward passes / the replay bursts   */
} er_queue_counters;
/* Opens the queue on the reserved cache: stores *p (max_new_tokens = the largest budget a job may have, the rest as for er_decode)
 * and parks every row.  check_every = steps between two host looks at the rows (0: the 32 of er_decode). */
int er_queue_begin(er_ctx* ctx, const er_decode_params* p, int check_every, void* stream);
/* Prefills n_rows free rows [row0, row0 + n_rows) from embeds_dev float[n_rows, S, hidden] in ONE forward pass and starts their
 * jobs: K/V into positions [0, S) of those rows' cache slices, the last position's state, the generation state at position S, the
 * Philox stream ids (stream_ids_host[n_rows]; NULL: the row index) and the budgets (max_new_host[n_rows]; NULL: p->max_new_tokens).
 * No other row is written.  ER_ERR_INVALID: a row is occupied / outside the slots, a budget outside [1, p->max_new_tokens];
 * ER_ERR_CAPACITY: S + budget + 1 exceeds the reserved cache or the position table. */
int er_queue_admit(er_ctx* ctx, int row0, int n_rows, const float* embeds_dev, int S, const uint32_t* stream_ids_host,
                   const int32_t* max_new_host, void* stream);
/* Starts n jobs in the free rows dst_rows_host[n] (distinct, not src_row, need not be contiguous) as COPIES of the job in src_row, which
 * must be fresh: occupied, not done and not stepped since its admission (no er_queue_run between).  K/V [0, S) of every layer
 * (kv_fork_kernel, csrc/k_kv_fork.h) and the last hidden state are copied from src_row, S being that job's prefill length; the
 * generation state at position S, the stream ids (NULL: the row index) and the budgets (NULL: p->max_new_tokens) are set as er_queue_admit
 * sets them.  No other row is written.  The copies are the jobs er_queue_admit would have started from the source's embeds, one per row:
 * the queue's contract holds for them.  er_queue_counters.admissions counts copied rows too, and prefill_ms includes the copies' time.
 * ER_ERR_INVALID: src_row holds no fresh job, a destination is occupied / named twice / the source / outside the slots, a bad budget;
 * ER_ERR_CAPACITY: S + budget + 1 exceeds the reserved cache or the position table. */
int er_queue_admit_copy(er_ctx* ctx, int src_row, const int32_t* dst_rows_host, int n, const uint32_t* stream_ids_host,
                        const int32_t* max_new_host, void* stream);
/* Replays the step until at least one occupied row is done (EOS emitted or budget spent) and lists every done row in
 * done_rows_host[<= slots].  The host looks every check_every steps, and earlier when a row is about to spend its budget, so a done
 * job waits fewer than check_every steps.  Returns at once with the rows that are already done, or with *n_done = 0 when no row is
 * occupied.  Fails (ER_ERR_INVALID) when a row had no finite candidate score, as er_decode does. */
int er_queue_run(er_ctx* ctx, int32_t* done_rows_host, int32_t* n_done, void* stream);
/* The ids of the finished job in `row`: ids_out_host[0, *n_tokens), *n_tokens = index of EOS + 1, or the budget; no PAD.  Parks the row. */
int er_queue_take(er_ctx* ctx, int row, int64_t* ids_out_host, int capacity, int32_t* n_tokens);
/* The log-probs of the finished job in `row` (queue opened with er_sampling.logprobs on): as many entries as er_queue_take will give ids,
 * into host arrays of `capacity` floats (either may be NULL).  Valid for a done row until that row is taken. */
int er_queue_row_logprobs(er_ctx* ctx, int row, float* model_out_host, float* policy_out_host, int capacity);
int er_queue_stats(er_ctx* ctx, er_queue_counters* out);
/* Closes the queue (jobs still in their rows are dropped) and leaves the context as a fresh er_kv_reserve does: row streams are the
 * identity again, every row's budget is er_decode's max_new_tokens, er_prefill is required before er_decode. */
int er_queue_end(er_ctx* ctx);

/* ---- shared prefix: rows of one reserved batch whose first prefix_len cache positions hold bit-identical K/V in every layer (the
 * same cloud, face count and BOS: many samples of one input) form a GROUP, named by its lowest row, the leader.  With groups set a decode
 * step computes row b's attention over keys [0, prefix_len) read from its LEADER's cache slice and keys [prefix_len, len_b) read from its
 * own, so the prefix crosses HBM once per group and step instead of once per row; nothing else of the step changes, the cache layout and
 * the prefill included (a follower's own [0, prefix_len) entries are written as always and not read by the step).  A row's tokens do not
 * depend on the size of its group, its place in it or the other groups.
 *   leader_host int32[n]: n = the reserved batch, 0 <= leader[b] <= b and leader[leader[b]] == leader[b] (a singleton is its own leader);
 *   prefix_len >= 1.  NULL or prefix_len == 0 clears the groups, and so does the next er_kv_reserve.
 * Call it after er_kv_reserve and before er_prefill.  ER_ERR_INVALID: a bad table, or a queue is open.  ER_ERR_UNSUPPORTED: the reserved
 * plan is not the batched class (B > 4 or ER_FORCE_BATCHED) with head_dim 96.  Setting or clearing rebuilds the stored plan (er_ctx_plan:
 * attn_kernel ER_ATTN_SHARED, merge_launch 1) and drops the captured step.  While groups are set er_prefill refuses seq_len < prefix_len
 * and, after its forward pass, compares every follower's K/V [0, prefix_len) of all layers with its leader's on the device: a mismatch
 * fails with ER_ERR_INVALID naming row and layer, and the context needs a new er_prefill; er_score and er_queue_begin refuse. */
int er_set_prefix_groups(er_ctx* ctx, const int32_t* leader_host, int n, int prefix_len);
/* Which kernel runs the prefix pass of a step under prefix groups.  ER_PREFIX_PASS_VALU (the default): attn_prefix_kernel, fp32 and
 * fp16 caches.  ER_PREFIX_PASS_MFMA: attn_prefix_mfma_kernel (csrc/k_attn_shared_mfma.h) - the rows of a group as columns of the fp16
 * matrix cores, fp16 caches (fast mode) at head_dim 96 only; er_ctx_plan then reports ER_ATTN_SHARED_MFMA.  The initial value comes
 * from env ER_PREFIX_PASS (valu | mfma) at er_create; an fp32- or byte-cache context ignores "mfma" there.  The setting takes effect at
 * the next er_set_prefix_groups, which derives the plan again and drops the captured step.  ER_ERR_UNSUPPORTED: ER_PREFIX_PASS_MFMA on
 * a context whose cache is not fp16 (nothing changes).  ER_ERR_INVALID: another value, or a queue is open. */
enum er_prefix_pass { ER_PREFIX_PASS_VALU = 0, ER_PREFIX_PASS_MFMA = 1 };
int er_set_prefix_pass(er_ctx* ctx, int pass);

/* ---- forked prefill: er_prefill for a reserved batch of n rows of which only the first n_leaders are distinct inputs (many samples of
 * one cloud).  Between two steps a row's whole state is its K/V slice, its row of the last hidden state and its generation-state entries;
 * after a prefill the third is the same for every row and the first two are plain bytes, so a repeat is started by copying.
 *   embeds_dev  float[n_leaders, seq_len, hidden]: the inputs of the leaders only;
 *   leader_host int32[n], n = the reserved batch, leaders first: leader[b] == b for b < n_leaders, leader[b] < n_leaders behind them
 *   (a table of this shape is also a valid er_set_prefix_groups table).
 * Runs exactly the forward pass er_prefill(embeds_dev, n_leaders, seq_len) runs on this context (rows [0, n_leaders) of the cache; the
 * scratch is sized for n_leaders rows), copies every follower's K/V [0, seq_len) of all layers (one kv_fork_kernel launch per 64
 * followers, csrc/k_kv_fork.h; any cache type, the e4m3 byte cache included) and its last hidden state from its leader, and starts the
 * generation state of all n rows at position seq_len.  The context is left as er_prefill leaves it.  Contract: a follower's state equals
 * its leader's bit for bit; the leaders' state is what er_prefill(embeds_dev, n_leaders, seq_len) computes for those rows.  Row stream ids
 * (er_set_row_streams) and budgets are not touched.  With n_leaders == n the call is er_prefill.
 * ER_ERR_INVALID: a table that is not leaders-first, n is not the reserved batch, a queue is open, prefix groups are set with a
 * different leader table, or seq_len < their prefix_len.  ER_ERR_CAPACITY: as er_prefill.  With prefix groups set to the SAME table the
 * call is allowed and er_prefill's device comparison of the followers' prefixes is skipped: those bytes were just copied from the leader. */
int er_prefill_fork(er_ctx* ctx, const float* embeds_dev, int n_leaders, int seq_len, const int32_t* leader_host, int n, void* stream);

/* Prefill with a past: the forward pass over n_new new positions [past_len, past_len + n_new) of every row of the reserved batch, behind
 * past_len cache positions that are kept (modeling_opt.py:191-192, 345-357 with past_key_values).  embeds_new_dev float[batch, n_new,
 * hidden].  Position embeddings come from past_len + t; query t attends to the row's cached keys [0, past_len) and the new keys up to
 * itself; the new positions' K/V go into the cache at their positions, rounded as the mode's prefill rounds them (fp16; kv8: e4m3, in
 * the cache and in what the attention reads); the generation state starts at position past_len + n_new.  Afterwards the context is what
 * er_prefill leaves: er_logits, er_feed and er_decode follow as usual.  The decoder is causal and encode_cond puts the face-count token
 * BEHIND the cloud's tokens (core/models.py:134-141), so another face count, another BOS / resume tail or a rewind of one row batch
 * costs its few positions, not the cloud's 2049.
 * The past: the context records the prefix [0, n) that the last er_prefill / er_prefill_fork / er_score / er_prefill_extend on this
 * reservation wrote for ALL rows; er_decode and er_feed write behind it; er_kv_reserve, er_set_prefix_groups, a queue and a failed
 * forward pass reset it to 0.  1 <= past_len <= n; positions >= past_len are overwritten (rewinding is the point of the call).
 * Attention: n_new up to a measured threshold (csrc/er_extend_plan.h) walks the new queries over 128-key chunks of the row's cache
 * held in registers (csrc/k_attn_extend.h, every cache type); beyond it the prefill's flash kernels run with a causal offset - on the
 * fp32 cache in place, in fast / kv8 mode on fp32 rows gathered from the cache.  ER_EXTEND_ATTN=rows|flash forces a route.
 * ER_ERR_INVALID: bad arguments, batch != the reserved batch, a queue is open, past_len outside [1, n], prefix groups set and past_len
 * < their prefix_len.  ER_ERR_CAPACITY: past_len + n_new >= the reserved length or > max_positions, or er_prefill's 32-bit row rule.
 * All before any launch. */
int er_prefill_extend(er_ctx* ctx, const float* embeds_new_dev, int batch, int past_len, int n_new, void* stream);

/* Rows of the embed_num_face table (core/models.py:137): face_bucket_host int[batch] = quantize_num_faces(num_faces) -> out_dev
 * float[batch, hidden], the token encode_cond appends behind the cloud's - for er_prefill_extend's inputs, without the point encoder.
 * ER_ERR_UNSUPPORTED when num_face_buckets == 0; ER_ERR_INVALID for a bucket outside the table. */
int er_embed_num_face(er_ctx* ctx, const int32_t* face_bucket_host, int batch, float* out_dev, void* stream);

/* ---- mesh tokenizer (host code, no device work): the reference's pybind11 module meto (meto/src/bindings.cpp,
 * meto.Engine(discrete_bins, verbose, backend), meto/meto/__init__.py:21-54) for the backends Options.meto_backend
 * admits (core/options.py:26). */
enum er_meto_backend { ER_METO_LR_ABSCO = 0, ER_METO_LR = 1 };

/* detokenise - the step right after the decode loop.
 * Engine_LR_ABSCO::decode (meto/include/meto/engine_lr_absco.h:223-295) / Engine_LR::decode
 * (meto/include/meto/engine_lr.h:171-253) + Vertex::undiscrete (meto/include/meto/mesh.h:36-42), reached from
 * save_mesh/detokenize_mesh (core/provider.py:39-66,112-147).  tokens_host = meto ids (model ids - 3, cut at EOS).
 * Capacities: vertices_out float[3*(n/3+3)], faces_out int32[3*(n/4+2)], face_type_out int32[n/4+3]. */
int er_meto_decode(const int32_t* tokens_host, int n_tokens, int discrete_bins, int backend, float* vertices_out,
                   int32_t* faces_out, int32_t* face_type_out, int32_t* n_vertices, int32_t* n_faces,
                   int32_t* n_face_types);

/* Engine_LR_ABSCO::encode (meto/include/meto/engine_lr_absco.h:66-220) / Engine_LR::encode
 * (meto/include/meto/engine_lr.h:59-168) over Mesh::Mesh (meto/include/meto/mesh.h:153-262):
 * vertices float[3*n_vertices] in [-1,1], faces int32[3*n_faces].  Capacities: tokens_out >= 10*n_faces and
 * face_order_out / face_type_out >= n_faces for LR_ABSCO; twice that for LR (it can emit a face twice). */
int er_meto_encode(const float* vertices_host, int n_vertices, const int32_t* faces_host, int n_faces,
                   int discrete_bins, int backend, int32_t* tokens_out, int32_t* n_tokens, int32_t* face_order_out,
                   int32_t* face_type_out, int32_t* n_faces_out);

/* ---- DiT image-conditioned front-end (scope row f3): core/transformer/dit.py + core/models_dit.py::MDiT ----
 * Produces the latents [B, latent_size, latent_dim] that LMM.generate consumes in cond_mode 'point_latent'
 * (infer_dit.py:55,111-113).  fp32, built from the prefill kernels (MFMA GEMM, row softmax) plus k_dit.h. */
typedef struct {
    int32_t hidden_dim, num_heads, num_layers;   /* Options.dit_hidden_dim / dit_num_heads / dit_num_layers */
    int32_t latent_size, latent_dim;             /* point_latent_size (2048), point_latent_dim (64)          */
    int32_t clip_dim;                            /* width of the image encoder's last_hidden_state (1280)   */
    int32_t clip_layers, clip_heads, clip_mlp_dim; /* CLIP ViT-H/14: 32 / 16 / 5120; clip_layers = 0: encoder not loaded */
    int32_t clip_image_size, clip_patch;         /* 224 / 14                                                  */
    int32_t weight_dtype;                        /* ER_F32 (exact) or ER_F16: every Linear on fp16-input MFMA, fp32 accumulate */
} er_dit_config;
typedef struct er_dit_ctx er_dit_ctx;
int er_dit_create(const er_dit_config* cfg, int device, er_dit_ctx** out);
int er_dit_destroy(er_dit_ctx* ctx);
/* MDiT checkpoint keys: "dit.*", "proj_cond.*", "norm_cond.*", "image_encoder.vision_model.*" when clip_layers > 0, and
 * "point_encoder.*" after er_dit_attach_point_encoder; any other key is ignored (returns 1) */
int er_dit_load_tensor(er_dit_ctx* ctx, const char* key, const void* data, int dtype, int ndim,
                       const int64_t* shape, int on_device);
int er_dit_finalize_weights(er_dit_ctx* ctx);
/* MDiT.get_cond after the image encoder: cond = norm_cond(proj_cond(clip_hidden))   core/models_dit.py:113
 * clip_hidden_dev float[B, M, clip_dim] -> cond_out_dev float[B, M, hidden_dim] */
int er_dit_project_cond(er_dit_ctx* ctx, const float* clip_hidden_dev, int batch, int m_tokens,
                        float* cond_out_dev, void* stream);
/* The frozen image encoder of MDiT.get_cond (core/models_dit.py:104-111): normalize + bilinear resize to 224 +
 * CLIPVisionModel(...).last_hidden_state.  images_dev float[B,3,H,W] in [0,1] -> clip_hidden_out_dev float[B, 257, clip_dim].
 * Checkpoint keys "image_encoder.vision_model.*" (transformers 4.46.2 names). */
int er_dit_encode_image(er_dit_ctx* ctx, const float* images_dev, int batch, int height, int width,
                        float* clip_hidden_out_dev, void* stream);
/* DiT.forward(x, c, t)   core/transformer/dit.py:168-196: x float[B,N,latent_dim], c float[B,M,hidden], t_host float[B] */
int er_dit_forward(er_dit_ctx* ctx, const float* x_dev, const float* c_dev, const float* t_host, int batch,
                   int m_tokens, float* out_dev, void* stream);
/* MDiT.run's denoise loop (core/models_dit.py:184-229; num_repeat is a repeat_interleave of cond on the caller's
 * side): DDIM (v-prediction, scaled-linear betas 0.00085..0.012, leading spacing, steps_offset 1, eta 0) with
 * classifier-free guidance over [zeros | cond], over scheduler.timesteps[init_step:] (init_step = 0: from pure
 * noise; > 0: the img2img branch, :207-209, the caller has already added noise at timesteps[init_step]).
 * latents_dev float[B, N, latent_dim] holds the starting latents on entry and the result on exit. */
int er_dit_sample(er_dit_ctx* ctx, const float* cond_dev, int batch, int m_tokens, float* latents_dev,
                  int num_inference_steps, float guidance_scale, int init_step, void* stream);

/* What the DiT predicts (Options.noise_scheduler_predtype, core/models_dit.py:80-101): the DDIM update of er_dit_sample (CFG is
 * applied to the prediction either way) and the target of er_dit_loss.  ER_PRED_EPSILON: x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t),
 * x <- sqrt(a_p) x0 + sqrt(1-a_p) eps.  Default ER_PRED_V_PREDICTION. */
typedef enum { ER_PRED_V_PREDICTION = 0, ER_PRED_EPSILON = 1 } er_pred_type;
int er_dit_set_prediction_type(er_dit_ctx* ctx, int pred_type);
/* Gives the context the frozen PointEncoderEmbed of MDiT (core/models_dit.py:68-75; point.py:172-206) with latent_size /
 * latent_dim of the DiT config.  Afterwards er_dit_load_tensor takes the "point_encoder.*" keys and er_dit_finalize_weights
 * requires them.  The encoder runs in fp32 in both DiT precisions (the reference runs it .half()). */
int er_dit_attach_point_encoder(er_dit_ctx* ctx, int point_hidden_dim, int point_num_heads, int point_freq_dim);
/* posterior.mode() of the attached encoder: points_dev float[B, n_points, 3] -> latent_out_dev float[B, latent_size, latent_dim]
 * (as er_point_latent, without the KL term).  ER_ERR_UNSUPPORTED when no encoder is attached. */
int er_dit_point_latent(er_dit_ctx* ctx, const float* points_dev, int batch, int n_points, float* latent_out_dev, void* stream);
/* er_set_point_encoder_mode for the attached encoder: after er_dit_attach_point_encoder, before its first point_encoder.* key. */
int er_dit_set_point_encoder_mode(er_dit_ctx* ctx, int mode);
/* MDiT.forward in eval mode (core/models_dit.py:137-177, no CFG dropout) on given latents, noise and timesteps:
 *   x_t = sqrt(a_t) nan_to_num(latents) + sqrt(1-a_t) noise; pred = DiT(x_t, cond_dev, t) (as er_dit_forward at integer t);
 *   target = sqrt(a_t) noise - sqrt(1-a_t) nan_to_num(latents) (v-prediction) or noise (epsilon);
 *   mse_out_dev[b] = mean((pred - target)^2) of sample b (unweighted), loss_out_dev[0] = mean_b(w_b mse_b) with
 *   w = min(snr, snr_gamma) / (snr + 1) (v) or / snr (epsilon), snr = a_t / (1 - a_t); w = 1 when snr_gamma <= 0 or NaN (None).
 * latents_dev / noise_dev float[B, latent_size, latent_dim], cond_dev float[B, m_tokens, hidden_dim], timesteps_host int32[B] in
 * [0, 1000) (ER_ERR_INVALID otherwise), pred_out_dev (nullable) float[B, latent_size, latent_dim].  Reductions in double, fixed order. */
int er_dit_loss(er_dit_ctx* ctx, const float* latents_dev, const float* noise_dev, const float* cond_dev,
                const int32_t* timesteps_host, int batch, int m_tokens, float snr_gamma, float* pred_out_dev,
                float* mse_out_dev, float* loss_out_dev, void* stream);

/* ---- which kernels a decode context of this shape runs (pure host logic: callable without a device) ----
 * The rules live in ONE function.  er_kv_reserve evaluates it once for the shape it reserves and stores the result, with everything
 * the step derives from it, beside that shape's memory; er_plan_decode evaluates it for a hypothetical shape under the environment
 * of the call (ER_DECODE_V, ER_ATTN_V_BATCHED, ER_FORCE_BATCHED are honoured, l_cap is rounded up to 32 like er_kv_reserve). */
typedef enum { ER_ATTN_SPLIT1 = 1, ER_ATTN_SPLIT2 = 2, ER_ATTN_BALANCED = 3, ER_ATTN_STREAM = 4,
               ER_ATTN_SHARED = 5,   /* prefix groups are set (er_set_prefix_groups): er_ctx_plan only, never er_plan_decode's shape-only rule */
               ER_ATTN_SHARED_MFMA = 6   /* ER_ATTN_SHARED with the matrix-core prefix pass (er_set_prefix_pass): er_ctx_plan only */
} er_attn_kernel;
typedef struct {
    int32_t batched;            /* 1: B > 4 path (matrix-core projections, weights once per 32 rows) */
    int32_t decode_version;     /* single-row path: 3 = balanced chunks + merge fused into out_proj, 2 = fixed chunks + merge kernel */
    int32_t attn_kernel;        /* er_attn_kernel */
    int32_t attn_chunks;        /* chunks per head of the balanced kernel */
    int32_t merge_launch;       /* 1: the attention partials are merged by their own launch */
    int32_t launches_per_layer; /* single-row path only (0 when batched: the count depends on the row passes); a token is
                                   layers x this + lm_head + sample_head launches */
} er_decode_plan;
int er_plan_decode(int batch, int heads, int head_dim, int hidden, int l_cap, er_decode_plan* out);
/* the stored plan of a live context (knobs as read by er_create, cache and ER_FORCE_BATCHED as of the last er_kv_reserve) */
int er_ctx_plan(er_ctx* ctx, er_decode_plan* out);
/* fp8 mode: which of qkv / out_proj / fc1 / fc2 (out[0..3]) the stored plan streams as e4m3 bytes - the row forms at batch <= 4, the
 * matrix-core batched forms above that where the measured rule (or ER_W8_BATCHED=1 at er_create; 0 = nowhere above batch 4) says so.
 * All zero in every other mode.  er_decode_plan keeps its layout. */
int er_ctx_w8_streams(er_ctx* ctx, int32_t out[4]);
/* fp4 mode: which of qkv / out_proj / fc1 / fc2 (out[0..3]) the stored plan streams as e2m1 nibbles - row forms at batch <= 4 only, and
 * only qkv, fc1 and fc2 have one.  ER_W4_ROWS at er_create: 0 = nowhere, 1 = every row form that has a nibble kernel, unset = the
 * measured rule (csrc/er_decode_proj.h w4_streams).  All zero in every other mode. */
int er_ctx_w4_streams(er_ctx* ctx, int32_t out[4]);
/* fp4 mode: which of qkv / out_proj / fc1 / fc2 (out[0..3]) the stored plan streams as e2m1 nibbles in their matrix-core batched forms
 * (batch > 4; a tiled nibble copy, csrc/er_w4_tile_map.h, in place of the fp16 tiled copy).  ER_W4_BATCHED at er_create: 0 = nowhere,
 * 1 = every matrix-core form of the four, unset = the measured rule (csrc/er_w4_rule.h w4_streams_batched).  All zero in every other
 * mode and for a plan that is not batched; er_ctx_w4_streams keeps reporting the row forms only. */
int er_ctx_w4_streams_batched(er_ctx* ctx, int32_t out[4]);
/* tile shape launch_gemm* picks for an [m, n] output in `batch` slices: 1 = 128x128, 2 = 64x128, 3 = 64x64 (ER_GEMM_TILE forces) */
int er_plan_gemm_tile(int m, int n, int batch);

/* ---- measurement ---- */
#define ER_NUM_KERNEL_KINDS 8
/* kinds: 0 qkv_gemv 1 attn_decode 2 attn_combine 3 out_proj_gemv 4 fc1_gemv 5 fc2_gemv 6 lm_head_gemv 7 sample_head */
const char* er_kernel_kind_name(int kind);
/* Times each decode kernel kind in place (HIP events on `stream`, eager launches
 * sweeping all layers so weights are not cache-resident): avg_us_out[kind] =
 * average duration of ONE launch, bytes_out[kind] = algorithmic HBM bytes of one
 * launch at the current context length.  Does not advance the generation state. */
int er_profile_decode_kernels(er_ctx* ctx, int repeats, float* avg_us_out, double* bytes_out, void* stream);
/* Same sweep with the attention kernels run at `context_len` keys (<= the reserved capacity; 0 = the current context
 * length): lets bench.py time the dominant kernel at the MEAN context length of the run it timed, which is what a
 * rocprofv3 --stats average over that run reports.  The launches are captured into a hipGraph and replayed, like the
 * generation loop does (`use_graph` != 0), or issued eagerly. */
int er_profile_decode_kernels_at(er_ctx* ctx, int repeats, int context_len, int use_graph, float* avg_us_out,
                                 double* bytes_out, void* stream);
/* Milliseconds spent inside the last er_decode between its first and last step (HIP events). */
int er_last_decode_ms(er_ctx* ctx, float* ms_out);

/* ---- single-kernel entry points (unit tests call these through the ABI) ---- */
/* y[b,n] = act(sum_k W[n,k] x[b,k] + bias[n]) (+resid) ; ln_w != NULL -> x = LayerNorm(x) first.
 * batch <= 4: the single-row decode kernels; batch > 4: the batched ones exactly as the decode step picks them
 * (matrix-core kernels on a tiled copy of W for the fc1- and fc2-shaped cases, VALU kernels for the narrow ones;
 * env ER_BATCHED_VALU=1 forces the VALU kernels) */
int er_k_gemv(const float* w_dev, const float* bias_dev, const float* x_dev, const float* ln_w_dev,
              const float* ln_b_dev, const float* resid_dev, float* y_dev, float* xnorm_out_dev,
              int batch, int n, int k, int relu, float eps, void* stream);
/* softmax(q K^T / sqrt(D)) V for one new token over a [B,H,Lcap,D] cache holding len[b] keys;
 * steps in {2,4,8}: one workgroup per chunk of 32*steps keys (split kernels); variant = ER_ATTN_SPLIT2 (the single-row fallback:
 * per-wave softmax + one-round-trip merge kernel), ER_ATTN_SPLIT1 (the leaner split kernel of mid-size batches + the same merge)
 * or ER_ATTN_STREAM (one workgroup per (row, head) walks the whole key range, head_dim 96 only).  kv_half, here and in
 * er_k_attn_stream_xt and er_k_gemv_form_args, names the cache type: 0 = fp32, 1 = fp16, 2 = e4m3 bytes (head_dim 96; of the
 * attention variants ER_ATTN_SPLIT2 with steps 4 and ER_ATTN_STREAM read bytes) */
int er_k_attn_decode(const float* q_dev, const void* k_dev, const void* v_dev, const int32_t* len_host,
                     float* out_dev, int batch, int heads, int head_dim, int l_cap, int steps, int kv_half,
                     int variant, void* stream);
/* ONE decode projection in ONE of the forms the decode step launches it in (er_k_gemv reaches the fp32-weight, 4-wave forms only).
 * The projection is named by (k, prologue, epilogue): qkv = 1536 / LN or EMBED / QKV (n = 3 * heads * head_dim, k = heads * head_dim),
 * out_proj = 1536 / NONE / RESID, fc1 = 1536 / LN / RELU, fc2 = 6144 / NONE / RESID, lm_head = 1536 / LN / STORE; the entry runs
 * the decode step's own launch table (one function maps (projection, form) to launches for the step and for this entry) and refuses
 * every (projection, form, batch, weight type) the step's own rule does not allow - and every batched form at batch <= 4 - with
 * ER_ERR_UNSUPPORTED before anything is launched.  Blocks until the work is complete. */
typedef enum { ER_PRO_NONE = 0, ER_PRO_LN = 1, ER_PRO_EMBED = 2,
               ER_PRO_LN_SK = 3      /* LayerNorm of ((p_0 + .. + p_{S-1}) + sk_bias) + sk_resid: a deferred split-K finish (batched forms) */
} er_gemv_prologue;
typedef enum { ER_EPI_STORE = 0, ER_EPI_RELU = 1, ER_EPI_RESID = 2, ER_EPI_QKV = 3 } er_gemv_epilogue;
typedef enum {
    ER_FORM_ROW = 0,           /* batch <= 4 (fp16 fc2 with rw 4 / 6: batch 1): the row kernel with nw waves x rw rows per workgroup */
    ER_FORM_ROWS8 = 1,         /* out_proj, batch 5..8: one pass of the 3-wave row kernel */
    ER_FORM_VALU = 2,          /* batch > 4: the VALU batched kernel, 16 rows per pass */
    ER_FORM_MFMA = 3,          /* batch > 4: matrix cores, 16-wave workgroups, row-major fp32 input (qkv, out_proj, fc1, fc2) */
    ER_FORM_MFMA_XT = 4,       /* the same reading the tiled hi | lo image (fp16 weights; qkv and fc1; fc1 writes xt_out INSTEAD of y) */
    ER_FORM_NARROW = 5,        /* 4-wave workgroups, tiled input, split-K partials finished by the finish kernel (fp16 fc2) */
    ER_FORM_NARROW_DEFER = 6,  /* the same with the partials left to the caller in part_out (fp16 out_proj: 4 slices, fc2: 16) */
    ER_FORM_PREP = 7           /* only the batched forms' prologue launch: xnorm_out (required) and prep_xt_out */
} er_gemv_form;
typedef struct {
    const void* w;             /* [n][k] row-major, fp32 or (w_half) fp16; the matrix-core forms tile a temporary copy */
    const float* bias;         /* [n], nullable */
    const float* x;            /* PRO_NONE: [B][k] fp32 - in the tiled forms the hi | lo image of it (k * 128 bytes per 32 rows); PRO_LN: the pre-LN rows */
    const float *ln_w, *ln_b;  /* PRO_LN / PRO_LN_SK */
    float* xnorm_out;          /* PRO_LN / PRO_EMBED / PRO_LN_SK: the prologue's rows [B][k], nullable except ER_FORM_PREP */
    const float *embd, *posemb;/* PRO_EMBED: token table [V][k], position table [P][k] */
    const int32_t* tok;        /* PRO_EMBED: device int32[B] */
    const int32_t* pos;        /* PRO_EMBED / EPI_QKV: device int32[B], position of the token being fed */
    const float* sk_part;      /* PRO_LN_SK: [groups][sk_slices][rows of the group][k] as ER_FORM_NARROW_DEFER leaves them */
    const float *sk_bias, *sk_resid;   /* [k], [B][k] */
    float* y;                  /* [B][n] (EPI_STORE / RELU / RESID) */
    const float* resid;        /* EPI_RESID: [B][n] */
    float* q_out;              /* EPI_QKV: [B][k] */
    void *kcache, *vcache;     /* EPI_QKV: [B][heads][l_cap][head_dim], fp32, (kv_half 1) fp16 or (kv_half 2) e4m3 bytes; row pos[b] is written */
    void* prep_xt_out;         /* tiled image the batched prologue launch also writes (fp16 weights; caller zeroes it), nullable */
    void* xt_out;              /* ER_FORM_MFMA_XT fc1: the tiled image of the output, n * 128 bytes per 32 rows (caller zeroes it) */
    float* part_out;           /* ER_FORM_NARROW_DEFER: [groups][k / 384][rows of the group][n]; group g starts g * (k / 384) * 32 * n floats in */
    int32_t w_half, kv_half;
    int32_t batch, n, k;
    int32_t prologue, epilogue, form;
    int32_t nw, rw;            /* ER_FORM_ROW */
    int32_t sk_slices;         /* PRO_LN_SK: 4 or 16 */
    int32_t heads, head_dim, l_cap;    /* EPI_QKV */
    float eps;
} er_k_gemv_form_args;
int er_k_gemv_form(const er_k_gemv_form_args* args, void* stream);
/* The fused single-row MLP of the decode step (hidden 1536, intermediate 6144): y = W2 . relu(W1 . LN(x) + b1) + b2 + LN(x) in two
 * launches that fetch a row of the k-major fc2 copy only where the ReLU output is non-zero; bit-identical to fc1 (ER_PRO_LN /
 * ER_EPI_RELU) followed by fc2 (ER_EPI_RESID) of er_k_gemv_form.  er_k_mlp_transpose builds w2t [6144][1536] from fc2.weight
 * [1536][6144] (fp32, or fp16 with w_half).  er_k_mlp_sparse only enqueues: it allocates nothing and does not synchronise, so the
 * pair of launches can be captured into a graph.  Every pointer is device memory. */
int er_k_mlp_transpose(const void* w2_dev, void* w2t_dev, int w_half, void* stream);
typedef struct er_k_mlp_sparse_args {
    const void* w1;            /* [6144][1536] fp32 / fp16 */
    const float* b1;           /* [6144] */
    const void* w2t;           /* [6144][1536] fp32 / fp16 (er_k_mlp_transpose) */
    const void* zero_row;      /* 6144 zero bytes */
    const float* b2;           /* [1536] */
    const float* x;            /* [1536] pre-LayerNorm input */
    const float* ln_w;
    const float* ln_b;
    float* h1_out;             /* [1536] LN(x): written by the first launch, read as the residual by the second */
    float* y;                  /* [1536] */
    float* part;               /* [256][1536] scratch: every word is rewritten by every call */
    int32_t* nnz;              /* [256] live neurons per workgroup (0 .. 24); may be null */
    int32_t w_half;
    float eps;
} er_k_mlp_sparse_args;
int er_k_mlp_sparse(const er_k_mlp_sparse_args* args, void* stream);
/* Live fc1 neurons per (layer, workgroup) that the fused MLP counted in the last decode step of the reserved single-row shape:
 * n = num_layers * 256 counts of 0 .. 24 into out (host memory). */
int er_mlp_nnz(er_ctx* ctx, int32_t* out, int n);
/* The ER_ATTN_STREAM kernel of er_k_attn_decode (head_dim 96) that also writes its output rows into the tiled hi | lo image
 * out_xt_dev (heads * 96 * 128 bytes per 32 rows; rows the batch does not have are left alone), as out_proj's tiled forms read it. */
int er_k_attn_stream_xt(const float* q_dev, const void* k_dev, const void* v_dev, const int32_t* len_host, float* out_dev,
                        void* out_xt_dev, int batch, int heads, int l_cap, int kv_half, void* stream);
/* The two launches of a decode step under prefix groups (er_set_prefix_groups; csrc/k_attn_shared.h), head_dim 96, on a [B,H,Lcap,96]
 * cache: out[b] = attention of q[b] over keys [0, prefix_len) of row leader[b]'s slice and keys [prefix_len, len[b]) of row b's own.
 * leader_host as for er_set_prefix_groups, prefix_len in [1, l_cap], prefix_len <= len[b] <= l_cap.  out_xt_dev (nullable) as for
 * er_k_attn_stream_xt.  Blocks until the work is complete. */
int er_k_attn_shared(const float* q_dev, const void* k_dev, const void* v_dev, const int32_t* len_host, const int32_t* leader_host,
                     int prefix_len, float* out_dev, void* out_xt_dev, int batch, int heads, int l_cap, int kv_half, void* stream);
/* er_k_attn_shared with the matrix-core prefix pass (csrc/k_attn_shared_mfma.h) in front of the same suffix / merge launch: fp16
 * caches only (kv_half = 1; anything else is ER_ERR_UNSUPPORTED). */
int er_k_attn_shared_mfma(const float* q_dev, const void* k_dev, const void* v_dev, const int32_t* len_host, const int32_t* leader_host,
                          int prefix_len, float* out_dev, void* out_xt_dev, int batch, int heads, int l_cap, int kv_half, void* stream);
/* The rows route of er_prefill_extend's attention (csrc/k_attn_extend.h: attn_extend_kernel + attn_extend_merge_kernel) on caller-owned
 * memory: q_dev float[batch, n_new, heads * head_dim], caches [batch, heads, l_cap, head_dim] of the type kv_half names (0 = fp32,
 * 1 = fp16, 2 = e4m3 bytes) holding positions [0, past_len + n_new); out_dev float[batch, n_new, heads * head_dim], row (b, t) = the
 * attention of query (b, t) over keys [0, past_len + t] of row b.  Cache positions >= past_len + n_new are never read.  head_dim 96
 * with every cache type, 64 with fp32 and fp16 (else ER_ERR_UNSUPPORTED).  ER_ERR_INVALID: past_len < 1, n_new outside [1, 65535];
 * ER_ERR_CAPACITY: past_len + n_new > l_cap - all before anything is allocated or launched.  Blocks until the work is complete. */
int er_k_attn_extend(const float* q_dev, const void* k_dev, const void* v_dev, int past_len, int n_new, float* out_dev, int batch, int heads,
                     int l_cap, int head_dim, int kv_half, void* stream);
/* Version 3 of the single-row decode attention (env ER_DECODE_V=3), one row, 16 heads of 96:
 * y[1536] = Wo . softmax(q K^T / sqrt(D)) V + bo + resid over a [16,Lcap,96] cache holding len keys (Lcap <= 8192):
 * balanced chunks (16 per head) + the partial merge fused into the out_proj GEMV; w_half: Wo is fp16 */
int er_k_attn_outproj3(const float* q_dev, const void* k_dev, const void* v_dev, int len, const void* wo_dev,
                       const float* bo_dev, const float* resid_dev, float* y_dev, int l_cap, int kv_half, int w_half,
                       void* stream);
/* fp8 mode on caller-owned operands (csrc/er_w8.h).  er_k_w8_quantize: the weight loader's row quantiser on a matrix [n][k] of
 * fp32 / fp16 / bf16 values in host (on_device = 0) or device memory - per row e = the smallest integer with amax * 2^-e <= 448 in
 * [-15, 7], bytes q = e4m3fn(w * 2^-e) (saturating, round to nearest even), and the dequantised values q * 2^e as fp16.  The four
 * outputs are device memory and nullable: q_dev uint8 [n][k], e_dev int32 [n], w16_dev fp16 [n][k], wscale_dev fp32 [n] = 2^e.
 * A NaN or an infinity in the source is ER_ERR_INVALID.
 * er_k_gemv_form_w8: er_k_gemv_form on (q_dev, wscale_dev) in place of args->w (not read) - ER_FORM_ROW with the fp16 row shapes and
 * the four matrix-core forms (ER_FORM_MFMA, _MFMA_XT, _NARROW, _NARROW_DEFER; the entry tiles the bytes itself), w_half set, of qkv,
 * out_proj, fc1 and fc2 only, with er_k_gemv_form's refusals before any launch; ER_FORM_VALU and ER_FORM_ROWS8 have no byte kernel and
 * are refused.  Bit-identical to er_k_gemv_form on the fp16 matrix q * 2^e.  er_k_attn_outproj3_w8: er_k_attn_outproj3 with Wo as bytes and row scales.  All block. */
int er_k_w8_quantize(const void* src, int dtype, int on_device, int n, int k, void* q_dev, int32_t* e_dev, void* w16_dev,
                     float* wscale_dev, void* stream);
int er_k_gemv_form_w8(const er_k_gemv_form_args* args, const void* q_dev, const float* wscale_dev, void* stream);
int er_k_attn_outproj3_w8(const float* q_dev, const void* k_dev, const void* v_dev, int len, const void* wo_q_dev,
                          const float* wo_scale_dev, const float* bo_dev, const float* resid_dev, float* y_dev, int l_cap,
                          int kv_half, void* stream);
/* fp4 mode on caller-owned operands (csrc/er_w4.h).  er_k_w4_quantize: the weight loader's block quantiser on a matrix [n][k] (k a
 * multiple of 32) of fp32 / fp16 / bf16 values in host (on_device = 0) or device memory - per block of 32 elements along a row e = the
 * smallest integer with amax * 2^-e <= 6 in [-15, 7], codes q = e2m1(w * 2^-e) (saturating, round to nearest, ties to even), and the
 * dequantised values q * 2^e as fp16.  The three outputs are device memory and nullable: block_dev = the canonical block, n * k / 2
 * nibble bytes row-major (element 2 i in the low nibble of byte i) followed by n * k / 32 e8m0 bytes (e + 127) row-major; e_dev int32
 * [n][k / 32]; w16_dev fp16 [n][k].  A NaN or an infinity in the source is ER_ERR_INVALID.
 * er_k_gemv_form_w4: er_k_gemv_form on a canonical block in place of args->w (not read), w_half set, an fp16 or e4m3 cache for qkv.
 * ER_FORM_ROW of qkv, fc1 and fc2: args->nw / rw name the fp16 row form the nibble kernel stands in for, n a multiple of 4; the entry
 * interleaves the block itself (csrc/er_w4_map.h).  ER_FORM_MFMA, _MFMA_XT, _NARROW and _NARROW_DEFER of qkv, out_proj, fc1 and fc2, with
 * the operands er_k_gemv_form takes for them: the entry tiles the block itself (csrc/er_w4_tile_map.h; any n, padded to 32 rows).  The
 * row form of out_proj, the lm_head, ER_FORM_VALU, ER_FORM_ROWS8 and an fp32 cache are ER_ERR_UNSUPPORTED before any launch.
 * Bit-identical to er_k_gemv_form on the fp16 matrix q * 2^e.
 * er_k_w4_cvt_probe: what the hardware's scaled conversion makes of every byte - out_dev fp32 [23][256][4][2]: exponent e = -15 .. 7,
 * byte value, byte select 0 .. 3, (low nibble, high nibble).  All block. */
int er_k_w4_quantize(const void* src, int dtype, int on_device, int n, int k, void* block_dev, int32_t* e_dev, void* w16_dev, void* stream);
int er_k_gemv_form_w4(const er_k_gemv_form_args* args, const void* block_dev, void* stream);
int er_k_w4_cvt_probe(float* out_dev, void* stream);
/* The device encoder of the byte KV cache (kv8; csrc/er_w8.h kv8_encode, what the K/V producers store with) on n fp32 values in
 * device memory: dst_dev receives n e4m3fn bytes.  Blocks. */
int er_k_kv8_encode(const float* src_dev, void* dst_dev, long long n, void* stream);
/* kv_fork_kernel (csrc/k_kv_fork.h) on caller-owned caches kc_dev / vc_dev [layers][batch][heads][l_cap][head_dim] of esz-byte elements
 * (4, 2 or 1): positions [0, len) of every layer and head, K and V, of row src_host[i] are copied to row dst_host[i], i < n_pairs; the
 * pairs of one source form one group (the source is read once for all of them).  ER_ERR_INVALID, before anything is launched: a row
 * outside [0, batch), a destination that is also a source or named twice, len outside [1, l_cap], esz not 1, 2 or 4, a slab len *
 * head_dim * esz that is not a multiple of 16 bytes (or caches not 16-byte aligned).  Unlike the other unit entries it does NOT block
 * and allocates nothing, so that the launch can be captured in a graph. */
int er_k_kv_fork(void* kc_dev, void* vc_dev, int esz, int layers, int batch, int heads, int l_cap, int head_dim, const int32_t* src_host,
                 const int32_t* dst_host, int n_pairs, int len, void* stream);
/* C[M,N] = A[M,K] op(B) (+bias)(relu)(+resid); b_is_kn=0: B is [N,K] (Linear weight), 1: B is [K,N] */
int er_k_gemm(const float* a_dev, const float* b_dev, const float* bias_dev, const float* resid_dev,
              float* c_dev, int m, int n, int k, int lda, int ldb, int ldc, int b_is_kn, int relu,
              float div, void* stream);
/* C[M,N] = relu?(fp16(A fp32 [M,K]) . W fp16 [N,K]^T + bias) (+resid): the fp16-input MFMA GEMM (k % 32 == 0) */
int er_k_gemm_f16(const float* a_dev, const void* w_half_dev, const float* bias_dev, const float* resid_dev,
                  float* c_dev, int m, int n, int k, int lda, int ldb, int ldc, int relu, void* stream);
/* Same shape with the fp32 activations split into fp16 hi + lo parts on their way to the matrix cores (fp32-grade operand,
 * two fp16 MFMAs per fragment): the fast-mode prefill Linears (fp16-stored weights x fp32 activations, fp32 accumulate). */
/* the same product with BOTH operands in fp16 brought in by LDS-DMA (k % 64 == 0): a is rounded to an fp16 copy first (in the
 * DiT path the producing kernel writes that copy); c16_out_dev (optional) receives the result rounded to fp16 [m][n] */
int er_k_gemm_hh(const float* a_dev, const void* w_half_dev, const float* bias_dev, const float* resid_dev, float* c_dev,
                 void* c16_out_dev, int m, int n, int k, int lda, int ldb, int ldc, int relu, void* stream);
/* ONE GEMM family with the whole plain epilogue of the product:
 *   C[m][n] = resid[(resid_mod ? m % resid_mod : m)][n] + gate[m / gate_rows][n] * relu?((A . W^T)[m][n] (/ div) + bias[n]),  c16 = fp16(C)
 * (adaLN gate rows of the DiT blocks; one residual table shared by every batch: the point encoder's cross-attention out_proj).  The
 * entry fills the launch arguments and calls the family's launcher - ER_GEMM_F32: er_k_gemm's kernels (w fp32; ER_GEMM_F32_DMA,
 * ER_GEMM_TILE pick the form), ER_GEMM_F16 / ER_GEMM_F16S: er_k_gemm_f16's / the register-staged split kernels (w fp16; ER_GEMM_TILE),
 * ER_GEMM_HH: the LDS-DMA fp16 kernels on an fp16 copy of a (w fp16; force_tile 1 / 2 / 3 = 128x128 / 64x128 / 64x64, 4 = 256x256,
 * 0 = the product rule, which ER_GEMM_STREAM=2 turns into the streamed form).  a is fp32 [m][lda]; every ld* counts elements of its
 * array; c16 (ER_GEMM_HH only, nullable) has row stride ldc as well; c may be null when c16 is given.  Nullable: bias, resid, gate.
 * ER_ERR_INVALID before anything is launched: a gate with gate_rows <= 0, k not a multiple of 16 (F32) / 32 (F16, F16S) / 64 (HH),
 * lda / ldb that break the 16-byte row alignment, c16 or force_tile outside ER_GEMM_HH.  ER_GEMM_HH blocks until the work is complete. */
typedef enum { ER_GEMM_F32 = 0, ER_GEMM_F16 = 1, ER_GEMM_F16S = 2, ER_GEMM_HH = 3 } er_gemm_family;
typedef struct er_k_gemm_epi_args {
    const float* a;            /* [m][lda] fp32 */
    const void* w;             /* [n][ldb] fp32 (ER_GEMM_F32) or fp16 */
    const float* bias;         /* [n] */
    const float* resid;        /* [resid_mod ? resid_mod : m][ldr] */
    const float* gate;         /* row b at gate + b * gate_bstride, ceil(m / gate_rows) rows of n */
    float* c;                  /* [m][ldc] */
    void* c16;                 /* [m][ldc] fp16 */
    int64_t gate_bstride;
    int32_t family;            /* er_gemm_family */
    int32_t m, n, k, lda, ldb, ldc, ldr;
    int32_t resid_mod, gate_rows;
    int32_t relu, force_tile;
    float div;                 /* != 0: the product is divided by it before the bias */
} er_k_gemm_epi_args;
int er_k_gemm_epi(const er_k_gemm_epi_args* args, void* stream);
/* the fused q/k/v projection of the DiT self-attention (core/transformer/dit.py:100-126 -> attention.py:176-178) as the LDS-DMA
 * kernel runs it: n = 3 * heads * 64 output columns, the first two thirds (q, k) rounded to fp16 into qk16_out_dev [m][n] (its V
 * columns are left untouched), the V third written by the GEMM epilogue as V^T per head into vt_out_dev
 * [m / rows_per_batch][heads][64][rows_per_batch], keys in the order flash_attn_hh_kernel reads them (position of key k inside its
 * group of 16: {0-3, 8-11, 4-7, 12-15}).  m, rows_per_batch multiples of 64; force_tile 0 = the product rule, 1 / 2 / 3 = 128x128 /
 * 64x128 / 64x64 tiles (4 waves), 4 = 256x256 (8 waves). */
int er_k_gemm_hh_qkv(const float* a_dev, const void* w_half_dev, const float* bias_dev, void* qk16_out_dev, void* vt_out_dev, int m,
                     int n, int k, int rows_per_batch, int force_tile, void* stream);
/* the GEGLU feed-forward-in of the DiT block (core/transformer/dit.py FeedForward: x, gate = Linear(h).chunk(2); x * gelu(gate),
 * erf form) as the LDS-DMA kernels run it: out16[m][f] = fp16((fp16(a) . Wx^T + bx) * gelu(fp16(a) . Wg^T + bg)) with w_half_dev the
 * [2 f][k] fp16 weight in checkpoint order; the [m][2 f] pre-activation never reaches HBM.  force_tile 0 = the product rule,
 * 1 / 2 = 128x128 / 64x128 tiles (4 waves), 4 = 256x256 (8 waves, f % 128 == 0): all forms are bit-identical. */
int er_k_gemm_hh_geglu(const float* a_dev, const void* w_half_dev, const float* bias_dev, void* out16_dev, int m, int f, int k,
                       int force_tile, void* stream);
int er_k_gemm_f16s(const float* a, const void* w_half, const float* bias, const float* resid, float* c, int m, int n, int k,
                   int lda, int ldb, int ldc, int relu, void* stream);
/* softmax(q k^T / 8) v, head_dim 64, non-causal, fp16 operands / fp32 accumulate; q,o [B,N,H*64], k,v [B,M,H*64] fp32 */
int er_k_flash_attn_f16(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int batch,
                        int heads, int n_queries, int m_keys, void* stream);
/* softmax(q k^T / sqrt(D) [+ causal mask]) v in exact fp32 on the f32-input matrix cores, no score matrix in HBM
 * (csrc/k_flash_attn_f32.h; replaces attention() of core/transformer/attention.py:27-62 for the prefill, N == M causal,
 * head_dim 96, and for the point encoder's cross-attention, head_dim 64).  q/o: [B, N, H*D], k/v: [B, M, H*D]. */
int er_k_flash_attn_f32(const float* q, const float* k, const float* v, float* o, int batch, int heads, int n, int m,
                        int head_dim, int causal, void* stream);
/* the same attention with q / k / v in fp16 brought in by LDS-DMA (V transposed per head): the unit entry converts and transposes
 * the fp32 inputs first and widens the fp16 output */
int er_k_flash_attn_hh(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int batch, int heads, int n, int m,
                       void* stream);
/* the attention of er_k_flash_attn_f32 for head_dim 96 on the fp16 matrix cores with hi/lo-split q and p (the fast-mode prefill's
 * prefix attention, csrc/k_flash_attn_f16s.h); k / v must hold fp16-representable values (the fast-mode prefill's scratch does) */
int er_k_flash_attn_f16s(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int batch, int heads,
                         int n_queries, int m_keys, int causal, void* stream);
int er_k_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev,
                   int rows, int cols, float eps, void* stream);
/* rows of scores[rows, ld]: softmax over the first n_valid(row) columns (causal: row+1+causal_offset), zeros after */
int er_k_softmax(float* s_dev, int rows, int cols, int ld, int causal, void* stream);
/* er_k_softmax's kernel as the attention calls it: batch score matrices [rows][ld], batch_stride floats apart (>= rows * ld), one
 * launch; row r keeps n_valid = causal ? min(cols, r + 1 + causal_off) : cols columns and columns [n_valid, ld_pad) become 0.
 * ER_ERR_INVALID unless cols <= ld_pad <= ld, causal_off >= 0 and 1 <= batch <= 65535. */
int er_k_softmax_batched(float* s_dev, int rows, int cols, long long ld, int ld_pad, int batch, long long batch_stride, int causal,
                         int causal_off, void* stream);

/* The once-per-sample row, element-wise and K/V scatter kernels (csrc/k_rowops.h, k_dit.h, k_gemm.h split_rows_f16_kernel) on
 * caller-owned device buffers, through the launchers the prefill, the point encoder, the CLIP front and the DiT sampler call.
 * Every entry returns ER_ERR_INVALID before anything is launched for a null pointer, a non-positive size or a shape the kernel's
 * vector accesses or its launcher do not have; a refused call writes nothing.  They enqueue on `stream` and return, except the two
 * that copy a host array (er_k_gather_rows, er_k_adaln_gate_all), which block.
 *
 * er_k_kv_scatter: the fast / kv8 prefill's move of the K and V thirds of qkv_dev [m][3 * hidden] (m = batch * s tokens) into caches
 * [batch][hidden / head_dim][l_cap][head_dim] whose batch rows lie kv_bstride ELEMENTS apart, kv_half 1 = fp16, 2 = e4m3 bytes; the
 * scratch's K / V thirds are rounded in place to the stored values.  Needs m % s == 0, s <= l_cap, hidden % 4 == 0, head_dim % 4 == 0,
 * hidden % head_dim == 0, kv_bstride % 4 == 0 and kv_bstride >= hidden * l_cap. */
int er_k_kv_scatter(float* qkv_dev, void* kcache_dev, void* vcache_dev, int kv_half, int m, int s, int hidden, int head_dim, int l_cap,
                    long long kv_bstride, void* stream);
/* hi = fp16(x), lo = fp16(x - hi) of x_dev [rows][ldx] into dense fp16 [rows][cols]; cols % 4 == 0, ldx % 4 == 0, ldx >= cols */
int er_k_split_rows_f16(const float* x_dev, void* hi_dev, void* lo_dev, long long rows, int cols, int ldx, void* stream);
/* out[b][t][:] = emb[b][t][:] + pos[pos0 + t][:], t < s; c % 4 == 0; out may be emb */
int er_k_add_pos(const float* emb_dev, const float* pos_dev, float* out_dev, int batch, int s, int c, int pos0, void* stream);
/* out[r][0 .. c) = table[ids_host[r]][0 .. c), output rows ldo floats apart; every id in [0, table_rows) */
int er_k_gather_rows(const float* table_dev, int table_rows, const int32_t* ids_host, float* out_dev, int rows, int c, long long ldo,
                     void* stream);
/* PointEmbed features of pts_dev [m][3] with basis_dev [3][f]: [sin | cos | xyz | zeros] in rows of ldo >= 2 f + 3 floats */
int er_k_point_embed(const float* pts_dev, const float* basis_dev, float* out_dev, long long m, int f, int ldo, void* stream);
/* out[r][j] = u[r][j] * gelu_erf(u[r][f + j]), u_dev [rows][2 f] */
int er_k_geglu(const float* u_dev, float* out_dev, long long rows, int f, void* stream);
/* y = gelu_erf(x) / y = x * sigmoid(x) over n elements; y may be x */
int er_k_gelu(const float* x_dev, float* y_dev, long long n, void* stream);
int er_k_silu(const float* x_dev, float* y_dev, long long n, void* stream);
/* The DiT's adaLN modulation y = LayerNorm(x, eps 1e-6, no affine) * (1 + scale_b) + shift_b over x_dev [rows][cols], rows_per_batch
 * rows per batch element (rows % rows_per_batch == 0), with scale_b = table[scale_idx][:] + tvec[b * t_bstride + scale_idx * t_cstride + :]
 * and shift_b likewise; y16_dev (nullable) receives the same rows in fp16; y may be x.  cols must be 1024, strides multiples of 4. */
int er_k_ln_modulate(const float* x_dev, float* y_dev, int rows, int rows_per_batch, int cols, const float* table_dev,
                     const float* tvec_dev, long long t_bstride, long long t_cstride, int shift_idx, int scale_idx, void* y16_dev,
                     void* stream);
/* out[b][:] = table[idx][:] + tada[b][idx][:] with table_dev [6][c], tada_dev [batch][6][c]; idx in [0, 6) */
int er_k_adaln_gate(const float* table_dev, const float* tada_dev, float* out_dev, int batch, int c, int idx, void* stream);
/* the same for chunks 2 and 5 of `layers` tables (tables_host: their device pointers): out_dev [layers][2][batch][c] */
int er_k_adaln_gate_all(const float* const* tables_host, const float* tada_dev, float* out_dev, int layers, int batch, int c, void* stream);
/* out[b] = [sin(t_b w_k) | cos(t_b w_k)], w_k = exp(-ln(10000) k / half), k < half: out_dev [batch][2 * half] */
int er_k_timestep_embed(const float* t_dev, float* out_dev, int batch, int half, void* stream);
/* one DDIM (eta 0) step with classifier-free guidance in place on latents_dev [n]; pred_dev [2][n] = uncond | cond rows;
 * prediction_type an er_pred_type; sa = sqrt(alpha_cumprod), sb = sqrt(1 - alpha_cumprod) at the current (t) and previous (p) step */
int er_k_ddim_cfg_step(float* latents_dev, const float* pred_dev, long long n, int prediction_type, float guidance, float sa_t,
                       float sb_t, float sa_p, float sb_p, void* stream);
/* CLIP normalisation then bilinear resize (align_corners false) of img_dev [batch][3][h][w] to out_dev [batch][3][out_size][out_size] */
int er_k_clip_preprocess(const float* img_dev, float* out_dev, int batch, int h, int w, int out_size, void* stream);
/* the patch Conv2d's A operand: a_dev [batch * (s / p)^2][lda], column c * p * p + ky * p + kx, zeros from 3 p p to lda; s % p == 0 */
int er_k_clip_im2col(const float* px_dev, float* a_dev, int batch, int s, int p, int lda, void* stream);
/* x[b][0] = cls + pos[0]; x[b][1 + i] = patches[b][i] + pos[1 + i], i < np: x_dev [batch][np + 1][c] */
int er_k_clip_assemble(const float* patches_dev, const float* cls_dev, const float* pos_dev, float* x_dev, int batch, int np, int c,
                       void* stream);
/* er_score's head on given logits float[B,S,V] (V <= 1088): nll / pred per position as er_score defines them; loss_out_dev
 * (nullable) = {mean NLL over supervised positions, count} from the fixed-order double reduction */
int er_k_score_rows(const float* logits_dev, const int32_t* labels_dev, int batch, int seq_len, int vocab, float* nll_out_dev,
                    int32_t* pred_out_dev, float* loss_out_dev, void* stream);
/* er_dit_loss's two loss kernels on given tensors float[B, n] (n % 4 == 0, 16-byte aligned; x0_dev may be NULL for epsilon):
 * mse_out_dev float[B], loss_out_dev float[1] as er_dit_loss defines them */
int er_k_dit_loss(const float* pred_dev, const float* x0_dev, const float* eps_dev, const int32_t* timesteps_host, int batch, int n,
                  int pred_type, float snr_gamma, float* mse_out_dev, float* loss_out_dev, void* stream);
/* farthest point sampling of the downsample encoder on given clouds points_dev float[B, n_points, 3] -> idx_out_dev
 * int32[B, n_samples] (0-based within each cloud; 1 <= n_samples <= n_points, B <= 65535) */
int er_k_fps(const float* points_dev, int batch, int n_points, int n_samples, int32_t* idx_out_dev, void* stream);
/* ---- reconstruction fidelity (csrc/k_fidelity.h): how close a generated mesh is to the cloud it was conditioned on.  All three
 * entry points take B <= 65535 and block until their result is in place (like er_k_fps: their scratch is freed on return).
 * er_k_nn_dist2: d2_out_dev[b,i] = min_j d(a[b,i], b[b,j]) with d = (dx*dx + dy*dy) + dz*dz in fp32, every operation rounded on its
 * own; idx_out_dev[b,i] (nullable) = the j that attains it, lowest j on ties.  a_dev float[B,n_a,3], b_dev float[B,n_b,3], any
 * n_a, n_b in [1, 2^30], B <= 65535.  No [n_a][n_b] buffer is allocated (scratch: 8 bytes per query). */
int er_k_nn_dist2(const float* a_dev, const float* b_dev, int batch, int n_a, int n_b, float* d2_out_dev, int32_t* idx_out_dev,
                  void* stream);
/* n_samples area-weighted surface samples of each of `batch` meshes, concatenated: vertices_dev float[vert_offset_host[B],3],
 * faces_dev int32[face_offset_host[B],3] with indices LOCAL to their mesh.  Bit-reproducible: face weights llrint(area * 2^32) from
 * double arithmetic, sample i of mesh m draws Philox4x32-10(key = seed, counter = (i, stream id of m, 0x53555246, 0)); the stream id
 * is m unless stream_ids_host gives it (a caller passes global job indices, as for er_set_row_streams, so a mesh's samples do not
 * depend on what shares its batch).  Precondition: |coordinate| <= 8.  ER_ERR_INVALID names the mesh that has no faces, more than
 * 2^22 faces, zero total area or a face index outside its vertices (checked before any vertex is read through it).  Blocks.
 * points_out_dev float[B,n_samples,3], face_out_dev int32[B,n_samples] (the chosen face, local; nullable). */
int er_k_surface_sample(const float* vertices_dev, const int32_t* faces_dev, const int32_t* vert_offset_host,
                        const int32_t* face_offset_host, int batch, int n_samples, uint64_t seed, const uint32_t* stream_ids_host,
                        float* points_out_dev, int32_t* face_out_dev, void* stream);
/* d2_ab_dev float[B,n_a] (reference cloud -> generated samples), d2_ba_dev float[B,n_b] (generated samples -> reference cloud) ->
 * metrics_out_dev double[B,8] = {chamfer_l1, chamfer_l2, hausdorff, precision, recall, fscore, mean_a2b, mean_b2a}: distances are
 * sqrt((double)d2), "within" is distance < (double)tau, precision / recall are the shares of b / a within tau, fscore = 2PR/(P+R)
 * (0 when P + R = 0).  Sums in double and in a fixed order.  n_a, n_b in [1, 2^30]. */
int er_k_fidelity_metrics(const float* d2_ab_dev, const float* d2_ba_dev, int batch, int n_a, int n_b, float tau,
                          double* metrics_out_dev, void* stream);
/* one sampling-head step on given logits float[B,V]; state arrays are int[B] on device */
int er_k_sample_head(const float* logits_dev, const er_decode_params* p, int vocab, int eos, int pad,
                     int batch, int step, const int32_t* last_tok_host, const int32_t* counter_host,
                     const int32_t* unfinished_host, int32_t* next_tok_host, int32_t* counter_out_host,
                     int32_t* unfinished_out_host, void* stream);
/* The same step through the head with controls (er_set_sampling; s == NULL: the defaults), and what it adds: the two log-probs of the
 * chosen id and the number of candidates the draw chose from (0: greedy, a finished row), each [batch] on the host. */
int er_k_sample_head_ctl(const float* logits_dev, const er_decode_params* p, const er_sampling* s, int vocab, int eos, int pad,
                         int batch, int step, const int32_t* last_tok_host, const int32_t* counter_host,
                         const int32_t* unfinished_host, int32_t* next_tok_host, int32_t* counter_out_host,
                         int32_t* unfinished_out_host, float* lp_model_host, float* lp_policy_host, int32_t* n_kept_host,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EDGERUNNER_HIP_H */
