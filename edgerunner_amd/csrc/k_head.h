// Device-side sampling head + grammar automaton: what HuggingFace's _sample loop does
// on the host between two forward passes of the reference
// (call site core/models.py:286-303; processors core/utils.py:118-141 and
// core/models.py:236-275; transformers 4.46.2 generation/utils.py::_sample):
//
//   s = logits[:, -1, :].float()
//   [MinNewTokensLength]  s[eos] = -inf while t < min_new_tokens
//   [PrefixConstrained]   s += mask(-inf / 0) from the grammar (integer state machine)
//   greedy: argmax(s) | sample: TopK(10) -> softmax -> one categorical draw
//   next = next*unfinished + pad*(1-unfinished); unfinished &= next != eos
//
// Keeping this on the device removes the per-token host syncs of the reference
// (`0 in attention_mask`, reading input_ids[-1], the EOS check).  One workgroup per
// batch row; all state (token, position, grammar counter, finished flag, output ids)
// lives in HBM so the step can be replayed from a hipGraph.
//
// Two kernels, one set of pieces.  sample_head_kernel (the default step) and sample_head_ctl_kernel (temperature, wide top-k,
// top-p, log-probs) are both written in terms of the head_* functions below: row entry, masked-score fill, block argmax, k-th
// largest on wave 0, ballot compaction, lane-0 serial draw, Philox uniform and state commit each have ONE definition, so the
// grammar, the NaN guard, the queue's row budget and the EOS bookkeeping cannot drift apart.  The ctl kernel's own are the raw
// row's logsumexp, the temperature division, the nucleus sort, the workgroup scan and the inverse-CDF draw.
#pragma once
#include "er_common.h"

namespace er {

struct DecodeParamsDev {       // device copy of er_decode_params + token ids
    int mode, top_k, grammar, max_new, min_new;
    int eos, pad, vocab;
    unsigned int seed_lo, seed_hi;
};

struct GenState {              // per-row arrays, all device
    int* tok;                  // last generated token (input of the next forward)
    int* pos;                  // position the next forward writes its K/V to
    int* counter;              // LR_ABSCO coordinate counter
    int* ngen;                 // tokens generated so far
    int* unfinished;           // 1 while the row has not emitted EOS
    int* eos_step;             // step index at which EOS was emitted (-1)
    int* base_pos;             // prefill length (position of the first generated token's forward)
    int* n_unfinished;         // scalar: rows still running
    int* error;                // scalar: set when a row had no finite candidate score (non-finite logits)
    const unsigned int* row_stream;   // per row: second Philox counter word of the sampler (null: the row index).  A caller that
                               // shards / batches independent jobs sets it to the GLOBAL job index, so a job's draws do not
                               // depend on which rows share its batch (er_set_row_streams)
    const int* row_budget;     // per row: token budget of the job in that row (null: P.max_new for every row).  The queue mode
                               // (er_queue_*) gives every job its own budget <= P.max_new and parks a free row with budget 0
};

// Philox4x32-10 (Salmon et al. 2011): counter-based, so a draw is a pure function of
// (seed, step, row) and a replayed graph needs no RNG state.
__device__ __host__ inline void philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                              unsigned int k0, unsigned int k1, unsigned int out[4]) {
    const unsigned int M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)M0 * c0;
        const unsigned long long p1 = (unsigned long long)M1 * c2;
        const unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
        const unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
        const unsigned int n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Grammar step (integer state machine).  Updates the counter from the last generated
// token and reports the allowed set as {lo, hi, extra EOS / control set}.
//   LR_ABSCO (core/models.py:246-268): t==0 -> {5}; last==5 -> c=9; last in {3,4} -> c=3;
//   last>=6 -> c-=1; c>0 -> [6,V) else {3,4,5,eos}.
//   NAIVE9 (core/models.py:237-242): [3,V) plus eos iff t % 9 == 1.
__device__ __forceinline__ bool grammar_allowed(int grammar, int t, int counter, int i, int V, int eos) {
    if (grammar == 2) {
        if (t == 0) return i == 5;
        if (counter > 0) return i >= 6;
        return i == 3 || i == 4 || i == 5 || i == eos;
    }
    if (grammar == 1) return (i >= 3) || (i == eos && (t % 9) == 1);
    return true;
}

__device__ __forceinline__ int grammar_update(int grammar, int t, int counter, int last) {
    if (grammar != 2 || t == 0) return counter;
    if (last == 5) return 9;
    if (last == 3 || last == 4) return 3;
    if (last >= 6) return counter - 1;
    return counter;
}

// Largest vocabulary the sampling head handles: the reference's are 515 (no meto), 518 (LR_ABSCO) and 1030 (LR, 2*512 + 6;
// core/models.py:78-84).
constexpr int ER_HEAD_MAX_VOCAB = 1088;

// ------------------------------------------------------------------------------------ the pieces both heads are made of
struct HeadRow {               // a row at the entry of its step
    int t, counter;            // tokens generated so far; the grammar counter after the last token
    bool running, past_end;    // not yet closed by EOS; replay past the end (or a parked row of the queue mode): the step is a no-op
};

// Reads only.  Uniform per workgroup: the caller returns on past_end before any barrier, and before it writes anything of the row.
__device__ __forceinline__ HeadRow head_row_entry(const DecodeParamsDev& P, const GenState& st, int b) {
    HeadRow r{};
    r.t = st.ngen[b];
    const int max_new = st.row_budget ? min(P.max_new, st.row_budget[b]) : P.max_new;
    r.past_end = r.t >= max_new;
    const int last = st.tok[b];
    r.running = st.unfinished[b] != 0;
    r.counter = st.counter[b];
    if (r.running) r.counter = grammar_update(P.grammar, r.t, r.counter, last);
    return r;
}

// sc[0, V) = the row's scores with the grammar's and min_new's ids at -inf; ends with the barrier that publishes them.  RAW_MAX:
// the thread's maximum over the RAW scores it read, in the same pass (the ctl head's lp_model); otherwise nothing is kept.
template <bool RAW_MAX>
__device__ __forceinline__ float head_fill_scores(const DecodeParamsDev& P, const HeadRow& r, const float* lg, float* sc) {
    float rmax = -INFINITY;
    for (int i = threadIdx.x; i < P.vocab; i += ER_WG) {
        bool ok = grammar_allowed(P.grammar, r.t, r.counter, i, P.vocab, P.eos);
        if (i == P.eos && r.t < P.min_new) ok = false;
        if constexpr (RAW_MAX) {
            const float x = lg[i];
            rmax = fmaxf(rmax, x);
            sc[i] = ok ? x : -INFINITY;
        } else {
            sc[i] = ok ? lg[i] : -INFINITY;
        }
    }
    __syncthreads();
    return rmax;
}

struct HeadMax {
    float gmax;                // largest masked score: greedy's value and the softmax maximum
    int gidx;                  // its first index (torch.argmax)
    bool no_candidate;         // every masked score is NaN or -inf (fp16 overflow upstream, corrupt weights): HF would raise inside
                               // torch.multinomial; here the row is closed with EOS and the error flag makes er_decode fail loudly
};

// Block argmax with first-index tie-break.  Every thread returns the same triple.  No trailing barrier: a caller that writes red
// again synchronises first.
__device__ __forceinline__ HeadMax head_block_argmax(const float* sc, int V, float* red, int* redi) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += ER_WG) {
        const float v = sc[i];
        if (v > bv) { bv = v; bi = i; }
    }
    auto take = [&](float ov, int oi) { if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; } };
    take(lane_xor_any<32>(bv, lane), (int)lane_xor_bits<32>((unsigned)bi, lane));
    take(lane_xor_any<16>(bv, lane), (int)lane_xor_bits<16>((unsigned)bi, lane));
    take(lane_xor_any<8>(bv, lane), (int)lane_xor_bits<8>((unsigned)bi, lane));
    take(lane_xor_any<4>(bv, lane), (int)lane_xor_bits<4>((unsigned)bi, lane));
    take(lane_xor_any<2>(bv, lane), (int)lane_xor_bits<2>((unsigned)bi, lane));
    take(lane_xor_any<1>(bv, lane), (int)lane_xor_bits<1>((unsigned)bi, lane));
    if (lane == 0) { red[wid] = bv; redi[wid] = bi; }
    __syncthreads();
    HeadMax m{red[0], redi[0], false};
#pragma unroll
    for (int w = 1; w < ER_NWAVES; ++w)
        if (red[w] > m.gmax || (red[w] == m.gmax && redi[w] < m.gidx)) { m.gmax = red[w]; m.gidx = redi[w]; }
    m.no_candidate = m.gidx < 0 || m.gidx >= V || !(m.gmax > -INFINITY);
    return m;
}

// Wave 0: the k-th largest score counting duplicates - remove one maximum k times, the lowest lane first, the scores of the whole
// vocabulary in the wave's registers.  Fewer than k finite scores: -inf.  top_k <= 0: no threshold (-inf) - the ctl head's rule,
// reached through er_sampling only: head_setup and er_k_sample_head guarantee top_k > 0 wherever sample_head_kernel draws.
__device__ __forceinline__ float head_kth_largest(const float* sc, int V, int top_k, float gmax, int lane) {
    if (top_k <= 0) return -INFINITY;
    constexpr int MAXPL = ER_HEAD_MAX_VOCAB / 64;
    float v[MAXPL];
#pragma unroll
    for (int j = 0; j < MAXPL; ++j) { const int i = j * 64 + lane; v[j] = (i < V) ? sc[i] : -INFINITY; }
    const int k = min(top_k, V);
    float kth = gmax;
    for (int it = 0; it < k; ++it) {
        float mv = -INFINITY; int mj = 0;
#pragma unroll
        for (int j = 0; j < MAXPL; ++j) if (v[j] > mv) { mv = v[j]; mj = j; }
        const float wmax = wave_max(mv);
        kth = wmax;
        if (wmax == -INFINITY) break;
        const unsigned long long holders = __ballot(mv == wmax);
        const int first = __ffsll((long long)holders) - 1;
        if (lane == first) {
#pragma unroll
            for (int j = 0; j < MAXPL; ++j) if (j == mj) v[j] = -INFINITY;
        }
    }
    return kth;
}

// Wave 0: the candidates - s >= kth and finite - compacted in ascending token id into cand_i / cand_e (weight expf(s - gmax)), and
// visible to the wave's lanes on return.  Returns their number.
__device__ __forceinline__ int head_compact(const float* sc, int V, float kth, float gmax, int* cand_i, float* cand_e, int lane) {
    int base = 0;
    for (int j = 0; j * 64 < V; ++j) {
        const int i = j * 64 + lane;
        const float s = (i < V) ? sc[i] : -INFINITY;
        const bool c = (s >= kth) && (s > -INFINITY);
        const unsigned long long mask = __ballot(c);
        if (c) {
            const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
            cand_i[slot] = i;
            cand_e[slot] = expf(s - gmax);
        }
        base += __popcll(mask);
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    return base;
}

// the step's uniform in [0, 1): 24 bits of Philox word 0 at counter (t, the row's stream), key = seed
__device__ __forceinline__ float head_uniform(const DecodeParamsDev& P, const GenState& st, int t, int b) {
    unsigned int r[4];
    philox4x32_10((unsigned int)t, st.row_stream ? st.row_stream[b] : (unsigned int)b, 0u, 0u, P.seed_lo, P.seed_hi, r);
    return (float)(r[0] >> 8) * (1.0f / 16777216.0f);
}

struct HeadDraw { int pick; float pe, total; };   // the id drawn, its weight and the weight of all n candidates

// One lane: ascending serial total, then the first candidate whose ascending running sum exceeds u * total; rounding may leave
// u * total above the last sum, then the last candidate.
__device__ __forceinline__ HeadDraw head_serial_draw(const int* cand_i, const float* cand_e, int n, float u, int eos) {
    HeadDraw d{n > 0 ? cand_i[n - 1] : eos, n > 0 ? cand_e[n - 1] : 1.f, 0.f};
    for (int c = 0; c < n; ++c) d.total += cand_e[c];
    const float target = u * d.total;
    float acc = 0.f;
    for (int c = 0; c < n; ++c) {
        acc += cand_e[c];
        if (acc > target) { d.pick = cand_i[c]; d.pe = cand_e[c]; break; }
    }
    return d;
}

// Thread 0 closes the step: the id goes out (PAD for a finished row) and the row's state moves on.  Returns the id written.
__device__ __forceinline__ int head_commit(const DecodeParamsDev& P, const GenState& st, int b, const HeadRow& r, int chosen,
                                           bool no_candidate, long long* out_ids, int out_ld) {
    if (no_candidate && r.running) *st.error = 1;
    const int next = r.running ? chosen : P.pad;
    out_ids[(long long)b * out_ld + r.t] = (long long)next;
    st.tok[b] = next;
    st.counter[b] = r.counter;
    st.pos[b] = st.base_pos[b] + r.t;
    st.ngen[b] = r.t + 1;
    if (r.running && next == P.eos) {
        st.unfinished[b] = 0;
        st.eos_step[b] = r.t;
        atomicSub(st.n_unfinished, 1);
    }
    return next;
}

// grid (B), 256 threads.  Dynamic LDS: vocab floats + 2*vocab ints-ish scratch (see launch).
__global__ __launch_bounds__(ER_WG) void sample_head_kernel(const float* logits, const DecodeParamsDev* pp, GenState st,
                                                            long long* out_ids, int out_ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[8];
    __shared__ int redi[8];
    __shared__ int chosen_s;
    const DecodeParamsDev P = *pp;
    const int V = P.vocab;
    float* sc = smem;                              // [V] masked scores
    float* cand_e = smem + V;                      // [V] candidate weights (compacted)
    int* cand_i = reinterpret_cast<int*>(smem + 2 * V);   // [V] candidate ids (compacted)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const HeadRow row = head_row_entry(P, st, b);
    if (row.past_end) return;
    head_fill_scores<false>(P, row, logits + (long long)b * V, sc);
    const HeadMax m = head_block_argmax(sc, V, red, redi);
    int chosen = m.no_candidate ? P.eos : m.gidx;

    if (P.mode == 1 && !m.no_candidate) {   // sample: TopK(top_k) -> softmax -> categorical
        if (wid == 0) {
            const float kth = head_kth_largest(sc, V, P.top_k, m.gmax, lane);
            const int n = head_compact(sc, V, kth, m.gmax, cand_i, cand_e, lane);
            if (lane == 0) chosen_s = head_serial_draw(cand_i, cand_e, n, head_uniform(P, st, row.t, b), P.eos).pick;
        }
        __syncthreads();
        chosen = chosen_s;
    }

    if (tid == 0) head_commit(P, st, b, row, chosen, m.no_candidate, out_ids, out_ld);
}

// er_feed: teacher-forced token (host-chosen ids copied to ids_dev beforehand)
__global__ void force_token_kernel(const int* ids_dev, GenState st, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int t = st.ngen[b];
    st.tok[b] = ids_dev[b];
    st.pos[b] = st.base_pos[b] + t;
    st.ngen[b] = t + 1;
}

__global__ void init_state_kernel(GenState st, int B, int base_pos) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) { *st.n_unfinished = B; *st.error = 0; }
    if (b >= B) return;
    st.tok[b] = 0; st.pos[b] = base_pos; st.counter[b] = 0; st.ngen[b] = 0;
    st.unfinished[b] = 1; st.eos_step[b] = -1; st.base_pos[b] = base_pos;
}

inline size_t sample_head_lds(int vocab) { return (size_t)vocab * 3 * sizeof(float); }

// ------------------------------------------------------------------------------------ the head with controls and log-probs
// sample_head_ctl_kernel: sample_head_kernel plus what HF's warpers add above TopK(10) - temperature, top-k of any width (0: none) and
// top-p, applied in HF's order - and the two log-probabilities of the chosen id:
//   lp_model  = logits[next] - logsumexp(logits) over the RAW row (what LMM.score reports as -nll)
//   lp_policy = log of the probability the id had in the distribution it was drawn from (greedy: log_softmax(masked)[next])
// er_decode / er_queue_begin launch it only when a control is off its default or log-probs are asked for (er_set_sampling): the default
// path keeps sample_head_kernel and its captured step.  With temperature 1, top_p 1 and top_k > 0 it picks the id sample_head_kernel picks:
// the entry, fill, argmax, threshold, compaction, draw and commit are the same functions.  Every other setting may keep hundreds of
// candidates, so it sums, filters and draws with the whole workgroup instead: a sort in LDS for the nucleus, a scan for the inverse CDF.
struct HeadCtlDev {            // device copy of er_sampling (the effective top_k travels in DecodeParamsDev)
    float temperature, top_p;
};
struct HeadCtlOut {            // where a step leaves its log-probs (null: not kept); n_kept is the unit entry's view of the filters
    float* lp_model;           // [B][ld] at [b][t]
    float* lp_policy;
    int* n_kept;               // [B]: candidates the draw of this step chose from (0: greedy, finished row, no candidate)
    int ld;
};

constexpr int HEAD_CTL_PER_THREAD = 5;   // candidates per thread in the workgroup-wide passes: a contiguous run of the compacted list
constexpr int HEAD_CTL_RANKS = 8;        // ranks per thread of the nucleus' sorted order: 2048 keys, the vocabulary padded to a power of two
static_assert(ER_HEAD_MAX_VOCAB <= HEAD_CTL_PER_THREAD * ER_WG && ER_HEAD_MAX_VOCAB <= HEAD_CTL_RANKS * ER_WG,
              "the workgroup-wide passes cover the whole vocabulary");

// sum of a[0, n) in LDS, the same bits from run to run: every thread adds its strided elements in ascending order, block_sum the rest
__device__ __forceinline__ float head_block_sum(const float* a, int n, float* red) {
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += ER_WG) v += fmaxf(a[i], 0.f);      // a candidate the nucleus dropped carries -1
    return block_sum(v, red);
}

// Inclusive scan of one value per thread (Hillis-Steele, 8 steps through scan[2][ER_WG]); returns the sum of the threads BEFORE this
// one.  Ends with a barrier; a caller that scans again has one more between its reads and the next call.
__device__ __forceinline__ float head_block_scan_before(float (*scan)[ER_WG], float mine) {
    const int tid = threadIdx.x;
    int cur = 0;
    scan[0][tid] = mine;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < ER_WG; off <<= 1) {
        const float x = scan[cur][tid] + (tid >= off ? scan[cur][tid - off] : 0.f);
        scan[cur ^ 1][tid] = x;
        cur ^= 1;
        __syncthreads();
    }
    return tid > 0 ? scan[cur][tid - 1] : 0.f;
}

// grid (B), 256 threads.  Dynamic LDS: sample_head_lds(vocab), as sample_head_kernel.
__global__ __launch_bounds__(ER_WG) void sample_head_ctl_kernel(const float* logits, const DecodeParamsDev* pp, const HeadCtlDev* cp,
                                                                GenState st, long long* out_ids, int out_ld, HeadCtlOut lp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[8];
    __shared__ int redi[8];
    __shared__ int chosen_s, n_cand_s, n_kept_s, first_hit_s, last_kept_s;
    __shared__ float lp_policy_s;
    __shared__ float scan[2][ER_WG];
    __shared__ unsigned long long keys[HEAD_CTL_RANKS * ER_WG];   // the nucleus' sort
    const DecodeParamsDev P = *pp;
    const HeadCtlDev Cc = *cp;
    const int V = P.vocab;
    float* sc = smem;                              // [V] masked scores
    float* cand_e = smem + V;                      // [V] candidate weights (compacted)
    int* cand_i = reinterpret_cast<int*>(smem + 2 * V);   // [V] candidate ids (compacted)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const HeadRow row = head_row_entry(P, st, b);
    if (row.past_end) return;

    // masked scores, and the raw row's logsumexp for lp_model
    const float* lg = logits + (long long)b * V;
    const float rmax = block_max(head_fill_scores<true>(P, row, lg, sc), red);
    float rsum = 0.f;
    for (int i = tid; i < V; i += ER_WG) rsum += expf(lg[i] - rmax);
    rsum = block_sum(rsum, red);
    const float raw_lse = rmax + logf(rsum);

    const HeadMax m = head_block_argmax(sc, V, red, redi);
    __syncthreads();                               // red is reused below
    float gmax = m.gmax;
    int chosen = m.no_candidate ? P.eos : m.gidx;
    float lp_policy = 0.f;
    int n_kept = 0;

    if (P.mode != 1 && !m.no_candidate) {          // greedy: log_softmax(masked)[argmax] = -log(sum exp(s - gmax))
        float e = 0.f;
        for (int i = tid; i < V; i += ER_WG) e += expf(sc[i] - gmax);
        lp_policy = -logf(block_sum(e, red));
    }

    if (P.mode == 1 && !m.no_candidate) {          // sample: temperature -> TopK -> TopP -> softmax -> categorical
        // TemperatureLogitsWarper: a true division (x / 1 is x: the default leaves every bit alone).  It is monotone, so gidx stays
        // a first maximum and the maximum is gmax / temperature
        for (int i = tid; i < V; i += ER_WG) sc[i] = sc[i] / Cc.temperature;
        gmax = gmax / Cc.temperature;
        __syncthreads();
        if (wid == 0) {
            const float kth = head_kth_largest(sc, V, P.top_k, gmax, lane);
            const int n = head_compact(sc, V, kth, gmax, cand_i, cand_e, lane);
            if (lane == 0) { n_cand_s = n; first_hit_s = 0x7fffffff; last_kept_s = -1; n_kept_s = 0; }
            if (P.top_k > 0 && !(Cc.top_p < 1.0f) && lane == 0) {   // sample_head_kernel's draw, sum for sum
                const HeadDraw d = head_serial_draw(cand_i, cand_e, n, head_uniform(P, st, row.t, b), P.eos);
                chosen_s = d.pick;
                lp_policy_s = logf(d.pe / d.total);
                n_kept_s = n;
            }
        }
        __syncthreads();
        if (P.top_k <= 0 || Cc.top_p < 1.0f) {     // wide sets: every pass over the candidates is the whole workgroup's
            const int n = n_cand_s;
            const int c0 = tid * HEAD_CTL_PER_THREAD;
            if (Cc.top_p < 1.0f) {
                // TopPLogitsWarper(min_tokens_to_keep=1): in the order (weight descending, id ascending) a candidate stays iff the mass
                // strictly ahead of it is < top_p.  The order comes from a bitonic sort of 64-bit keys in LDS - inverted weight bits (a
                // positive float orders as its bit pattern) over the compacted index, padded to a power of two with keys that sort last:
                // log2(n) (log2(n) + 1) / 2 passes of n / 512 exchanges per thread, 55 for the 518-id vocabulary, whatever the
                // distribution - then one scan over the ranks gives every candidate the mass ahead of it.
                const float total = head_block_sum(cand_e, n, red);
                int n2 = 2;
                while (n2 < n) n2 <<= 1;
                for (int i = tid; i < n2; i += ER_WG)
                    keys[i] = i < n ? ((unsigned long long)(~__float_as_uint(cand_e[i])) << 32) | (unsigned)i : ~0ull;
                __syncthreads();
                for (int k = 2; k <= n2; k <<= 1)
                    for (int jj = k >> 1; jj > 0; jj >>= 1) {
                        for (int i = tid; i < n2; i += ER_WG) {
                            const int o = i ^ jj;
                            if (o > i) {
                                const unsigned long long x = keys[i], y = keys[o];
                                if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[o] = x; }
                            }
                        }
                        __syncthreads();
                    }
                // rank r holds the r-th candidate of the order; thread tid owns ranks [8 tid, 8 tid + 8)
                const int r0 = tid * HEAD_CTL_RANKS;
                float w[HEAD_CTL_RANKS];
                float mine_r = 0.f;
#pragma unroll
                for (int q = 0; q < HEAD_CTL_RANKS; ++q) {
                    w[q] = (r0 + q < n) ? __uint_as_float(~(unsigned)(keys[r0 + q] >> 32)) : 0.f;
                    mine_r += w[q];
                }
                const float limit = Cc.top_p * total;
                float ahead = head_block_scan_before(scan, mine_r);
#pragma unroll
                for (int q = 0; q < HEAD_CTL_RANKS; ++q) {
                    if (r0 + q < n && !(ahead < limit)) cand_e[(unsigned)keys[r0 + q]] = -1.f;      // dropped (a weight is >= 0)
                    ahead += w[q];
                }
                __syncthreads();
            }
            // a dropped candidate weighs 0 from here on: it takes no part in the sums and is never drawn
            const float total = head_block_sum(cand_e, n, red);
            float e[HEAD_CTL_PER_THREAD];
            bool in[HEAD_CTL_PER_THREAD];
            float mine = 0.f;
            int kept = 0, my_last = -1;
#pragma unroll
            for (int q = 0; q < HEAD_CTL_PER_THREAD; ++q) {
                const float x = (c0 + q < n) ? cand_e[c0 + q] : -1.f;
                in[q] = x >= 0.f;
                e[q] = fmaxf(x, 0.f);
                mine += e[q];
                if (in[q]) { ++kept; my_last = c0 + q; }
            }
            // inverse CDF: acc = weight of candidates [0, c0) before the thread's own run
            float acc = head_block_scan_before(scan, mine);
            const float target = head_uniform(P, st, row.t, b) * total;
            int hit = 0x7fffffff;
#pragma unroll
            for (int q = 0; q < HEAD_CTL_PER_THREAD; ++q) {
                acc += e[q];
                if (in[q] && acc > target && hit == 0x7fffffff) hit = c0 + q;
            }
            if (hit != 0x7fffffff) atomicMin(&first_hit_s, hit);
            if (kept) { atomicMax(&last_kept_s, my_last); atomicAdd(&n_kept_s, kept); }
            __syncthreads();
            if (tid == 0) {
                const int slot = first_hit_s != 0x7fffffff ? first_hit_s : last_kept_s;   // rounding left u * total above the last sum
                chosen_s = slot >= 0 ? cand_i[slot] : P.eos;
                lp_policy_s = slot >= 0 ? logf(cand_e[slot] / total) : 0.f;
            }
            __syncthreads();
        }
        chosen = chosen_s;
        lp_policy = lp_policy_s;
        n_kept = n_kept_s;
    }

    if (tid == 0) {
        const int next = head_commit(P, st, b, row, chosen, m.no_candidate, out_ids, out_ld);
        const bool scored = row.running && !m.no_candidate;
        if (lp.lp_model) lp.lp_model[(long long)b * lp.ld + row.t] = scored ? lg[next] - raw_lse : 0.f;
        if (lp.lp_policy) lp.lp_policy[(long long)b * lp.ld + row.t] = scored ? lp_policy : 0.f;
        if (lp.n_kept) lp.n_kept[b] = row.running ? n_kept : 0;
    }
}

}  // namespace er
