// Host-side bookkeeping of the queue mode (er_queue_* in include/edgerunner_hip.h): which cache rows ("slots") hold a job, what a job
// may still generate, how many steps the next replay burst may run before the host has to look, and the row-step counters of
// er_queue_stats.  Pure C++ with no device call, so that argument validation and the counter arithmetic can be compiled into a
// stand-alone program and run under the host sanitizers (tests/host/queue_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/edgerunner_hip.h"

namespace erq {

struct Row {
    bool occupied = false;   // a job was admitted and not yet taken
    bool done = false;       // ... and it has emitted EOS or spent its budget (seen by a host look)
    int S = 0;               // prefill length of the job
    int budget = 0;          // tokens the job may generate
    int steps = 0;           // step replays since the job was admitted
    int n_tokens = 0;        // done: tokens er_queue_take returns
};

struct QueueHost {
    bool active = false;
    int slots = 0, l_cap = 0, max_positions = 0, max_new = 0, check_every = 32;
    std::vector<Row> rows;
    er_queue_counters stats{};
    char why[256] = "";

    void begin(int slots_, int l_cap_, int max_positions_, int max_new_, int check_every_) {
        active = true;
        slots = slots_; l_cap = l_cap_; max_positions = max_positions_; max_new = max_new_;
        check_every = check_every_ > 0 ? check_every_ : 32;
        rows.assign((size_t)slots, Row{});
        stats = er_queue_counters{};
        why[0] = 0;
    }
    void end() { active = false; rows.clear(); }

    int budget_of(const int32_t* max_new_host, int i) const { return max_new_host ? max_new_host[i] : max_new; }

    // ER_OK, or the status er_queue_admit returns (the reason in `why`).  width = widest row of the prefill scratch (32-bit indexing).
    int check_admit(int row0, int n_rows, int S, const int32_t* max_new_host, long long width) {
        if (!active) return say(ER_ERR_INVALID, "er_queue_admit: no queue is open (call er_queue_begin)");
        if (n_rows <= 0 || row0 < 0 || row0 > slots - n_rows)
            return say(ER_ERR_INVALID, "er_queue_admit: rows [%d, %d + %d) outside the %d slots", row0, row0, n_rows, slots);
        if (S <= 0) return say(ER_ERR_INVALID, "er_queue_admit: prefix length %d", S);
        for (int i = 0; i < n_rows; ++i)
            if (rows[(size_t)(row0 + i)].occupied) return say(ER_ERR_INVALID, "er_queue_admit: row %d is occupied", row0 + i);
        for (int i = 0; i < n_rows; ++i) {
            const int b = budget_of(max_new_host, i);
            if (b <= 0 || b > max_new)
                return say(ER_ERR_INVALID, "er_queue_admit: budget %d of row %d outside [1, %d] (er_queue_begin's max_new_tokens)", b, row0 + i, max_new);
            const long long need = (long long)S + b + 1;
            if (need > l_cap) return say(ER_ERR_CAPACITY, "er_queue_admit: prefix %d + budget %d + 1 > reserved cache (%d)", S, b, l_cap);
            if (need > max_positions) return say(ER_ERR_CAPACITY, "er_queue_admit: prefix %d + budget %d + 1 > position table (%d)", S, b, max_positions);
        }
        if ((long long)n_rows * S * width > 0x7fffffffLL)
            return say(ER_ERR_CAPACITY, "er_queue_admit: %d x %d positions x %lld columns overflows the 32-bit row indexing of the prefill", n_rows, S, width);
        return ER_OK;
    }
    void admit(int row0, int n_rows, int S, const int32_t* max_new_host) {
        for (int i = 0; i < n_rows; ++i) {
            Row& r = rows[(size_t)(row0 + i)];
            r = Row{};
            r.occupied = true; r.S = S; r.budget = budget_of(max_new_host, i);
        }
        stats.admissions += n_rows;
    }

    // er_queue_admit_copy: n free rows dst_rows[i] start as copies of the FRESH job in src_row (occupied, not done, no step replayed since
    // its admission: only then do its K/V [0, S), its last hidden state and its generation state still describe "right after the prefill").
    int check_admit_copy(int src_row, const int32_t* dst_rows, int n, const int32_t* max_new_host) {
        if (!active) return say(ER_ERR_INVALID, "er_queue_admit_copy: no queue is open (call er_queue_begin)");
        if (src_row < 0 || src_row >= slots) return say(ER_ERR_INVALID, "er_queue_admit_copy: source row %d outside the %d slots", src_row, slots);
        const Row& s = rows[(size_t)src_row];
        if (!s.occupied || s.done || s.steps != 0)
            return say(ER_ERR_INVALID, "er_queue_admit_copy: source row %d holds no fresh job (%s)", src_row,
                       !s.occupied ? "it is free" : s.done ? "its job is done" : "its job has run a step");
        if (n <= 0 || n >= slots || !dst_rows) return say(ER_ERR_INVALID, "er_queue_admit_copy: %d destination rows", n);
        for (int i = 0; i < n; ++i) {
            const int d = dst_rows[i];
            if (d < 0 || d >= slots) return say(ER_ERR_INVALID, "er_queue_admit_copy: destination row %d outside the %d slots", d, slots);
            if (d == src_row) return say(ER_ERR_INVALID, "er_queue_admit_copy: row %d is the source and a destination", d);
            if (rows[(size_t)d].occupied) return say(ER_ERR_INVALID, "er_queue_admit_copy: row %d is occupied", d);
            for (int k = 0; k < i; ++k)
                if (dst_rows[k] == d) return say(ER_ERR_INVALID, "er_queue_admit_copy: row %d is a destination twice", d);
        }
        for (int i = 0; i < n; ++i) {
            const int b = budget_of(max_new_host, i);
            if (b <= 0 || b > max_new)
                return say(ER_ERR_INVALID, "er_queue_admit_copy: budget %d of row %d outside [1, %d] (er_queue_begin's max_new_tokens)", b, dst_rows[i], max_new);
            const long long need = (long long)s.S + b + 1;
            if (need > l_cap) return say(ER_ERR_CAPACITY, "er_queue_admit_copy: prefix %d + budget %d + 1 > reserved cache (%d)", s.S, b, l_cap);
            if (need > max_positions) return say(ER_ERR_CAPACITY, "er_queue_admit_copy: prefix %d + budget %d + 1 > position table (%d)", s.S, b, max_positions);
        }
        return ER_OK;
    }
    void admit_copy(int src_row, const int32_t* dst_rows, int n, const int32_t* max_new_host) {
        const int S = rows[(size_t)src_row].S;
        for (int i = 0; i < n; ++i) {
            Row& r = rows[(size_t)dst_rows[i]];
            r = Row{};
            r.occupied = true; r.S = S; r.budget = budget_of(max_new_host, i);
        }
        stats.admissions += n;      // a copied row is an admitted row
    }

    int occupied() const { return (int)std::count_if(rows.begin(), rows.end(), [](const Row& r) { return r.occupied; }); }
    int list_done(int32_t* out) const {
        int n = 0;
        for (int b = 0; b < slots; ++b)
            if (rows[(size_t)b].occupied && rows[(size_t)b].done) out[n++] = b;
        return n;
    }
    // Steps to replay before the next host look: check_every, or fewer when a running row spends its budget earlier (the host
    // knows ngen of a running row without looking: one token per step).  0: no row is running.
    int next_burst() const {
        int k = 0;
        for (const Row& r : rows)
            if (r.occupied && !r.done) {
                const int left = std::max(1, r.budget - r.steps);
                k = k == 0 ? std::min(check_every, left) : std::min(k, left);
            }
        return k;
    }
    void advance(int n) {
        const int occ = occupied();
        stats.steps += n;
        stats.occupied_row_steps += (int64_t)n * occ;
        stats.parked_row_steps += (int64_t)n * (slots - occ);
        for (Row& r : rows)
            if (r.occupied) r.steps += n;
    }
    // After a look: ngen / unfinished / eos_step as the device holds them, [slots] each.  Marks the rows that finished, charges the
    // steps they waited, lists every done row.  ER_ERR_INVALID when the device state contradicts the host's count.
    int collect(const int* ngen, const int* unfinished, const int* eos_step, int32_t* done_rows, int32_t* n_done) {
        for (int b = 0; b < slots; ++b) {
            Row& r = rows[(size_t)b];
            if (!r.occupied || r.done) continue;
            if (ngen[b] != std::min(r.steps, r.budget))
                return say(ER_ERR_INVALID, "er_queue_run: row %d holds %d tokens after %d steps (budget %d)", b, ngen[b], r.steps, r.budget);
            const bool eos = unfinished[b] == 0;
            if (eos && (eos_step[b] < 0 || eos_step[b] >= r.budget))
                return say(ER_ERR_INVALID, "er_queue_run: row %d finished at step %d outside its budget %d", b, eos_step[b], r.budget);
            if (!eos && ngen[b] < r.budget) continue;
            r.done = true;
            r.n_tokens = eos ? eos_step[b] + 1 : r.budget;
            stats.wait_row_steps += r.steps - r.n_tokens;
        }
        *n_done = list_done(done_rows);
        return ER_OK;
    }
    int check_take(int row, int capacity) {
        if (!active) return say(ER_ERR_INVALID, "er_queue_take: no queue is open");
        if (row < 0 || row >= slots) return say(ER_ERR_INVALID, "er_queue_take: row %d outside the %d slots", row, slots);
        const Row& r = rows[(size_t)row];
        if (!r.occupied || !r.done) return say(ER_ERR_INVALID, "er_queue_take: row %d holds no finished job", row);
        if (capacity < r.n_tokens) return say(ER_ERR_CAPACITY, "er_queue_take: %d tokens do not fit a buffer of %d", r.n_tokens, capacity);
        return ER_OK;
    }
    void release(int row) { rows[(size_t)row] = Row{}; }

    __attribute__((format(printf, 3, 4))) int say(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, sizeof(why), fmt, ap);
        va_end(ap);
        return code;
    }
};

}  // namespace erq
