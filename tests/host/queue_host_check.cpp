// Stand-alone check of the queue mode's host logic (edgerunner_amd/csrc/er_queue_host.h): argument validation of er_queue_admit /
// er_queue_take and the row-step counters of er_queue_stats, against a scripted device (every running row emits one token per step
// and EOS at a given length).  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o queue_host_check tests/host/queue_host_check.cpp
// (tests/test_queue_cpu.py does).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "../../edgerunner_amd/csrc/er_queue_host.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

struct FakeDevice {          // the per-row generation state as sample_head_kernel leaves it
    std::vector<int> ngen, unfinished, eos_step, len, budget;
    explicit FakeDevice(int slots) : ngen(slots, 0), unfinished(slots, 0), eos_step(slots, -1), len(slots, 0), budget(slots, 0) {}
    void admit(int b, int length, int bud) { ngen[b] = 0; unfinished[b] = 1; eos_step[b] = -1; len[b] = length; budget[b] = bud; }
    void park(int b) { ngen[b] = 0; unfinished[b] = 0; eos_step[b] = -1; budget[b] = 0; }
    void step() {
        for (size_t b = 0; b < ngen.size(); ++b) {
            if (ngen[b] >= budget[b]) continue;
            if (unfinished[b] && ngen[b] + 1 == len[b]) { unfinished[b] = 0; eos_step[b] = ngen[b]; }
            ++ngen[b];
        }
    }
};

// serves `lens` (EOS lengths) with `budgets` on `slots` rows; returns the counters and the token count per job
static er_queue_counters serve(int slots, int check_every, const std::vector<int>& lens, const std::vector<int>& budgets,
                               std::vector<int>* tokens) {
    erq::QueueHost q;
    const int max_new = *std::max_element(budgets.begin(), budgets.end());
    q.begin(slots, 64 + max_new + 1, 1 << 20, max_new, check_every);
    FakeDevice dev(slots);
    std::deque<int> waiting;
    for (size_t j = 0; j < lens.size(); ++j) waiting.push_back((int)j);
    std::vector<int> job_in(slots, -1);
    std::vector<int32_t> done(slots);
    tokens->assign(lens.size(), -1);
    size_t finished = 0;
    while (finished < lens.size()) {
        for (int b = 0; b < slots && !waiting.empty(); ++b) {
            if (q.rows[b].occupied) continue;
            const int j = waiting.front();
            waiting.pop_front();
            const int32_t bud = budgets[j];
            CHECK(q.check_admit(b, 1, 64, &bud, 6144) == ER_OK);
            q.admit(b, 1, 64, &bud);
            dev.admit(b, lens[j], bud);
            job_in[b] = j;
        }
        int32_t n = q.list_done(done.data());
        while (n == 0) {
            const int burst = q.next_burst();
            CHECK(burst >= 1 && burst <= q.check_every);
            for (int t = 0; t < burst; ++t) dev.step();
            q.advance(burst);
            CHECK(q.collect(dev.ngen.data(), dev.unfinished.data(), dev.eos_step.data(), done.data(), &n) == ER_OK);
        }
        for (int i = 0; i < n; ++i) {
            const int b = done[i];
            CHECK(q.check_take(b, max_new) == ER_OK);
            (*tokens)[job_in[b]] = q.rows[b].n_tokens;
            q.release(b);
            dev.park(b);
            job_in[b] = -1;
            ++finished;
        }
    }
    const er_queue_counters s = q.stats;
    q.end();
    return s;
}

int main() {
    {   // argument validation
        erq::QueueHost q;
        CHECK(q.check_admit(0, 1, 10, nullptr, 6144) == ER_ERR_INVALID);          // no queue open
        q.begin(4, 128, 100, 50, 0);
        CHECK(q.check_every == 32);
        CHECK(q.check_admit(0, 4, 10, nullptr, 6144) == ER_OK);
        CHECK(q.check_admit(-1, 1, 10, nullptr, 6144) == ER_ERR_INVALID);
        CHECK(q.check_admit(3, 2, 10, nullptr, 6144) == ER_ERR_INVALID);
        CHECK(q.check_admit(0, 0, 10, nullptr, 6144) == ER_ERR_INVALID);
        CHECK(q.check_admit(2147483647, 2147483647, 10, nullptr, 6144) == ER_ERR_INVALID);
        CHECK(q.check_admit(0, 1, 0, nullptr, 6144) == ER_ERR_INVALID);
        const int32_t too_big = 51, zero = 0, fits = 20;
        CHECK(q.check_admit(0, 1, 10, &too_big, 6144) == ER_ERR_INVALID);
        CHECK(q.check_admit(0, 1, 10, &zero, 6144) == ER_ERR_INVALID);
        CHECK(q.check_admit(0, 1, 78, nullptr, 6144) == ER_ERR_CAPACITY);         // 78 + 50 + 1 > 128
        CHECK(q.check_admit(0, 1, 77, nullptr, 6144) == ER_ERR_CAPACITY);         // 77 + 50 + 1 = 128 fits the cache, not the 100 positions
        CHECK(q.check_admit(0, 1, 79, &fits, 6144) == ER_OK);                     // 79 + 20 + 1 = 100
        CHECK(q.check_admit(0, 1, 80, &fits, 6144) == ER_ERR_CAPACITY);
        CHECK(q.check_admit(0, 4, 100000, &fits, 6144) < 0);
        q.admit(1, 1, 10, &fits);
        CHECK(q.check_admit(0, 2, 10, nullptr, 6144) == ER_ERR_INVALID);          // row 1 is occupied
        CHECK(q.check_admit(2, 2, 10, nullptr, 6144) == ER_OK);
        CHECK(q.check_take(1, 64) == ER_ERR_INVALID);                             // not finished
        CHECK(q.check_take(4, 64) == ER_ERR_INVALID && q.check_take(-1, 64) == ER_ERR_INVALID);
        CHECK(q.next_burst() == 20);                                              // the budget comes before the 32-step look
        q.advance(20);
        const int ngen[4] = {0, 20, 0, 0}, unf[4] = {0, 1, 0, 0}, eos[4] = {-1, -1, -1, -1};
        int32_t done[4], n = 0;
        CHECK(q.collect(ngen, unf, eos, done, &n) == ER_OK && n == 1 && done[0] == 1);
        CHECK(q.check_take(1, 19) == ER_ERR_CAPACITY && q.check_take(1, 20) == ER_OK);
        CHECK(q.stats.wait_row_steps == 0 && q.stats.occupied_row_steps == 20 && q.stats.parked_row_steps == 60);
        const int bad[4] = {0, 19, 0, 0};
        q.rows[1].done = false;
        CHECK(q.collect(bad, unf, eos, done, &n) == ER_ERR_INVALID);              // the device contradicts the host's count
    }
    {   // the natural-EOS fixture's lengths on two slots, looked at every 4 steps
        const std::vector<int> lens = {95, 39, 11, 39, 95, 11, 11}, budgets(7, 160);
        std::vector<int> tokens;
        const er_queue_counters s = serve(2, 4, lens, budgets, &tokens);
        CHECK(tokens == lens);
        CHECK(s.admissions == 7 && s.wait_row_steps <= 7 * 3);
        long long up = 0, mx = 0;
        for (int n : lens) { const long long u = (n + 3) / 4 * 4; up += u; mx = std::max(mx, u); }
        CHECK(s.steps * 2 <= up + mx);                                            // sum / 2 + (1 - 1 / 2) max
        CHECK(s.occupied_row_steps + s.parked_row_steps == s.steps * 2);
        long long useful = 0;
        for (int n : lens) useful += n;
        CHECK(s.occupied_row_steps == useful + s.wait_row_steps);
    }
    {   // budgets end jobs exactly: nobody waits, whatever the look interval
        const std::vector<int> lens(9, 1 << 20), budgets = {50, 7, 33, 64, 1, 20, 64, 12, 5};
        std::vector<int> tokens;
        const er_queue_counters s = serve(3, 32, lens, budgets, &tokens);
        CHECK(tokens == budgets && s.wait_row_steps == 0 && s.admissions == 9);
    }
    printf("queue_host_check: ok\n");
    return 0;
}
