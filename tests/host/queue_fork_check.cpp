// Stand-alone check of er_queue_admit_copy's host logic (edgerunner_amd/csrc/er_queue_host.h check_admit_copy / admit_copy): every
// refusal, what a copied row looks like afterwards, and the counters.  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o queue_fork_check tests/host/queue_fork_check.cpp
// (tests/test_fork_prefill_cpu.py does).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../edgerunner_amd/csrc/er_queue_host.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

int main() {
    erq::QueueHost q;
    const int32_t one = 1, d1[1] = {1}, d23[2] = {2, 3};
    CHECK(q.check_admit_copy(0, d1, 1, nullptr) == ER_ERR_INVALID);               // no queue open
    q.begin(6, 128, 100, 50, 4);                                                  // 6 slots, cache 128, 100 positions, budgets <= 50
    CHECK(q.check_admit_copy(0, d1, 1, nullptr) == ER_ERR_INVALID);               // the source row is free
    CHECK(strstr(q.why, "free") != nullptr);
    const int32_t b20 = 20;
    CHECK(q.check_admit(0, 1, 40, &b20, 6144) == ER_OK);
    q.admit(0, 1, 40, &b20);
    CHECK(q.stats.admissions == 1);

    // the source
    CHECK(q.check_admit_copy(-1, d1, 1, nullptr) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(6, d1, 1, nullptr) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(1, d23, 2, nullptr) == ER_ERR_INVALID);              // row 1 holds no job
    // the destinations
    CHECK(q.check_admit_copy(0, d1, 0, nullptr) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(0, d1, -3, nullptr) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(0, nullptr, 1, nullptr) == ER_ERR_INVALID);
    const int32_t out_hi[1] = {6}, out_lo[1] = {-1}, self[2] = {1, 0}, twice[3] = {1, 2, 1}, all6[6] = {1, 2, 3, 4, 5, 1};
    CHECK(q.check_admit_copy(0, out_hi, 1, nullptr) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(0, out_lo, 1, nullptr) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(0, self, 2, nullptr) == ER_ERR_INVALID);             // the source among the destinations
    CHECK(q.check_admit_copy(0, twice, 3, nullptr) == ER_ERR_INVALID);            // a destination named twice
    CHECK(strstr(q.why, "twice") != nullptr);
    CHECK(q.check_admit_copy(0, all6, 6, nullptr) == ER_ERR_INVALID);             // more destinations than other rows
    // budgets and capacity, with S = the source's 40
    const int32_t too_big[1] = {51}, zero[1] = {0};
    CHECK(q.check_admit_copy(0, d1, 1, too_big) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(0, d1, 1, zero) == ER_ERR_INVALID);
    CHECK(q.check_admit_copy(0, d1, 1, nullptr) == ER_OK);                        // 40 + 50 + 1 = 91 fits both
    {
        erq::QueueHost t;          // a tighter queue: the default budget overflows the position table, a smaller one fits
        t.begin(3, 128, 80, 50, 0);
        const int32_t b = 39, b1 = 40;
        CHECK(t.check_admit(0, 1, 40, &b, 6144) == ER_OK);
        t.admit(0, 1, 40, &b);
        CHECK(t.check_admit_copy(0, d1, 1, nullptr) == ER_ERR_CAPACITY);          // 40 + 50 + 1 > 80 positions
        CHECK(t.check_admit_copy(0, d1, 1, &b) == ER_OK);                         // 40 + 39 + 1 = 80
        CHECK(t.check_admit_copy(0, d1, 1, &b1) == ER_ERR_CAPACITY);
        erq::QueueHost u;
        u.begin(3, 64, 1000, 50, 0);
        const int32_t c = 10;
        CHECK(u.check_admit(0, 1, 40, &c, 6144) == ER_OK);
        u.admit(0, 1, 40, &c);
        CHECK(u.check_admit_copy(0, d1, 1, nullptr) == ER_ERR_CAPACITY);          // 40 + 50 + 1 > 64 cache positions
        CHECK(strstr(u.why, "reserved cache") != nullptr);
        CHECK(u.check_admit_copy(0, d1, 1, &c) == ER_OK);
    }

    // a good copy: rows 2 and 3 with budgets of their own, not contiguous with the source
    const int32_t buds[2] = {7, 33};
    CHECK(q.check_admit_copy(0, d23, 2, buds) == ER_OK);
    q.admit_copy(0, d23, 2, buds);
    CHECK(q.stats.admissions == 3);                                               // copied rows are admitted rows
    CHECK(q.occupied() == 3);
    CHECK(q.rows[2].occupied && !q.rows[2].done && q.rows[2].S == 40 && q.rows[2].budget == 7 && q.rows[2].steps == 0);
    CHECK(q.rows[3].occupied && q.rows[3].S == 40 && q.rows[3].budget == 33);
    CHECK(!q.rows[1].occupied && !q.rows[4].occupied && !q.rows[5].occupied);     // no other row is touched
    CHECK(q.rows[0].occupied && q.rows[0].budget == 20 && q.rows[0].S == 40);
    CHECK(q.check_admit_copy(0, d23, 2, nullptr) == ER_ERR_INVALID);              // now occupied
    CHECK(strstr(q.why, "occupied") != nullptr);
    // a copy is itself fresh: it can be a source
    const int32_t d4[1] = {4};
    CHECK(q.check_admit_copy(2, d4, 1, &one) == ER_OK);

    // one step later nobody is fresh any more
    CHECK(q.next_burst() == 4);
    q.advance(1);
    CHECK(q.check_admit_copy(0, d1, 1, nullptr) == ER_ERR_INVALID);
    CHECK(strstr(q.why, "has run a step") != nullptr);
    CHECK(q.check_admit_copy(2, d1, 1, nullptr) == ER_ERR_INVALID);
    CHECK(q.stats.occupied_row_steps == 3 && q.stats.parked_row_steps == 3);
    // a done job is no source either (row 2 spends its budget of 7)
    q.advance(6);
    const int ngen[6] = {7, 0, 7, 7, 0, 0}, unf[6] = {1, 0, 1, 1, 0, 0}, eos[6] = {-1, -1, -1, -1, -1, -1};
    int32_t done[6], n = 0;
    CHECK(q.collect(ngen, unf, eos, done, &n) == ER_OK && n == 1 && done[0] == 2);
    CHECK(q.check_admit_copy(2, d1, 1, nullptr) == ER_ERR_INVALID);
    CHECK(strstr(q.why, "done") != nullptr);
    // a newly admitted row is fresh while the old ones are not
    CHECK(q.check_admit(5, 1, 30, &b20, 6144) == ER_OK);
    q.admit(5, 1, 30, &b20);
    CHECK(q.check_admit_copy(5, d1, 1, nullptr) == ER_OK);
    q.admit_copy(5, d1, 1, nullptr);
    CHECK(q.rows[1].S == 30 && q.rows[1].budget == 50 && q.stats.admissions == 5);
    q.end();
    printf("queue_fork_check: ok\n");
    return 0;
}
