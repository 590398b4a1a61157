// Stand-alone check of the host rules of the prefill with a past (edgerunner_amd/csrc/er_extend_plan.h): the attention route over every
// n_new up to a few thousand, with and without the rows kernels and under each value of the ER_EXTEND_ATTN switch, and the rule for the
// past a call may keep.  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o extend_plan_check tests/host/extend_plan_check.cpp
// (tests/test_prefill_extend_cpu.py does).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../edgerunner_amd/csrc/er_extend_plan.h"

#define CHECK(cond)                                                                                                        \
    do {                                                                                                                   \
        if (!(cond)) {                                                                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at %s\n", __FILE__, __LINE__, #cond, where);                          \
            exit(1);                                                                                                       \
        }                                                                                                                  \
    } while (0)

using namespace er;

int main() {
    char where[128] = "";
    long routes = 0, pasts = 0;
    static_assert(EXTEND_ROWS_MAX_NEW >= 2, "another face count (face token + BOS) takes the rows route");
    static_assert(EXTEND_ROWS_MAX_NEW <= 65535, "the merge launch's grid holds n_new");
    int switches = 0;
    for (int n = 1; n <= 4100; ++n) {
        snprintf(where, sizeof(where), "n_new=%d", n);
        const ExtendRoute dflt = extend_attn_route(n, true, nullptr);
        CHECK(dflt == (n <= EXTEND_ROWS_MAX_NEW ? EXTEND_ROWS : EXTEND_FLASH));
        CHECK(extend_attn_route(n, true, "") == dflt);                     // an empty or unknown value is the measured rule
        CHECK(extend_attn_route(n, true, "auto") == dflt);
        CHECK(extend_attn_route(n, true, "rows") == EXTEND_ROWS);
        CHECK(extend_attn_route(n, true, "flash") == EXTEND_FLASH);
        for (const char* env : {(const char*)nullptr, "rows", "flash", "x"}) CHECK(extend_attn_route(n, false, env) == EXTEND_FLASH);
        if (n > 1 && dflt != extend_attn_route(n - 1, true, nullptr)) ++switches;
        routes += 8;
    }
    CHECK(switches == 1);                                                   // one threshold: rows below it, flash above
    CHECK(extend_attn_route(70000, true, "rows") == EXTEND_FLASH);          // beyond the merge grid even the switch takes the flash route
    for (int valid = 0; valid <= 70; ++valid)
        for (int prefix = 0; prefix <= 70; prefix += 7)
            for (int past = -2; past <= 75; ++past) {
                snprintf(where, sizeof(where), "valid=%d prefix=%d past=%d", valid, prefix, past);
                const int r = extend_past_check(past, valid, prefix);
                const bool in_range = past >= 1 && past <= valid;
                CHECK((r == 1) == !in_range);
                CHECK((r == 2) == (in_range && prefix > 0 && past < prefix));
                CHECK((r == 0) == (in_range && (prefix == 0 || past >= prefix)));
                ++pasts;
            }
    printf("extend_plan_check: ok (%ld routes, %ld pasts, rows up to n_new = %d)\n", routes, pasts, EXTEND_ROWS_MAX_NEW);
    return 0;
}
