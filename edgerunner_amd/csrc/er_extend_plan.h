// Which attention route a prefill with a past takes (er_prefill_extend, csrc/k_attn_extend.h), and what the call may rewind to.  Pure
// C++ with no device call (csrc/er_decode_plan.h is the precedent), enumerated by tests/host/extend_plan_check.cpp.
#pragma once
#include <cstring>

namespace er {

enum ExtendRoute { EXTEND_ROWS = 0, EXTEND_FLASH = 1 };

// The rows route (one 128-key chunk in registers, the new queries walked over it) costs VALU time per (query, chunk) and reads the cache
// once; the flash route tiles 32 queries per wave and pays its tile whether 2 or 32 of them exist.  Measured at past_len 2048 in both
// modes at B = 1 and B = 32 (profiles/prefill_extend_bench.json, the route table, n_new = 2 .. 128): the last measured n_new at which the
// rows route still wins in every one of the four columns.  The column that decides is B = 32 (n_new = 16: 18.8 vs 16.7 ms exact, 17.6 vs
// 14.8 ms fast - the walk's VALU time grows with rows x queries); a single row keeps winning up to n_new = 64 in both modes (exact: 9.9
// vs 13.7 ms), which a rule on rows x queries would keep - one constant for now.
constexpr int EXTEND_ROWS_MAX_NEW = 8;

// env: the value of ER_EXTEND_ATTN (null or empty: the measured rule; "rows" / "flash": that route wherever it can run - the A/B switch
// of scripts/bench_prefill_extend.py and the tests).  rows_supported: the rows kernels have this (head_dim, cache type).
inline ExtendRoute extend_attn_route(int n_new, bool rows_supported, const char* env) {
    if (!rows_supported) return EXTEND_FLASH;
    if (env && !strcmp(env, "rows")) return n_new <= 65535 ? EXTEND_ROWS : EXTEND_FLASH;     // the merge launch's grid holds n_new
    if (env && !strcmp(env, "flash")) return EXTEND_FLASH;
    return n_new <= EXTEND_ROWS_MAX_NEW ? EXTEND_ROWS : EXTEND_FLASH;
}

// The prefix a call may keep: valid = positions [0, valid) that the last full or extending pass on this reservation wrote for ALL rows
// (0: none), prefix_len = what prefix groups share (0: none).  0 = fine, 1 = past_len outside [1, valid], 2 = below the groups' prefix.
inline int extend_past_check(int past_len, int valid, int prefix_len) {
    if (past_len < 1 || past_len > valid) return 1;
    if (prefix_len > 0 && past_len < prefix_len) return 2;
    return 0;
}

}  // namespace er
