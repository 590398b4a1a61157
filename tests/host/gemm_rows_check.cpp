// Stand-alone check of the GEMM epilogues' row -> batch arithmetic (edgerunner_amd/csrc/er_gemm_rows.h): RowBatch with its compare and
// division forms, and the gate-row pair / residual rows of a wave that forms addresses before it knows which of its rows exist - also
// a wave wholly beyond M.  No device call: build with the host sanitizers and run,
//     c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o gemm_rows_check tests/host/gemm_rows_check.cpp
// (tests/test_gemm_rows_cpu.py does).  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../edgerunner_amd/csrc/er_gemm_rows.h"

static int g_span, g_period, g_M, g_mw, g_gm;
#define CHECK(cond)                                                                                                       \
    do {                                                                                                                  \
        if (!(cond)) {                                                                                                    \
            fprintf(stderr, "%s:%d: CHECK(%s) failed at span=%d period=%d M=%d mw=%d gm=%d\n", __FILE__, __LINE__, #cond, \
                    g_span, g_period, g_M, g_mw, g_gm);                                                                   \
            exit(1);                                                                                                      \
        }                                                                                                                 \
    } while (0)

using namespace er;

int main() {
    long long waves = 0, past = 0;
    for (int span : {32, 64})                      // rows per wave: 32 (64-row tiles, the streamed form's halves), 64 (128- and 256-row tiles)
        for (int period = 1; period <= 300; ++period)
            for (int M = 1; M <= 600; ++M) {
                const int nb = (M + period - 1) / period;      // batches = rows of the gate table
                const int mend = (M + 255) / 256 * 256;        // the largest row tile is 256
                for (int mw = 0; mw < mend; mw += 32) {
                    g_span = span; g_period = period; g_M = M; g_mw = mw; g_gm = -1;
                    ++waves;
                    // hh_epi_rows / gs_load_pre: the wave's map and its gate pair
                    const RowBatch wb = wave_row_batch(mw, M, period, span);
                    const GatePair gp = gate_row_pair(wb, mw, M, span);
                    CHECK(gp.gb0 >= 0 && gp.gb0 < nb);
                    CHECK(gp.gb1 >= 0 && gp.gb1 < nb);
                    // the fast flag: only when the span crosses at most one boundary (from any start row)
                    if (wb.fast) CHECK((mw + span - 1) / period - mw / period <= 1);
                    if (mw >= M) ++past;
                    // gemm_epilogue: the plain map of a 32-row block, rows checked before any address is formed
                    const RowBatch eb(mw, period);
                    if (eb.fast) CHECK((mw + 31) / period - mw / period <= 1);
                    for (int gm = mw; gm < mw + span; ++gm) {
                        g_gm = gm;
                        if (gm < M) {
                            CHECK(wb.batch(gm) == gm / period);
                            CHECK(wb.inner(gm) == gm % period);
                            if (wb.fast) CHECK(wb.batch(gm) == gp.gb0 || wb.batch(gm) == gp.gb1);
                            if (gm < mw + 32) {
                                CHECK(eb.batch(gm) == gm / period);
                                CHECK(eb.inner(gm) == gm % period);
                            }
                        }
                        // the residual row a wave pre-fetches for a pass (hh_epi_rows, 32-row blocks): the row clamped to M - 1
                        const int cm = gm < M ? gm : M - 1, r = wb.inner(cm);
                        CHECK(r >= 0 && r < period && r <= M - 1);
                        if (mw < M) CHECK(r == cm % period);
                    }
                }
            }
    CHECK(past > 0);
    printf("gemm_rows_check: ok (%lld waves, %lld wholly beyond M)\n", waves, past);
    return 0;
}
