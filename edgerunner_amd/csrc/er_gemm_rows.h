// Row -> batch arithmetic of the GEMM epilogues (k_gemm.h gemm_epilogue / hh_epi_rows, k_gemm_stream.h gs_load_pre): which adaLN gate
// row, which row of a shared residual table, which cache row a matrix row m belongs to, without a division per element.
// Pure C++ with no device call (er_mlp_map.h is the precedent): the kernels include it, and tests/host/gemm_rows_check.cpp enumerates
// it against m / period and m % period on the host.
//
// The one rule every caller keeps: a row index that forms a gate or residual ADDRESS is <= M - 1, also in a wave whose rows lie wholly
// beyond M (the ragged last tile: 128 x 128 tile, M = 192, wave at row 192).  Such a wave stores nothing, but it requests its operands
// before it looks at a row, so an unclamped index reads behind (gate row = number of batches) or in front of (residual row -1) the table.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ER_ROWS_FN __host__ __device__ __forceinline__
#else
#define ER_ROWS_FN inline
#endif

namespace er {

struct RowBatch {          // batch index (row / period) and row inside the batch for the rows [row0, row0 + span) (span 32: one MFMA block)
    int q0, next, period;
    bool fast;             // period >= span: the rows cross at most one batch boundary, batch() is a compare
    ER_ROWS_FN RowBatch(int row0, int period_, int span = 32) : period(period_) {
        fast = period_ >= span;
        q0 = period_ > 0 ? row0 / period_ : 0;
        next = (q0 + 1) * period_;
    }
    // for the rows gm >= row0 of the span (the fast form knows nothing about rows in front of row0)
    ER_ROWS_FN int batch(int gm) const { return fast ? q0 + (gm >= next ? 1 : 0) : gm / period; }
    ER_ROWS_FN int inner(int gm) const { return gm - batch(gm) * period; }
};

// The map of a wave that owns the rows [mw, mw + span) of an M-row product and forms addresses BEFORE it knows which of its rows exist:
// anchored at min(mw, M - 1), so that batch() / inner() of any row clamped to M - 1 stay inside the tables.  For mw < M it is RowBatch(mw, ..).
ER_ROWS_FN RowBatch wave_row_batch(int mw, int M, int period, int span) { return RowBatch(mw < M ? mw : M - 1, period, span); }

// The gate rows of the two batches the existing rows of such a wave can lie in (gb = wave_row_batch(mw, M, gate_rows, span)): every row
// gm < M of a fast wave is in batch gb0 or gb1, and both are < ceil(M / gate_rows) whatever mw is.
struct GatePair { int gb0, gb1; };
ER_ROWS_FN GatePair gate_row_pair(const RowBatch& gb, int mw, int M, int span) {
    const int last = mw + span - 1 < M ? mw + span - 1 : M - 1;
    return GatePair{gb.q0, gb.batch(last)};
}

}   // namespace er
