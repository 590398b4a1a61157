// Checkpoint weights of a context (er_ctx, er_dit_ctx): every state_dict key is registered once, with where and how it is
// stored, and one loader serves them all.  The table owns every block it allocates.  Included by er_api.hip after er_devbuf.h.
#pragma once

struct WeightEntry {
    float** dst = nullptr;        // the fp32 block
    size_t n = 0;                 // elements of the checkpoint tensor
    size_t total = 0, off = 0;    // elements of the block; the tensor lands at [off, ...)
    size_t cols = 0, pitch = 0;   // rows of `cols` values stored `pitch` apart (pitch > cols: zero-padded rows)
    bool f16 = false;             // fp16 mode: keep an fp16 copy (WeightTable::half_of); the fp32 block holds the same rounded values
    _Float16** dst16 = nullptr;   // ... and publish it here too (nullable)
    bool q8 = false;              // fp8 mode: quantised by row (er_w8.h) - a byte block [rows][cols] e4m3 + [rows] 2^e (WeightTable::q8_of,
    unsigned char** dstq = nullptr;   // k_gemv.h w8_scales), published here; the fp16 copy and the fp32 block then hold the dequantised values
    size_t qcols = 0;             // ... values per quantised row
    bool q4 = false;              // fp4 mode: quantised by blocks of 32 along a row (er_w4.h) - the canonical block [rows][cols / 2] nibble bytes +
    unsigned char** dstq4 = nullptr;  // [rows][cols / 32] e8m0 bytes (WeightTable::q4_of), published here; the fp16 copy and the fp32 block hold the dequantised values
    bool loaded = false;

    // [off, off + n) of a fused block of `total` elements (q / k / v of one layer)
    WeightEntry& slice(size_t total_, size_t off_) { total = total_; off = off_; return *this; }
    // rows of kin values stored zero-padded to kpad columns, so that a GEMM's K is a whole number of tiles
    WeightEntry& pad(size_t kin, size_t kpad) { cols = kin; pitch = kpad; total = n / kin * kpad; return *this; }
    WeightEntry& half(_Float16** p = nullptr) { f16 = true; dst16 = p; return *this; }
    WeightEntry& rows8(unsigned char** q, size_t in) { q8 = true; dstq = q; qcols = in; return *this; }      // rows of `in` values ([out][in])
    WeightEntry& blocks4(unsigned char** q, size_t in) { q4 = true; dstq4 = q; qcols = in; return *this; }   // ... the same rows, for fp4 mode
};

struct WeightTable {
    std::map<std::string, WeightEntry> keys;
    std::map<const float*, _Float16*> half_of;   // fp32 block -> its fp16 copy (fp16 mode, entries with half())
    std::vector<DevBuf<char>> owned;             // every weight block (derived copies included); the entries and weight structs hold views
    std::map<const float*, unsigned char*> q8_of;   // fp32 block -> its byte block (fp8 mode, entries with rows8())
    std::map<const float*, unsigned char*> q4_of;   // fp32 block -> its canonical MXFP4 block (fp4 mode, entries with blocks4())
    DevBuf<char> stage;                          // upload of one host tensor: grow-only, freed by weights_finalize
    DevBuf<int> bad;                             // fp8 / fp4 mode: the quantiser's "non-finite source value" flag
    bool fp16 = false;
    bool w8 = false;                             // fp8 mode (implies fp16: every other tensor is stored as fast mode stores it)
    bool w4 = false;                             // fp4 mode (implies fp16 in the same way)

    // a block of n T that lives as long as the table
    template <typename T>
    int alloc(T** p, size_t n) {
        DevBuf<char> b;
        ERCHK(b.ensure(n * sizeof(T)));
        *p = reinterpret_cast<T*>(b.p);
        owned.push_back(std::move(b));
        return 0;
    }

    // a block of its own; (re)registering a key resets it to "not loaded"
    WeightEntry& add(const std::string& key, float** dst, size_t n) {
        WeightEntry& e = keys[key] = WeightEntry{};
        e.dst = dst; e.n = e.total = e.cols = e.pitch = n;
        return e;
    }
    // name.weight [out][in] and name.bias [out] (in = 1: a LayerNorm's two vectors); returns the weight's entry
    WeightEntry& lin(const std::string& name, float** w, float** b, size_t out, size_t in) {
        add(name + ".bias", b, out);
        return add(name + ".weight", w, out * in);
    }
};

// fp32 / fp16 / bf16 source element i as fp32 (exact)
__device__ __forceinline__ float raw_to_f32(const void* src, int dtype, size_t i) {
    if (dtype == ER_F32) return reinterpret_cast<const float*>(src)[i];
    if (dtype == ER_F16) return (float)reinterpret_cast<const _Float16*>(src)[i];
    const unsigned int u = (unsigned int)reinterpret_cast<const unsigned short*>(src)[i] << 16;      // bf16
    return __uint_as_float(u);
}
// n source elements into rows of `cols` values `pitch` apart; with dst16, the fp16 copy (round to nearest even) and fp32 values
// that are the same rounded numbers
__global__ void cvt_weights_kernel(const void* src, int dtype, float* dst32, _Float16* dst16, size_t n, size_t cols, size_t pitch) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t d = cols == pitch ? i : i / cols * pitch + i % cols;
        float v = raw_to_f32(src, dtype, i);
        if (dst16) {
            const _Float16 hv = (_Float16)v;
            dst16[d] = hv;
            v = (float)hv;
        }
        dst32[d] = v;
    }
}

// Row-wise e4m3 quantiser (er_w8.h): one workgroup per row of `cols` source values.  Row maximum -> exponent e -> bytes q, wscale = 2^e,
// and the dequantised values q * 2^e as fp16 and fp32 (both exact).  Every output pointer is nullable; eout takes e itself.  A NaN or
// an infinity anywhere in the source raises *bad (the row's outputs are then meaningless).  Rows are independent, so the three slices
// of a fused q / k / v block are quantised by three calls on their own row ranges.
__global__ __launch_bounds__(ER_WG) void quant_rows_kernel(const void* src, int dtype, size_t cols, float* dst32, _Float16* dst16,
                                                          unsigned char* q, float* wscale, int* eout, int* bad) {
    __shared__ float red[ER_NWAVES];
    const size_t base = (size_t)blockIdx.x * cols;
    const int tid = threadIdx.x;
    float amax = 0.f;
    bool finite = true;
    for (size_t k = tid; k < cols; k += ER_WG) {
        const float a = fabsf(raw_to_f32(src, dtype, base + k));
        finite = finite && a <= 3.402823466e38f;      // false for NaN and infinity
        amax = fmaxf(amax, a);
    }
    if (!finite) *bad = 1;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const int e = w8_row_exponent(amax);
    const float up = w8_pow2(e), down = w8_pow2(-e);      // both exact powers of two
    if (tid == 0) {
        if (wscale) wscale[blockIdx.x] = up;
        if (eout) eout[blockIdx.x] = e;
    }
    for (size_t k = tid; k < cols; k += ER_WG) {
        const unsigned char c = w8_encode(raw_to_f32(src, dtype, base + k) * down);
        const float v = w8_decode(c) * up;
        if (q) q[base + k] = c;
        if (dst16) dst16[base + k] = (_Float16)v;
        if (dst32) dst32[base + k] = v;
    }
}

// Block-wise MXFP4 quantiser (er_w4.h): one workgroup per row of `cols` source values (a multiple of 32), four consecutive lanes per
// block of 32 - a lane holds 8 consecutive elements, i.e. 4 nibble bytes.  Block maximum -> exponent e -> e2m1 codes, the e8m0 byte
// e + 127, and the dequantised values q * 2^e as fp16 and fp32 (both exact).  Every output pointer is nullable; eout takes e itself
// ([rows][cols / 32]).  A NaN or an infinity anywhere in the source raises *bad.  Rows are independent (quant_rows_kernel's remark).
__global__ __launch_bounds__(ER_WG) void quant_blocks_kernel(const void* src, int dtype, size_t cols, float* dst32, _Float16* dst16,
                                                            unsigned char* nib, unsigned char* scale, int* eout, int* bad) {
    const size_t row = blockIdx.x, base = row * cols;
    bool finite = true;
    for (size_t g = threadIdx.x; g < cols / 8; g += ER_WG) {      // cols / 8 is a multiple of 4: the four lanes of a block run together
        float v[8], amax = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = raw_to_f32(src, dtype, base + g * 8 + i);
            const float a = fabsf(v[i]);
            finite = finite && a <= 3.402823466e38f;      // false for NaN and infinity
            amax = fmaxf(amax, a);
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        const int e = w4_block_exponent(amax);
        const float up = w4_pow2(e), down = w4_pow2(-e);      // both exact powers of two
        if ((g & 3) == 0) {
            const size_t blk = row * (cols / W4_BLOCK) + g / 4;
            if (scale) scale[blk] = w4_scale_byte(e);
            if (eout) eout[blk] = e;
        }
        unsigned int packed = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned char c = w4_encode(v[i] * down);
            const float d = w4_decode(c) * up;
            packed |= (unsigned int)c << (4 * i);      // element 2 b in the low nibble of byte b
            if (dst16) dst16[base + g * 8 + i] = (_Float16)d;
            if (dst32) dst32[base + g * 8 + i] = d;
        }
        if (nib) reinterpret_cast<unsigned int*>(nib)[(base + g * 8) / 8] = packed;
    }
    if (!finite) *bad = 1;
}

// The canonical block of a matrix [n][k] (nibble bytes, then scale bytes) into the copy the nibble kernels stream (er_w4_map.h): one
// thread per nibble byte and per scale byte.  n a multiple of 4, k of 1536.
__global__ __launch_bounds__(ER_WG) void w4_interleave_kernel(const unsigned char* canon, unsigned char* stream, long long n, int k) {
    const long long nb = n * k / 2, ns = n * k / W4_BLOCK;
    const unsigned char* scales = canon + nb;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nb + ns; i += (long long)gridDim.x * blockDim.x) {
        if (i < nb) {
            const long long row = i / (k / 2), kk = (i - row * (k / 2)) * 2;      // the byte's even element
            stream[w4map::byte_offset(w4map::where(row, kk), k)] = canon[i];
        } else {
            const long long b = i - nb, row = b / (k / W4_BLOCK), kk = (b - row * (k / W4_BLOCK)) * W4_BLOCK;
            stream[w4map::scale_offset(w4map::where(row, kk), k)] = scales[b];
        }
    }
}

// The canonical block of a matrix [n][k] into the tiled copy the matrix-core batched forms stream (er_w4_tile_map.h): one thread per
// dword of the copy - a lane's piece (eight consecutive elements of one row: one aligned dword of the canonical nibbles), or the three
// scales of a row's blocks 3 s .. 3 s + 2 and the padding byte.  Rows n .. rows(n) - 1 are the padding: zero nibbles, scale byte 127.
// k a multiple of 96.
__global__ __launch_bounds__(ER_WG) void w4_tile_kernel(const unsigned char* canon, unsigned int* tiled, long long n, int k) {
    const long long total = w4t::block_bytes(n, k) / 4;
    const unsigned char* scales = canon + n * k / 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const w4t::What w = w4t::what(k, i * 4);
        unsigned int v = 0;
        if (w.kind == w4t::WEIGHT) {
            if (w.n < n) v = *reinterpret_cast<const unsigned int*>(canon + (w.n * k + w.k) / 2);
        } else {      // the dword starts at a row's first scale of the unit: blocks w.k .. w.k + 2, then the padding byte
            const unsigned char* s = scales + w.n * (k / W4_BLOCK) + w.k;
            v = w.n < n ? (unsigned int)s[0] | (unsigned int)s[1] << 8 | (unsigned int)s[2] << 16
                        : (unsigned int)w4t::PAD_SCALE * 0x010101u;
        }
        tiled[i] = v;
    }
}

template <typename T>
static int weights_alloc(WeightTable& t, T** p, size_t n) {   // once per block, zeroed
    if (*p) return 0;
    ERCHK(t.alloc(p, n));
    HIPCHK(hipMemset(*p, 0, n * sizeof(T)));
    return 0;
}

// One checkpoint tensor (fp32 / fp16 / bf16, host or device memory) into its block, converted on the device.  Returns 1 for a key the
// table does not hold; the copy is complete when this returns (the caller's buffer and the staging block may be reused).
static int weights_load(WeightTable& t, hipStream_t st, const char* who, const std::string& key, const void* data, int dtype,
                        int ndim, const int64_t* shape, int on_device) {
    if (!data || !shape || ndim < 1 || ndim > 4) return fail(ER_ERR_INVALID, "%s: bad argument", who);
    if (dtype != ER_F32 && dtype != ER_F16 && dtype != ER_BF16) return fail(ER_ERR_INVALID, "%s: dtype %d", who, dtype);
    auto it = t.keys.find(key);
    if (it == t.keys.end()) return 1;     // strict=False: unknown keys are ignored
    WeightEntry& e = it->second;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    if (n != e.n) return fail(ER_ERR_INVALID, "%s(%s): %zu elements, expected %zu", who, key.c_str(), n, e.n);
    const void* src = data;
    if (!on_device) {
        const size_t bytes = n * (dtype == ER_F32 ? 4 : 2);
        ERCHK(t.stage.ensure((bytes + 3) / 4 * 4));      // whole 32-bit words
        HIPCHK(hipMemcpy(t.stage.p, data, bytes, hipMemcpyHostToDevice));
        src = t.stage.p;
    }
    ERCHK(weights_alloc(t, e.dst, e.total));
    _Float16* h = nullptr;
    if (t.fp16 && e.f16) {
        _Float16*& hb = t.half_of[*e.dst];
        ERCHK(weights_alloc(t, &hb, e.total));
        if (e.dst16) *e.dst16 = hb;
        h = hb + e.off;
    }
    if (t.w8 && e.q8) {      // rows of e.cols values, unpadded: bytes + row scales, the fp16 and fp32 blocks get the dequantised values
        const size_t qc = e.qcols;
        if (!h || e.cols != e.pitch || !qc || e.n % qc || e.off % qc || e.total % qc) return fail(ER_ERR_INVALID, "%s(%s): not a row-quantised matrix", who, key.c_str());
        unsigned char*& qb = t.q8_of[*e.dst];
        const size_t rows = e.total / qc;
        ERCHK(weights_alloc(t, &qb, w8_block_bytes(rows, qc)));
        if (e.dstq) *e.dstq = qb;
        float* wscale = const_cast<float*>(w8_scales(qb, (long long)rows, (long long)qc));
        ERCHK(t.bad.ensure(1));
        e.loaded = false;                 // until the new values are known to be finite: a refused reload leaves the key unloaded
        HIPCHK(hipMemsetAsync(t.bad.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(quant_rows_kernel, dim3((unsigned)(e.n / qc)), dim3(ER_WG), 0, st, src, dtype, qc, *e.dst + e.off, h, qb + e.off,
                           wscale + e.off / qc, (int*)nullptr, t.bad.p);
        HIPCHK(hipGetLastError());
        int bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, t.bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (bad) return fail(ER_ERR_INVALID, "%s(%s): the tensor holds a NaN or an infinity; fp8 rows are quantised from finite values only", who, key.c_str());
        e.loaded = true;
        return 0;
    }
    if (t.w4 && e.q4) {      // rows of e.qcols values: the canonical MXFP4 block, the fp16 and fp32 blocks get the dequantised values
        const size_t qc = e.qcols;
        if (!h || e.cols != e.pitch || !qc || qc % W4_BLOCK || e.n % qc || e.off % qc || e.total % qc) return fail(ER_ERR_INVALID, "%s(%s): not a block-quantised matrix", who, key.c_str());
        unsigned char*& qb = t.q4_of[*e.dst];
        const size_t rows = e.total / qc;
        ERCHK(weights_alloc(t, &qb, w4_block_bytes(rows, qc)));
        if (e.dstq4) *e.dstq4 = qb;
        unsigned char* scales = const_cast<unsigned char*>(w4_scales(qb, rows, qc));
        ERCHK(t.bad.ensure(1));
        e.loaded = false;                 // until the new values are known to be finite: a refused reload leaves the key unloaded
        HIPCHK(hipMemsetAsync(t.bad.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(quant_blocks_kernel, dim3((unsigned)(e.n / qc)), dim3(ER_WG), 0, st, src, dtype, qc, *e.dst + e.off, h, qb + e.off / 2,
                           scales + e.off / W4_BLOCK, (int*)nullptr, t.bad.p);
        HIPCHK(hipGetLastError());
        int bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, t.bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (bad) return fail(ER_ERR_INVALID, "%s(%s): the tensor holds a NaN or an infinity; fp4 blocks are quantised from finite values only", who, key.c_str());
        e.loaded = true;
        return 0;
    }
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(cvt_weights_kernel, dim3(grid), dim3(256), 0, st, src, dtype, *e.dst + e.off, h, n, e.cols, e.pitch);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    e.loaded = true;
    return 0;
}

// the first registered key that was never loaded, or null
static const char* weights_missing(const WeightTable& t) {
    for (auto& kv : t.keys)
        if (!kv.second.loaded) return kv.first.c_str();
    return nullptr;
}

static int weights_finalize(WeightTable& t) {
    if (const char* k = weights_missing(t)) return fail(ER_ERR_MISSING, "tensor '%s' was never loaded", k);
    t.stage.reset();                      // checkpoint complete: the upload staging block (up to one tensor) is not needed any more
    return 0;
}
