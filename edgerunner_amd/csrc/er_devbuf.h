// The one owner of device memory in the host layer: every hipMalloc / hipFree of er_api.hip, er_weights.h and er_dit.h happens here.
// A context declares its buffers as members and its destructor frees them; a temporary of a single-kernel entry point is a local and
// every return path frees it.  One hipMalloc per buffer: no pool, no caching.  Included by er_api.hip after fail / HIPCHK.
#pragma once

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;   // elements of T

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }

    void reset() {
        if (p) hipFree(p);
        p = nullptr;
        n = 0;
    }
    // grow-only: room for at least `want` elements; growing drops the old contents
    int ensure(size_t want) {
        if (n >= want) return 0;
        reset();
        HIPCHK(hipMalloc((void**)&p, want * sizeof(T)));
        n = want;
        return 0;
    }
};

// fp16 GEMM / attention operands carry 16 spare elements (32 bytes) behind their last row.  Whether an LDS-DMA or 16-byte vector load
// of the last tile relies on them has not been established, so they stay.
constexpr size_t F16_TAIL = 16;
