// Host enumeration of csrc/er_w4.h (e2m1 encode / decode, block exponent, canonical block): prints what the header computes for inputs
// it generates itself, and quantises a matrix read from a file; tests/test_w4_cpu.py compares every line with tests/w4_ref.py.  Built
// with ASan + UBSan.
//   D <code> <fp32 bits of w4_decode(code)>
//   E <fp32 bits of v> <w4_encode(v)>
//   X <fp32 bits of amax> <w4_block_exponent(amax)>
//   H <e> <code> <1 if w4_decode(code) * 2^e survives fp32 -> fp16 -> fp32>     (needs _Float16: printed where the compiler has it)
// w4_check <in.f32> <n> <k> <out.bin>: the canonical block of the fp32 matrix [n][k] in the file (nibble bytes, then scale bytes).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../edgerunner_amd/csrc/er_w4.h"

using namespace er;

static int quantize_file(const char* in, size_t n, size_t k, const char* out) {
    std::vector<float> w(n * k);
    FILE* f = std::fopen(in, "rb");
    if (!f || std::fread(w.data(), sizeof(float), n * k, f) != n * k) return 2;
    std::fclose(f);
    std::vector<uint8_t> blk(w4_block_bytes(n, k), 0);
    uint8_t* scales = blk.data() + w4_nibble_bytes(n, k);
    for (size_t r = 0; r < n; ++r)
        for (size_t b = 0; b < k / W4_BLOCK; ++b) {
            const float* v = &w[r * k + b * W4_BLOCK];
            float amax = 0.f;
            for (int i = 0; i < W4_BLOCK; ++i) amax = std::fmax(amax, std::fabs(v[i]));
            const int e = w4_block_exponent(amax);
            scales[r * (k / W4_BLOCK) + b] = w4_scale_byte(e);
            for (int i = 0; i < W4_BLOCK; i += 2)
                blk[(r * k + b * W4_BLOCK + i) / 2] = w4_pack(w4_encode(v[i] * w4_pow2(-e)), w4_encode(v[i + 1] * w4_pow2(-e)));
        }
    f = std::fopen(out, "wb");
    if (!f || std::fwrite(blk.data(), 1, blk.size(), f) != blk.size()) return 3;
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5) return quantize_file(argv[1], (size_t)std::atoll(argv[2]), (size_t)std::atoll(argv[3]), argv[4]);

    for (int c = 0; c < 16; ++c) std::printf("D %d %u\n", c, (unsigned)w4_f32_bits(w4_decode((uint8_t)c)));
    for (int c = 0; c < 16; ++c)      // encode and decode round-trip on all codes (-0 keeps its sign), pack and unpack
        for (int d = 0; d < 16; ++d) {
            const uint8_t b = w4_pack(w4_encode(w4_decode((uint8_t)c)), w4_encode(w4_decode((uint8_t)d)));
            if (w4_nibble(b, 0) != c || w4_nibble(b, 1) != d) { std::printf("round trip of (%d, %d) is wrong\n", c, d); return 1; }
        }

    std::vector<float> in;
    for (int c = 0; c < 7; ++c) {      // every magnitude, every midpoint between adjacent magnitudes (a tie) and both fp32 neighbours of each
        const float lo = w4_decode((uint8_t)c), hi = w4_decode((uint8_t)(c + 1)), mid = 0.5f * (lo + hi);
        for (float v : {lo, std::nextafterf(lo, -1.f), std::nextafterf(lo, 1e9f), mid, std::nextafterf(mid, 0.f), std::nextafterf(mid, 1e9f)}) {
            in.push_back(v); in.push_back(-v);
        }
    }
    for (float v : {6.f, std::nextafterf(6.f, 0.f), std::nextafterf(6.f, 1e9f), 7.f, 8.f, 1e6f, 3.0e38f, 0.f, 1e-30f, 1.1754944e-38f, 1e-41f, 1.4e-45f}) {
        in.push_back(v); in.push_back(-v);
    }
    for (float v : in) std::printf("E %u %d\n", (unsigned)w4_f32_bits(v), (int)w4_encode(v));

    std::printf("X %u %d\n", 0u, w4_block_exponent(0.f));
    for (int E = -30; E <= 12; ++E) {      // every binade at mantissas 1.0, 1.5 - ulp, 1.5, 1.5 + ulp, 2 - ulp
        const float one = std::ldexp(1.f, E), mid = std::ldexp(1.5f, E), two = std::ldexp(2.f, E);
        for (float v : {one, std::nextafterf(mid, 0.f), mid, std::nextafterf(mid, 1e30f), std::nextafterf(two, 0.f)})
            std::printf("X %u %d\n", (unsigned)w4_f32_bits(v), w4_block_exponent(v));
    }
    for (float v : {1e-41f, 1.4e-45f, 3.0e38f}) std::printf("X %u %d\n", (unsigned)w4_f32_bits(v), w4_block_exponent(v));

    for (int e = W4_E_MIN; e <= W4_E_MAX; ++e) {
        if (w4_pow2(e) != std::ldexp(1.f, e) || w4_scale_f32(w4_scale_byte(e)) != std::ldexp(1.f, e)) { std::printf("the scale of %d is wrong\n", e); return 1; }
#if defined(__FLT16_MANT_DIG__)
        for (int c = 0; c < 16; ++c) {
            const float v = w4_decode((uint8_t)c) * w4_pow2(e);
            std::printf("H %d %d %d\n", e, c, (float)(_Float16)v == v ? 1 : 0);
        }
#endif
    }
    std::printf("w4_check: ok\n");
    return 0;
}
