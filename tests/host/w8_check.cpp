// Host enumeration of csrc/er_w8.h (e4m3fn encode / decode, row exponent): prints what the header computes for inputs it generates
// itself; tests/test_w8_cpu.py compares every line with torch's float8_e4m3fn cast and tests/w8_ref.py.  Built with ASan + UBSan.
//   D <code> <fp32 bits of w8_decode(code)>
//   E <fp32 bits of v> <w8_encode(v)>
//   X <fp32 bits of amax> <w8_row_exponent(amax)>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../edgerunner_amd/csrc/er_w8.h"

using namespace er;

int main() {
    for (int c = 0; c < 256; ++c) std::printf("D %d %u\n", c, (unsigned)w8_f32_bits(w8_decode((uint8_t)c)));

    std::vector<float> in;
    for (int c = 0; c < 0x7e; ++c) {      // every midpoint between adjacent magnitudes (a tie) and its two fp32 neighbours
        const float lo = w8_decode((uint8_t)c), hi = w8_decode((uint8_t)(c + 1)), mid = 0.5f * (lo + hi);
        for (float v : {lo, mid, std::nextafterf(mid, 0.f), std::nextafterf(mid, 1e9f)}) { in.push_back(v); in.push_back(-v); }
    }
    const float sub = w8_decode(1);       // 2^-9
    for (float v : {448.f, std::nextafterf(448.f, 1e9f), 464.f, 480.f, 1e6f, 3.0e38f, 0.f, sub, 0.5f * sub, std::nextafterf(0.5f * sub, 1.f),
                    std::nextafterf(0.5f * sub, 0.f), 0.25f * sub, 1e-30f, 1e-44f}) { in.push_back(v); in.push_back(-v); }
    for (float v : in) std::printf("E %u %d\n", (unsigned)w8_f32_bits(v), (int)w8_encode(v));

    std::printf("X %u %d\n", 0u, w8_row_exponent(0.f));
    for (int e = -16; e <= 8; ++e) {      // amax exactly on 448 * 2^e and one ulp above
        const float on = std::ldexp(448.f, e);
        std::printf("X %u %d\n", (unsigned)w8_f32_bits(on), w8_row_exponent(on));
        std::printf("X %u %d\n", (unsigned)w8_f32_bits(std::nextafterf(on, 1e30f)), w8_row_exponent(std::nextafterf(on, 1e30f)));
    }
    for (float v : {1e-30f, 1e-44f, 0.02f, 1.f, 3e4f, 1e6f, 3.0e38f}) std::printf("X %u %d\n", (unsigned)w8_f32_bits(v), w8_row_exponent(v));
    // 2^e round trip of the scale
    for (int e = W8_E_MIN; e <= W8_E_MAX; ++e)
        if (w8_pow2(e) != std::ldexp(1.f, e)) { std::printf("w8_pow2(%d) is wrong\n", e); return 1; }
    std::printf("w8_check: ok\n");
    return 0;
}
