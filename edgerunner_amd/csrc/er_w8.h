// The two 8-bit storage modes, both OCP e4m3fn.  kv8 mode (KV cache): one byte per element and NO scale - kv8_encode below; the
// post-LN decoder's K/V are O(1), e4m3's own exponent covers 2^-9 .. 448, and a power-of-two row scale would add no relative precision
// inside that range.
// Row-scaled 8-bit weight storage (fp8 mode): OCP e4m3fn bytes times a power of two per output row.
//   e[n]    = the smallest integer with amax(row n) * 2^-e <= 448, clamped to [-15, 7]; a zero row gets -15
//   q[n][k] = e4m3fn(clamp(w * 2^-e, +-448)), round to nearest even; the NaN bytes 0x7F / 0xFF are never produced
//   value   = q * 2^e: at most 448 * 2^7, in steps of at least 2^-9 * 2^-15 = 2^-24 - every one an fp16 number
// Encode, decode and the exponent rule in integer arithmetic on the fp32 bits: no conversion instruction, no rounding mode, no
// libm call.  The device quantiser (er_weights.h) encodes with w8_encode; the decode kernels (k_gemv.h, k_outproj_merge.h) read the
// bytes with the hardware's packed conversion, and tests/host/w8_check.cpp enumerates this file on the host (er_gemm_map.h is the
// precedent).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ER_W8_FN __host__ __device__ __forceinline__
#else
#define ER_W8_FN inline
#endif

namespace er {

constexpr int W8_E_MIN = -15, W8_E_MAX = 7;
constexpr float W8_MAX = 448.0f;      // 0x7E: the largest e4m3fn magnitude

ER_W8_FN uint32_t w8_f32_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
ER_W8_FN float w8_bits_f32(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }

// 2^e as fp32, e in [-126, 127]
ER_W8_FN float w8_pow2(int e) { return w8_bits_f32((uint32_t)(e + 127) << 23); }

// The row exponent from the bits of amax (finite, >= 0): amax = 1.m * 2^E and 448 = 1.75 * 2^8, so e = E - 8, one more when 1.m > 1.75.
ER_W8_FN int w8_row_exponent(float amax) {
    const uint32_t u = w8_f32_bits(amax) & 0x7fffffffu;
    if (u == 0) return W8_E_MIN;
    const int E = (int)(u >> 23) - 127;      // an fp32 subnormal reads as 2^-127: far below the clamp
    const int e = E - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
    return e < W8_E_MIN ? W8_E_MIN : e > W8_E_MAX ? W8_E_MAX : e;
}

// fp32 -> e4m3fn byte: magnitudes above 448 (infinity included) saturate to 448, then round to nearest, ties to even.  The sign of a
// zero or of a value that rounds to zero is kept (0x80).  NaN never gets here (the loader refuses non-finite sources); it would give 0x7E.
ER_W8_FN uint8_t w8_encode(float v) {
    const uint32_t u = w8_f32_bits(v);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    uint32_t a = u & 0x7fffffffu;
    if (a > 0x43e00000u) a = 0x43e00000u;                          // 448.0f
    const int E = (int)(a >> 23) - 127;
    if (E >= -6) {                                                 // normal in e4m3: keep three mantissa bits
        const uint32_t r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;      // (biased exponent << 3 | mantissa), a carry moves up into the exponent
        return (uint8_t)(sign | (r - ((127u - 7u) << 3)));
    }
    // subnormal in e4m3: a whole number of 2^-9 steps, 0 .. 8 (8 is the smallest normal, code 0x08)
    const int s = 14 - E;                                          // the 24-bit significand m24 stands for m24 * 2^(E - 23) = m24 * 2^-9 * 2^-s
    if (s > 24 || (a >> 23) == 0) return sign;                     // below half a step
    const uint32_t m24 = (a & 0x7fffffu) | 0x800000u;
    uint32_t q = m24 >> s;
    const uint32_t rem = m24 & ((1u << s) - 1u), half = 1u << (s - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return (uint8_t)(sign | q);
}

// The KV cache's byte (kv8 mode: one e4m3fn byte per element, no scale): w8_encode, and a NaN keeps being one - 0x7F | sign - so that a
// poisoned activation still reaches the sampling head's NaN guard instead of reading back as 448.
ER_W8_FN uint8_t kv8_encode(float v) {
    const uint32_t u = w8_f32_bits(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint8_t)(((u >> 24) & 0x80u) | 0x7fu);
    return w8_encode(v);
}

// e4m3fn byte -> fp32 (exact); 0x7F / 0xFF are NaN
ER_W8_FN float w8_decode(uint8_t c) {
    const uint32_t sign = (uint32_t)(c & 0x80u) << 24, e4 = (c >> 3) & 15u, m = c & 7u;
    if ((c & 0x7fu) == 0x7fu) return w8_bits_f32(sign | 0x7fc00000u);
    if (e4 == 0) return w8_bits_f32(sign | w8_f32_bits((float)m * 0.001953125f));      // m * 2^-9
    return w8_bits_f32(sign | ((e4 + 120u) << 23) | (m << 20));
}

}   // namespace er
