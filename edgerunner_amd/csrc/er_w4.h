// Block-scaled 4-bit weight storage (fp4 mode): OCP MXFP4 - e2m1 elements, one e8m0 scale byte per block of 32 consecutive K-elements of
// one output row.
//   element  sign | 2 exponent bits | 1 mantissa bit: magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}; no infinity, no NaN
//   packing  two elements per byte, element 2 i in the LOW nibble of byte i, element 2 i + 1 in the high nibble - the order in which
//            v_cvt_scalef32_pk_f32_fp4 hands out the two numbers of the byte its byte select names
//   e[blk]   = the smallest integer with amax(block) * 2^-e <= 6, clamped to [-15, 7]; a zero block gets -15.  Stored as the e8m0 byte
//            e + 127.  (NOT the exponent the OCP document suggests, floor(log2 amax) - 2, which clips values between 6 and 8 times the
//            scale; any e8m0 byte is a valid MX scale, so the data stays MXFP4.)
//   q        = e2m1(clamp(w * 2^-e, +-6)), round to nearest, ties to the even code; the sign of a zero is kept
//   value    = q * 2^e: at most 6 * 2^7 = 768, in steps of at least 0.5 * 2^-15 = 2^-16 - every one an fp16 number; the fp32 image of the
//            scale is the normal number (byte << 23)
// Encode, decode and the exponent rule in integer arithmetic on the fp32 bits (er_w8.h is the precedent): the device quantiser
// (er_weights.h) encodes with w4_encode, the decode kernels (k_gemv.h) read the nibbles with the hardware's scaled packed conversion,
// and tests/host/w4_check.cpp enumerates this file on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ER_W4_FN __host__ __device__ __forceinline__
#else
#define ER_W4_FN inline
#endif

namespace er {

constexpr int W4_E_MIN = -15, W4_E_MAX = 7;
constexpr int W4_BLOCK = 32;          // elements that share a scale
constexpr float W4_MAX = 6.0f;        // code 7: the largest e2m1 magnitude

ER_W4_FN uint32_t w4_f32_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
ER_W4_FN float w4_bits_f32(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }

// 2^e as fp32, e in [-126, 127]; the e8m0 byte of e and the fp32 image of a scale byte
ER_W4_FN float w4_pow2(int e) { return w4_bits_f32((uint32_t)(e + 127) << 23); }
ER_W4_FN uint8_t w4_scale_byte(int e) { return (uint8_t)(e + 127); }
ER_W4_FN float w4_scale_f32(uint8_t byte) { return w4_bits_f32((uint32_t)byte << 23); }

// The block exponent from the bits of amax (finite, >= 0): amax = 1.m * 2^E and 6 = 1.5 * 2^2, so e = E - 2, one more when 1.m > 1.5.
ER_W4_FN int w4_block_exponent(float amax) {
    const uint32_t u = w4_f32_bits(amax) & 0x7fffffffu;
    if (u == 0) return W4_E_MIN;
    const int E = (int)(u >> 23) - 127;      // an fp32 subnormal reads as 2^-127: far below the clamp
    const int e = E - 2 + ((u & 0x7fffffu) > 0x400000u ? 1 : 0);
    return e < W4_E_MIN ? W4_E_MIN : e > W4_E_MAX ? W4_E_MAX : e;
}

// fp32 -> e2m1 code (4 bits): the magnitude code is the number of rounding boundaries at or below |v|.  Non-negative fp32 numbers order
// like their bits; a boundary is the midpoint of two neighbouring magnitudes and belongs to the neighbour with the EVEN code (ties to
// even), so the boundaries below an even code are exclusive (>) and those below an odd code inclusive (>=).  Magnitudes above 6
// (infinity included) saturate to 6; NaN never gets here (the loader refuses non-finite sources) and would give 6.
ER_W4_FN uint8_t w4_encode(float v) {
    const uint32_t u = w4_f32_bits(v), a = u & 0x7fffffffu;
    const uint32_t c = (a > 0x3e800000u ? 1u : 0u)       // 0.25: 0 | 0.5, the tie goes to 0
                     + (a >= 0x3f400000u ? 1u : 0u)      // 0.75: 0.5 | 1, the tie goes to 1 (code 2)
                     + (a > 0x3fa00000u ? 1u : 0u)       // 1.25: 1 | 1.5, the tie goes to 1
                     + (a >= 0x3fe00000u ? 1u : 0u)      // 1.75: 1.5 | 2, the tie goes to 2 (code 4)
                     + (a > 0x40200000u ? 1u : 0u)       // 2.5: 2 | 3, the tie goes to 2
                     + (a >= 0x40600000u ? 1u : 0u)      // 3.5: 3 | 4, the tie goes to 4 (code 6)
                     + (a > 0x40a00000u ? 1u : 0u);      // 5: 4 | 6, the tie goes to 4
    return (uint8_t)(((u >> 28) & 8u) | c);
}

// e2m1 code -> fp32 (exact): all 16 codes are numbers
ER_W4_FN float w4_decode(uint8_t c) {
    const uint32_t sign = (uint32_t)(c & 8u) << 28, m = c & 7u;
    if (m == 0) return w4_bits_f32(sign);
    if (m == 1) return w4_bits_f32(sign | 0x3f000000u);                              // 0.5, the one subnormal
    return w4_bits_f32(sign | (((m >> 1) + 126u) << 23) | ((m & 1u) << 22));
}

// two codes in a byte and back: element 2 i low, 2 i + 1 high
ER_W4_FN uint8_t w4_pack(uint8_t even, uint8_t odd) { return (uint8_t)((even & 15u) | (odd << 4)); }
ER_W4_FN uint8_t w4_nibble(uint8_t byte, int k) { return (uint8_t)((k & 1) ? byte >> 4 : byte & 15u); }

// The canonical block of a matrix [N][K] (K a multiple of 32): N * K / 2 nibble bytes row-major, then N * K / 32 scale bytes row-major.
ER_W4_FN size_t w4_nibble_bytes(size_t n, size_t k) { return n * k / 2; }
ER_W4_FN size_t w4_scale_bytes(size_t n, size_t k) { return n * k / W4_BLOCK; }
ER_W4_FN size_t w4_block_bytes(size_t n, size_t k) { return w4_nibble_bytes(n, k) + w4_scale_bytes(n, k); }
ER_W4_FN const uint8_t* w4_scales(const void* blk, size_t n, size_t k) { return reinterpret_cast<const uint8_t*>(blk) + w4_nibble_bytes(n, k); }

}   // namespace er
