// numfmt.h -- the scalar number formats of this library, each stated once: bit casts, the 16-bit activation types, the element formats
// e2m1 / e4m3 / e2m3, the E8M0 block scale, and the block-scale rule of the quantised activations ("petit-qact/1", layout.h).
// Plain C++ that is also device code (PETIT_HD, as layout.h): the kernels, their host twins and the stand-alone host programs
// (tools/invariant_hostcheck.cc) evaluate the same lines.  Where two callers need different answers for the same input the difference is a
// named variant with its reason, not a second copy.  The oracle and the tests' numpy statements stay independent of this file.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "layout.h" // PETIT_HD

namespace petit_amd {

PETIT_HD unsigned f32_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(unsigned, x);
#else
    unsigned u;
    memcpy(&u, &x, 4);
    return u;
#endif
}
PETIT_HD float bits_f32(unsigned u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, u);
#else
    float x;
    memcpy(&x, &u, 4);
    return x;
#endif
}

// ---- the 16-bit types (bf16, fp16) -----------------------------------------------------------------------------------------------------------

// a 16-bit element -> f32 (exact; bits above the 16 are not read for fp16 and must be clear for bf16)
template <bool BF16> PETIT_HD float h16_f32(unsigned h) {
    if constexpr (BF16)
        return bits_f32(h << 16);
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
#endif
    const unsigned sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 0)
        return bits_f32(sign | f32_bits((float)m * (1.0f / 16777216.0f))); // subnormals: m x 2^-24
    return bits_f32(sign | (e == 31 ? 0x7f800000u : (e + 112u) << 23) | (m << 13));
}
PETIT_HD float h16_f32(bool bf16, unsigned h) { return bf16 ? h16_f32<true>(h) : h16_f32<false>(h); }

// f32 -> the 16-bit element, round to nearest even.  bf16: the integer rule on EVERY pattern, a NaN included (RMSNorm's contract: "by the
// integer rule on both sides").  fp16: the hardware convert on the device and the same rule spelled out on the host -- overflow to infinity
// from 65520 up, subnormals as multiples of 2^-24, a NaN as the quiet 0x7e00.
template <bool BF16> PETIT_HD unsigned f32_h16(float x) {
    const unsigned u = f32_bits(x);
    if constexpr (BF16)
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)x);
#endif
    const unsigned sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u)
        return sign | 0x7e00u;
    if (a >= 0x477ff000u) // 65520 and above, infinity included
        return sign | 0x7c00u;
    if (a < 0x38800000u) // below 2^-14: a x 2^24 is exact and below 1024; the add rounds it to an integer (1024 = the pattern of 2^-14)
        return sign | (f32_bits(bits_f32(a) * 16777216.0f + 8388608.0f) & 0x7fffffu);
    const unsigned r = a - 0x38000000u;
    return sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);
}
// the variant that quietens a bf16 NaN (upper payload bits kept, bit 6 set) as the hardware's vector convert does, where the integer rule
// would carry a NaN with a full low half into infinity: the GEMM epilogues' and the MoE combine's rounding
template <bool BF16> PETIT_HD unsigned f32_h16_quiet_nan(float x) {
    if constexpr (BF16) {
        const unsigned u = f32_bits(x);
        if ((u & 0x7fffffffu) > 0x7f800000u)
            return (u >> 16) | 0x40u;
    }
    return f32_h16<BF16>(x);
}
PETIT_HD unsigned f32_h16_quiet_nan(bool bf16, float x) { return bf16 ? f32_h16_quiet_nan<true>(x) : f32_h16_quiet_nan<false>(x); }

// ---- e2m1 (FP4): sign, codes 0 .. 7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6 ---------------------------------------------------------------------------------

constexpr float kE2m1Mag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
// the midpoints between neighbouring magnitudes: code c is the number of midpoints below |x|, a tie going to the even code (midpoints 1, 3, 5
// count with <=, the others with <)
constexpr float kE2m1Mid[7] = {0.25f, 0.75f, 1.25f, 1.75f, 2.5f, 3.5f, 5.0f};

PETIT_HD float e2m1_f32(unsigned code) { return (code & 8u) ? -kE2m1Mag[code & 7u] : kE2m1Mag[code & 7u]; }
// round to nearest even of an exact quotient, saturating at 6; the sign is kept, on a zero too (the hardware convert's); host only
inline unsigned e2m1_rne(double x) {
    const unsigned sign = signbit(x) ? 8u : 0u;
    const double a = fabs(x);
    return sign | ((unsigned)(kE2m1Mid[0] < a) + (unsigned)(kE2m1Mid[1] <= a) + (unsigned)(kE2m1Mid[2] < a) + (unsigned)(kE2m1Mid[3] <= a) +
                   (unsigned)(kE2m1Mid[4] < a) + (unsigned)(kE2m1Mid[5] <= a) + (unsigned)(kE2m1Mid[6] < a));
}

// ---- e4m3 (OCP FP8 e4m3fn): no infinities, 0x7f / 0xff are NaN, subnormals 2^-9 .. 7 x 2^-9 ------------------------------------------------------

PETIT_HD bool e4m3_is_nan(unsigned b) { return (b & 0x7fu) == 0x7fu; }
// the magnitude from the exponent and mantissa fields (e = 15, m = 7, the NaN pattern, reads as 480: callers that can meet it ask e4m3_is_nan)
PETIT_HD float e4m3_fields_f32(unsigned e, unsigned m) {
    return e == 0 ? (float)m * (1.0f / 512.0f) : bits_f32(((e + 120u) << 23) | (m << 20));
}
// of a byte known to be below 0x7f (what e4m3_rne_sat returns): no mask on the device's path
PETIT_HD float e4m3_mag_f32(unsigned b7) { return e4m3_fields_f32(b7 >> 3, b7 & 7u); }
// sign and magnitude of any byte, no NaN test (nvnative.hip carries the NaN of a scale byte as a flag of its own)
PETIT_HD float e4m3_finite_f32(unsigned b) {
    const float v = e4m3_fields_f32((b >> 3) & 15u, b & 7u);
    return (b & 0x80u) ? -v : v;
}
PETIT_HD float e4m3_f32(unsigned b) {
    const float v = e4m3_is_nan(b) ? bits_f32(0x7fc00000u) : e4m3_fields_f32((b >> 3) & 15u, b & 7u);
    return (b & 0x80u) ? -v : v;
}
// f32 >= 0 -> the byte, round to nearest even, saturating at 448 (0x7e; a NaN saturates too).  Unsigned: the weight quantiser's block scales,
// on the device, where a sign would cost instructions for nothing
PETIT_HD unsigned e4m3_rne_sat(float x) {
    if (!(x < 448.0f))
        return 0x7eu;
    if (x < 0.015625f) // below 2^-6: multiples of 2^-9; x * 512 is exact, the add rounds it to an integer (8 = the byte of 2^-6)
        return f32_bits(x * 512.0f + 8388608.0f) & 15u;
    const unsigned u = f32_bits(x);
    return ((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - (120u << 3);
}
// any sign: the sign is kept, on a zero (and a NaN) too, as the hardware convert does -- the activation twins' elements
PETIT_HD unsigned e4m3_rne(float x) { return ((f32_bits(x) >> 24) & 0x80u) | e4m3_rne_sat(bits_f32(f32_bits(x) & 0x7fffffffu)); }

// ---- e2m3 (FP6): sign, 2 exponent bits (bias 1), 3 mantissa bits; subnormal step 1/8, normals 1 .. 7.5 -----------------------------------------

PETIT_HD float e2m3_f32(unsigned c) {
    const unsigned e = (c >> 3) & 3u, m = c & 7u;
    const float v = e == 0 ? (float)m * 0.125f : (1.0f + (float)m * 0.125f) * (float)(1u << (e - 1));
    return (c & 32u) ? -v : v;
}
// round to nearest even of an exact quotient, saturating at 7.5; the sign is kept, on a zero too (the hardware converts'); host only.  An f32
// argument widens exactly, so the one function serves the f32 products of nvnative.hip too (profiles/qact_single_definition.md)
inline unsigned e2m3_rne(double x) {
    const unsigned sign = signbit(x) ? 32u : 0u;
    const double ax = fabs(x);
    if (ax >= 7.5)
        return sign | 31u;
    if (ax < 1.0)
        return sign | (unsigned)nearbyint(ax * 8.0); // (8 = the code of 1.0)
    int e;
    (void)frexp(ax, &e);
    e -= 1; // floor(log2 ax): 0 .. 2
    unsigned r = (unsigned)nearbyint(ldexp(ax, 3 - e)); // 8 .. 16
    if (r == 16)
        r = 8, e += 1;
    return sign | ((unsigned)(e + 1) << 3) | (r - 8u);
}

// ---- e8m0: the block scale 2^(b - 127) ---------------------------------------------------------------------------------------------------------

// as the kernels decode it (the hardware convert): byte 0 is 2^-127, an fp32 subnormal -- NOT the 0.0 of `b << 23`, which is what dequant.hip
// and the oracle restate from the reference --, byte 255 is `b << 23` = inf, whose product with any code or activation ends as NaN
PETIT_HD float e8m0_f32(unsigned b) { return bits_f32((b & 0xffu) ? (b & 0xffu) << 23 : 0x00400000u); }
// the same as a double (exact for every byte)
PETIT_HD double e8m0_f64(unsigned b) { return (double)e8m0_f32(b); }

// The block-scale rule of the quantised activations: the E8M0 byte of 2^(E - emax_elem), E the exponent of the block maximum (OCP MX),
// emax_elem = 7 for e4m3 as the native kernels use it (the maximum lands in [128, 256) <= 448), 2 for e2m3 (in [4, 8), above 7.5 saturates)
// and e2m1 (above 6 saturates); a zero block: byte 127; never byte 0 or 255.
template <int ACT> PETIT_HD unsigned act_scale_byte(float amax) {
    constexpr unsigned kEmax = ACT == 8 ? 7u : 2u;
    const unsigned ebits = (f32_bits(amax) >> 23) & 0xffu;
    const unsigned sbyte = amax == 0.f ? 127u : (ebits > kEmax ? ebits - kEmax : 1u);
    return sbyte > 254u ? 254u : sbyte;
}
// The rule for emax_elem = 2 on a maximum that is zero or a normal f32 in [2^-10, 2^9] (fp4 x e4m3: the image builder of nvnative.hip), where
// neither clamp can act: the same byte as act_scale_byte<6>, without the instructions of the clamps on the builder's hot path.
PETIT_HD unsigned act_scale_byte_nv6(float amax) { return amax == 0.f ? 127u : ((f32_bits(amax) >> 23) & 0xffu) - 2u; }

} // namespace petit_amd
