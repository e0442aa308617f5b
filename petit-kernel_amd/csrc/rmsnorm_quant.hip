// rmsnorm_quant.hip -- (residual add +) RMSNorm that writes the native class's quantised activations: one launch computes h = x (+ residual),
// y = RMSNorm(h) * (weight + offset) and the "petit-qact/1" bytes of y in MXFP8 / MXFP6 / MXFP4, with a bit-identical host twin.
// The contract (every rounding, the ONE summation order) is stated in include/petit_amd.h "RMSNorm into quantised activations"; this file is its
// evaluation.  No counterpart in the reference, which has no norm and no activation quantiser.
//
// A memory-bound row kernel: one 256-thread workgroup per row, thread t owns the 8-element columns t + 256 j, j < ILP, as one 16-byte load each
// (the thread map of quantize_act32_kernel, gemm_native32.hpp), so the row is read from memory ONCE, stays in registers through the reduction, and
// MXFP8 / MXFP4 quantise in the map the loads already have (a quad of lanes = one 32-k block).  MXFP6 needs 32 consecutive values per lane for the
// hardware's 32-element convert: the 16-bit y row goes through LDS once (<= 32 KiB) and is quantised as quantize_act32_fp6_kernel does.
// The quantise-and-store code is COPIED from those two kernels, not shared with them: they compile to the device code they had.
//
// Host and device evaluate the same scalar helpers below; this file is compiled with floating-point contraction OFF (the pragma), so a product
// and a sum fuse only where the code says fma, on either side.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "device_common.hpp"
#include "petit_internal.h"

#pragma clang fp contract(off)

namespace petit_amd {

namespace {

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

// one rounding each, never fused with a neighbour (contraction is off in this file)
PETIT_HD float mul_rn(float a, float b) { return a * b; }
PETIT_HD float add_rn(float a, float b) { return a + b; }
PETIT_HD float fma_rn(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// a 16-bit element -> f32 (exact)
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
// f32 -> the 16-bit element, round to nearest even (bf16 by the integer rule on both sides; fp16 by the hardware convert on the device and the
// same rule spelled out on the host: overflow to infinity from 65520 up, subnormals as multiples of 2^-24)
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
// the two elements of a dword
template <bool BF16> PETIT_HD void unpack2(unsigned w, float &lo, float &hi) {
    if constexpr (BF16) {
        lo = bits_f32(w << 16), hi = bits_f32(w & 0xffff0000u);
    } else {
        lo = h16_f32<false>(w & 0xffffu), hi = h16_f32<false>(w >> 16);
    }
}
template <bool BF16> PETIT_HD unsigned pack2(float lo, float hi) { return (f32_h16<BF16>(lo) & 0xffffu) | (f32_h16<BF16>(hi) << 16); }

// the quantiser's scale rule (quantize_act32_kernel, gemm_native32.hpp): E8M0 byte of 2^(E - emax_elem), E the exponent of the block maximum,
// emax_elem = 7 for e4m3 as the native kernels use it, 2 for e2m3 and e2m1; a zero block: byte 127
template <int ACT> PETIT_HD unsigned act_scale_byte(float amax) {
    constexpr unsigned kEmax = ACT == 8 ? 7u : 2u;
    const unsigned ebits = (f32_bits(amax) >> 23) & 0xffu;
    const unsigned sbyte = amax == 0.f ? 127u : (ebits > kEmax ? ebits - kEmax : 1u);
    return sbyte > 254u ? 254u : sbyte;
}

// the sum of squares of one 8-element column: an ascending chain
PETIT_HD float column_sumsq(const float (&v)[8]) {
    float p = mul_rn(v[0], v[0]);
#pragma unroll
    for (int i = 1; i < 8; ++i)
        p = fma_rn(v[i], v[i], p);
    return p;
}
// steps 3 and 4 of the contract
PETIT_HD float inv_rms(float sumsq, float rk, float eps) {
#if defined(__HIP_DEVICE_COMPILE__)
    return 1.0f / __builtin_sqrtf(add_rn(mul_rn(sumsq, rk), eps)); // (correctly rounded: no fast-math in this library's build)
#else
    return 1.0f / std::sqrt(add_rn(mul_rn(sumsq, rk), eps));
#endif
}
PETIT_HD float normed(float h, float inv, float w, float woff) { return mul_rn(mul_rn(h, inv), add_rn(w, woff)); }

} // namespace

struct RmsQuantArgs {
    unsigned char *qa;
    void *y16, *res_out;      // nullable
    const void *x, *res, *w;  // res nullable
    float eps, woff, rk;      // rk = 1 / k, rounded once on the host
    unsigned m, k;
};

// grid = (M): one workgroup per row.  ILP = columns per thread: K <= 2048 ILP.  Lanes whose column lies past K / 8 hold zeros and add +0 to the sum;
// K / 8 is a multiple of 32, so the 16 lanes of a k-tile (and the 4 of a block) are masked together and every shuffle below stays among live lanes.
template <bool BF16, int ACT, int ILP> __global__ __launch_bounds__(256) void rmsnorm_quant_kernel(const RmsQuantArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float wave_sum[4];
    __shared__ u32x4 y_row[ACT == 6 ? 256 * ILP : 1]; // MXFP6 only: the 16-bit y row
    const unsigned t = threadIdx.x, row = blockIdx.x, cols = p.k / 8, m = p.m;
    const size_t row_v = (size_t)row * cols;
    const u32x4 *const x_row = reinterpret_cast<const u32x4 *>(p.x) + row_v;
    const u32x4 *const w_row = reinterpret_cast<const u32x4 *>(p.w);
    // every load of the row is requested before the first is used
    u32x4 h[ILP], wv[ILP];
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        const unsigned c = t + 256u * j;
        h[j] = c < cols ? x_row[c] : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        const unsigned c = t + 256u * j;
        wv[j] = c < cols ? w_row[c] : u32x4{0u, 0u, 0u, 0u};
    }
    if (p.res) { // (wave-uniform: one branch around all the residual loads, not one per load)
        const u32x4 *const r_row = reinterpret_cast<const u32x4 *>(p.res) + row_v;
        u32x4 r[ILP];
#pragma unroll
        for (int j = 0; j < ILP; ++j) {
            const unsigned c = t + 256u * j;
            r[j] = c < cols ? r_row[c] : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < ILP; ++j)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned xw = h[j][d], rw = r[j][d];
                float x0, x1, r0, r1;
                unpack2<BF16>(xw, x0, x1);
                unpack2<BF16>(rw, r0, r1);
                h[j][d] = pack2<BF16>(add_rn(x0, r0), add_rn(x1, r1));
            }
        if (p.res_out) { // a thread writes only the columns it has read: res_out may be residual or x
            u32x4 *const o_row = reinterpret_cast<u32x4 *>(p.res_out) + row_v;
#pragma unroll
            for (int j = 0; j < ILP; ++j) {
                const unsigned c = t + 256u * j;
                if (c < cols)
                    o_row[c] = h[j];
            }
        }
    }
    // the sum of squares in the contract's order: column chains, the thread's columns ascending, butterflies 1 .. 32, the four waves ascending
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        float v[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned hw = h[j][d];
            unpack2<BF16>(hw, v[2 * d], v[2 * d + 1]);
        }
        s = add_rn(s, column_sumsq(v));
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
        s = add_rn(s, __shfl_xor(s, off));
    if (t % 64 == 0)
        wave_sum[t / 64] = s;
    __syncthreads();
    const float sumsq = add_rn(add_rn(add_rn(wave_sum[0], wave_sum[1]), wave_sum[2]), wave_sum[3]);
    const float inv = inv_rms(sumsq, p.rk, p.eps), woff = p.woff;

    const unsigned row_bytes = p.k / 8 * ACT;
    unsigned char *const qa = p.qa;
    unsigned char *const qs = p.qa + (size_t)m * row_bytes;
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        const unsigned c8 = t + 256u * j; // 8-element column
        if (c8 < cols) {
            u32x4 yv;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned hw = h[j][d], ww = wv[j][d];
                float h0, h1, w0, w1;
                unpack2<BF16>(hw, h0, h1);
                unpack2<BF16>(ww, w0, w1);
                yv[d] = pack2<BF16>(normed(h0, inv, w0, woff), normed(h1, inv, w1, woff));
            }
            if (p.y16)
                (reinterpret_cast<u32x4 *>(p.y16) + row_v)[c8] = yv;
            if constexpr (ACT == 6) {
                y_row[c8] = yv;
            } else {
                // from here: quantize_act32_kernel's column, on the 16-bit y
                float v[8];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned yw = yv[d];
                    unpack2<BF16>(yw, v[2 * d], v[2 * d + 1]);
                }
                float amax = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    amax = fmaxf(amax, fabsf(v[i]));
                amax = fmaxf(amax, __shfl_xor(amax, 1));
                amax = fmaxf(amax, __shfl_xor(amax, 2));
                const unsigned sbyte = act_scale_byte<ACT>(amax);
                const unsigned kt = c8 / 16, col16 = c8 % 16;
                if constexpr (ACT == 8) {
                    const float sc = bits_f32((254u - sbyte) << 23); // 2^-(sbyte-127)
                    int q0 = 0, q1 = 0;
                    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * sc, v[1] * sc, q0, false);
                    q0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * sc, v[3] * sc, q0, true);
                    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * sc, v[5] * sc, q1, false);
                    q1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * sc, v[7] * sc, q1, true);
                    const unsigned u16 = col16 >> 1, half = col16 & 1u;
                    const unsigned pos = (u16 & 4u) | ((u16 & 1u) << 1) | ((u16 >> 1) & 1u);
                    uint2 o;
                    o.x = (unsigned)q0, o.y = (unsigned)q1;
                    *reinterpret_cast<uint2 *>(qa + ((size_t)kt * m + row) * 128 + pos * 16 + half * 8) = o;
                } else {
                    const float scale = bits_f32(sbyte << 23); // 2^(sbyte-127)
                    unsigned q = 0;
                    q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[0], v[1], scale, 0);
                    q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[2], v[3], scale, 1);
                    q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[4], v[5], scale, 2);
                    q = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(q, v[6], v[7], scale, 3);
                    *reinterpret_cast<unsigned *>(qa + ((size_t)kt * m + row) * 64 + col16 * 4) = q;
                }
                // the four scale bytes of a row's k-tile leave as one dword: the first lane of each quad holds the quad's byte
                const unsigned s1 = __shfl_down(sbyte, 4, 16), s2 = __shfl_down(sbyte, 8, 16), s3 = __shfl_down(sbyte, 12, 16);
                if (col16 == 0)
                    *reinterpret_cast<unsigned *>(qs + ((size_t)kt * m + row) * 4) = sbyte | (s1 << 8) | (s2 << 16) | (s3 << 24);
            }
        }
    }
    if constexpr (ACT == 6) {
        // from here: quantize_act32_fp6_kernel's block, read from the LDS row -- one thread = one 32-k block, the four blocks of a k-tile on four
        // consecutive lanes
        __syncthreads();
        const unsigned blocks = p.k / 32;
        unsigned char *const qa_hi = p.qa + (size_t)m * (p.k / 2);
#pragma unroll
        for (int i = 0; i < (ILP + 3) / 4; ++i) {
            const unsigned blk = t + 256u * i;
            if (blk < blocks) {
                u32x4 raw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    raw[q] = y_row[blk * 4 + q];
                unsigned mx = 0; // the block maximum on the 16-bit patterns, sign cleared
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const unsigned w = raw[q][d] & 0x7fff7fffu;
                        const unsigned lo = w & 0xffffu, hi = w >> 16;
                        mx = mx > lo ? mx : lo;
                        mx = mx > hi ? mx : hi;
                    }
                const unsigned sbyte = act_scale_byte<6>(h16_f32<BF16>(mx));
                const float scale = bits_f32(sbyte << 23);
                const u32x16 packed = u32x16{raw[0][0], raw[0][1], raw[0][2], raw[0][3], raw[1][0], raw[1][1], raw[1][2], raw[1][3],
                                             raw[2][0], raw[2][1], raw[2][2], raw[2][3], raw[3][0], raw[3][1], raw[3][2], raw[3][3]};
                const u32x6 q = cvt_pk32_fp6_16bit<BF16>(packed, scale); // (early-clobber form: device_common.hpp)
                const unsigned kt = blk / 4, b = blk % 4;
                const size_t tile_row = (size_t)kt * m + row;
                *reinterpret_cast<u32x4 *>(qa + tile_row * 64 + 16 * b) = u32x4{q[0], q[1], q[2], q[3]};
                uint2 tail;
                tail.x = q[4], tail.y = q[5];
                *reinterpret_cast<uint2 *>(qa_hi + tile_row * 32 + 8 * ((b & 1u) * 2 + (b >> 1))) = tail;
                const unsigned s1 = __shfl_down(sbyte, 1, 4), s2 = __shfl_down(sbyte, 2, 4), s3 = __shfl_down(sbyte, 3, 4);
                if (b == 0)
                    *reinterpret_cast<unsigned *>(qs + tile_row * 4) = sbyte | (s1 << 8) | (s2 << 16) | (s3 << 24);
            }
        }
    }
#endif
}

namespace {

// what both forms refuse, in one place (include/petit_amd.h lists it); kOk with *run = false: nothing to do
int rmsq_check(const void *qa, const void *y16, const void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
               unsigned k, int a_type, int format, bool *run) {
    *run = false;
    if (m == 0 || k == 0)
        return kOk;
    if (format != 8 && format != 6 && format != 4)
        return kErrBadArgument;
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrKernelShape;
    if (k % 256 != 0 || m > kMaxM)
        return kErrProblemShape;
    if (k > 16384)
        return kErrKernelShape; // (the row is held in registers)
    if (!std::isfinite(eps) || !(eps > 0.f) || !std::isfinite(woff))
        return kErrBadArgument;
    if (!qa || !x || !w || (res_out && !res))
        return kErrBadArgument;
    if (((uintptr_t)qa | (uintptr_t)y16 | (uintptr_t)res_out | (uintptr_t)x | (uintptr_t)res | (uintptr_t)w) & 15)
        return kErrBadArgument;
    *run = true;
    return kOk;
}

template <bool BF16, int ACT> auto rmsq_kernel_for(unsigned k) {
    return k <= 2048   ? rmsnorm_quant_kernel<BF16, ACT, 1>
           : k <= 4096 ? rmsnorm_quant_kernel<BF16, ACT, 2>
           : k <= 8192 ? rmsnorm_quant_kernel<BF16, ACT, 4>
                       : rmsnorm_quant_kernel<BF16, ACT, 8>;
}
template <bool BF16> auto rmsq_kernel_for(int format, unsigned k) {
    return format == 8 ? rmsq_kernel_for<BF16, 8>(k) : format == 6 ? rmsq_kernel_for<BF16, 6>(k) : rmsq_kernel_for<BF16, 4>(k);
}

// --- the host twin's element converts: round to nearest even of x (any sign; the sign is kept, on a zero too), as the hardware converts do ---
// e4m3fn byte; |x| <= 256 here (the block maximum lands in [128, 256))
unsigned e4m3_rne_host(float x) {
    const unsigned sign = (f32_bits(x) >> 24) & 0x80u;
    const float ax = std::fabs(x);
    if (!(ax < 448.0f))
        return sign | 0x7eu;
    if (ax < 0.015625f) // below 2^-6: multiples of 2^-9; ax x 512 is exact, the add rounds it to an integer (8 = the byte of 2^-6)
        return sign | (f32_bits(ax * 512.0f + 8388608.0f) & 15u);
    const unsigned u = f32_bits(ax);
    return sign | (((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - (120u << 3));
}
// e2m1 code of x = v / scale (exact in f64): the number of midpoints below |x|, a tie to the even code; saturates at 6
unsigned e2m1_rne_host(double x) {
    const unsigned sign = std::signbit(x) ? 8u : 0u;
    const double a = std::fabs(x);
    return sign | ((unsigned)(0.25 < a) + (unsigned)(0.75 <= a) + (unsigned)(1.25 < a) + (unsigned)(1.75 <= a) + (unsigned)(2.5 < a) +
                   (unsigned)(3.5 <= a) + (unsigned)(5.0 < a));
}
// e2m3 code: subnormal step 1/8, normals 1 .. 7.5, saturating (nvnative.hip e2m3_rne_host, on an exact f64 quotient)
unsigned e2m3_rne_host(double x) {
    const unsigned sign = std::signbit(x) ? 32u : 0u;
    const double ax = std::fabs(x);
    if (ax >= 7.5)
        return sign | 31u;
    if (ax < 1.0)
        return sign | (unsigned)std::nearbyint(ax * 8.0); // (8 = the code of 1.0)
    int e;
    (void)std::frexp(ax, &e);
    e -= 1; // floor(log2 ax): 0 .. 2
    unsigned r = (unsigned)std::nearbyint(std::ldexp(ax, 3 - e)); // 8 .. 16
    if (r == 16)
        r = 8, e += 1;
    return sign | ((unsigned)(e + 1) << 3) | (r - 8u);
}

// one row of the quantiser on the 16-bit y, written where the kernels write it
template <bool BF16, int ACT> void quantize_row_host(unsigned char *ws, const uint16_t *y, unsigned m, unsigned k, unsigned row) {
    unsigned char *const qs = ws + (size_t)m * (k / 8 * ACT);
    unsigned char *const qa_hi = ws + (size_t)m * (k / 2); // (MXFP6)
    for (unsigned blk = 0; blk < k / 32; ++blk) {
        float v[32], amax = 0.f;
        for (int i = 0; i < 32; ++i) {
            v[i] = h16_f32<BF16>(y[32 * blk + i]);
            amax = std::fmax(amax, std::fabs(v[i])); // (a NaN does not count, as fmaxf on the device)
        }
        const unsigned sbyte = act_scale_byte<ACT>(amax);
        const unsigned kt = blk / 4, b = blk % 4;
        const size_t tile_row = (size_t)kt * m + row;
        qs[tile_row * 4 + b] = (unsigned char)sbyte;
        if constexpr (ACT == 8) {
            const float sc = bits_f32((254u - sbyte) << 23);
            for (unsigned c = 0; c < 4; ++c) { // the block's four 8-element columns
                const unsigned col16 = 4 * b + c, u16 = col16 >> 1, half = col16 & 1u;
                const unsigned pos = (u16 & 4u) | ((u16 & 1u) << 1) | ((u16 >> 1) & 1u);
                unsigned char *const o = ws + tile_row * 128 + pos * 16 + half * 8;
                for (int i = 0; i < 8; ++i)
                    o[i] = (unsigned char)e4m3_rne_host(v[8 * c + i] * sc);
            }
        } else if constexpr (ACT == 4) {
            unsigned char *const o = ws + tile_row * 64 + 16 * b;
            for (int i = 0; i < 16; ++i)
                o[i] = (unsigned char)(e2m1_rne_host(std::ldexp((double)v[2 * i], 127 - (int)sbyte)) |
                                       (e2m1_rne_host(std::ldexp((double)v[2 * i + 1], 127 - (int)sbyte)) << 4));
        } else {
            unsigned char bytes[24] = {};
            for (int i = 0; i < 32; ++i) { // element i at bits [6 i, 6 i + 6)
                const unsigned code = e2m3_rne_host(std::ldexp((double)v[i], 127 - (int)sbyte));
                const unsigned bit = 6 * i;
                bytes[bit / 8] |= (unsigned char)(code << (bit % 8));
                if (bit % 8 > 2)
                    bytes[bit / 8 + 1] |= (unsigned char)(code >> (8 - bit % 8));
            }
            memcpy(ws + tile_row * 64 + 16 * b, bytes, 16);
            memcpy(qa_hi + tile_row * 32 + 8 * ((b & 1u) * 2 + (b >> 1)), bytes + 16, 8);
        }
    }
}

// steps 2 and 3 on one row of h -- the kernel's reduction, walked literally: 256 thread sums, six butterflies inside each wave of 64, the four
// waves in ascending order
template <bool BF16> float row_inv_host(const uint16_t *h, unsigned k, float rk, float eps) {
    const unsigned cols = k / 8;
    float s[256];
    for (unsigned t = 0; t < 256; ++t) {
        s[t] = 0.f;
        for (unsigned c = t; c < cols; c += 256) {
            float v[8];
            for (int i = 0; i < 8; ++i)
                v[i] = h16_f32<BF16>(h[8 * c + i]);
            s[t] = add_rn(s[t], column_sumsq(v));
        }
    }
    for (unsigned off = 1; off < 64; off <<= 1) {
        float n[256];
        for (unsigned t = 0; t < 256; ++t)
            n[t] = add_rn(s[t], s[t ^ off]);
        memcpy(s, n, sizeof(s));
    }
    return inv_rms(add_rn(add_rn(add_rn(s[0], s[64]), s[128]), s[192]), rk, eps);
}
template <bool BF16> void add_row_host(uint16_t *h, const uint16_t *x, const uint16_t *r, unsigned k) {
    for (unsigned i = 0; i < k; ++i)
        h[i] = r ? (uint16_t)f32_h16<BF16>(add_rn(h16_f32<BF16>(x[i]), h16_f32<BF16>(r[i]))) : x[i];
}

template <bool BF16, int ACT> void rmsq_host(const RmsQuantArgs &p) {
    const unsigned k = p.k;
    std::vector<uint16_t> h(k), y(k);
    const uint16_t *const w = (const uint16_t *)p.w;
    for (unsigned row = 0; row < p.m; ++row) {
        const uint16_t *const x = (const uint16_t *)p.x + (size_t)row * k;
        const uint16_t *const r = p.res ? (const uint16_t *)p.res + (size_t)row * k : nullptr;
        add_row_host<BF16>(h.data(), x, r, k);
        if (p.res_out)
            memcpy((uint16_t *)p.res_out + (size_t)row * k, h.data(), 2 * (size_t)k);
        const float inv = row_inv_host<BF16>(h.data(), k, p.rk, p.eps);
        for (unsigned i = 0; i < k; ++i)
            y[i] = (uint16_t)f32_h16<BF16>(normed(h16_f32<BF16>(h[i]), inv, h16_f32<BF16>(w[i]), p.woff));
        if (p.y16)
            memcpy((uint16_t *)p.y16 + (size_t)row * k, y.data(), 2 * (size_t)k);
        quantize_row_host<BF16, ACT>(p.qa, y.data(), p.m, k, row);
    }
}

RmsQuantArgs rmsq_args(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
                       unsigned k) {
    return RmsQuantArgs{(unsigned char *)qa, y16, res_out, x, res, w, eps, woff, 1.0f / (float)k, m, k};
}

} // namespace

int rmsnorm_quantize(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m, unsigned k,
                     int a_type, int format, hipStream_t stream) {
    bool run;
    if (const int rc = rmsq_check(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, &run); rc != kOk || !run)
        return rc;
    const auto kern = a_type == kDataTypeBf16 ? rmsq_kernel_for<true>(format, k) : rmsq_kernel_for<false>(format, k);
    hipLaunchKernelGGL(kern, dim3(m), dim3(256), 0, stream, rmsq_args(qa, y16, res_out, x, res, w, eps, woff, m, k));
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int rmsnorm_quantize_host(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
                          unsigned k, int a_type, int format) {
    bool run;
    if (const int rc = rmsq_check(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, &run); rc != kOk || !run)
        return rc;
    const RmsQuantArgs p = rmsq_args(qa, y16, res_out, x, res, w, eps, woff, m, k);
    const bool bf16 = a_type == kDataTypeBf16;
    if (format == 8)
        bf16 ? rmsq_host<true, 8>(p) : rmsq_host<false, 8>(p);
    else if (format == 6)
        bf16 ? rmsq_host<true, 6>(p) : rmsq_host<false, 6>(p);
    else
        bf16 ? rmsq_host<true, 4>(p) : rmsq_host<false, 4>(p);
    return kOk;
}

// the f32 `inv` of every row as the host twin (and so the kernel) forms it: what a test of steps 2 and 3 needs, since y carries it only through
// a 16-bit rounding
int rmsnorm_inv_host(float *inv, const void *x, const void *res, float eps, unsigned m, unsigned k, int a_type) {
    bool run;
    alignas(16) static const uint64_t aligned[2] = {0, 0}; // (stands in for the pointers this query does not take)
    if (const int rc = rmsq_check(aligned, nullptr, nullptr, x, res, aligned, eps, 0.f, m, k, a_type, 8, &run); rc != kOk || !run)
        return rc;
    if (!inv)
        return kErrBadArgument;
    std::vector<uint16_t> h(k);
    for (unsigned row = 0; row < m; ++row) {
        const uint16_t *const xr = (const uint16_t *)x + (size_t)row * k;
        const uint16_t *const rr = res ? (const uint16_t *)res + (size_t)row * k : nullptr;
        if (a_type == kDataTypeBf16) {
            add_row_host<true>(h.data(), xr, rr, k);
            inv[row] = row_inv_host<true>(h.data(), k, 1.0f / (float)k, eps);
        } else {
            add_row_host<false>(h.data(), xr, rr, k);
            inv[row] = row_inv_host<false>(h.data(), k, 1.0f / (float)k, eps);
        }
    }
    return kOk;
}

} // namespace petit_amd
