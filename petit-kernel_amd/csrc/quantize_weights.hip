// quantize_weights.hip -- 16-bit weights -> packed NVFP4 / MXFP4 ("petit-cdna4/1", layout.h) on the device, with a bit-identical host twin.
// The contract (global scale, block scales, codes, ties) is stated in include/petit_amd.h "Weight quantiser"; this file is its evaluation.
//
// A pure HBM stream (2 B in, 0.5625 B out per weight) that writes the packed layout directly: a lane's 32 consecutive k of one weight row are
// its 16 bytes of a weight tile and its two NV scales (one MX scale) of the span's scale record, so neither a row-major FP4 intermediate nor the
// two repack launches exist.  The packed layout is n-tile-major: the E experts of a stacked [E][N][K] tensor are one [E N, K] matrix to it, and
// only the global scale knows about experts.
//
// Exactness.  Every code is a count of thresholds below |w|, and no comparison sees a rounded threshold's error:
//   NVFP4  t_i = mid_i x s x gs has 3 + 4 + 24 significant bits: exact in f64 (7 products per block of 16).  |w| is an f32 number, so
//          t < |w| holds exactly when (the largest f32 <= t) < |w|, and t <= |w| exactly when (the smallest f32 >= t) <= |w|: each threshold
//          is rounded once per block, in the direction its comparison asks, and the 16 elements compare in f32;
//   MXFP4  t_i = mid_i x 2^e is an f32 number (an overflow to +inf at e = 126 stands for a threshold no finite weight reaches).
// A tie goes to the even code, so thresholds 1, 3, 5 (below the codes of 1, 2, 4) count with <= and the others with <.  The only rounded
// operations are the two f32 divisions and the e4m3 encode of the NV block scale and the one division of the global scale -- IEEE on both
// sides (this file is compiled without fast-math).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "device_common.hpp"
#include "hal.h"
#include "layout.h"
#include "numfmt.h"
#include "petit_internal.h"

namespace petit_amd {

namespace {

// (|x| of a 16-bit element from its 15 magnitude bits is h16_f32 of numfmt.h on the pattern without its sign)
PETIT_HD float nv_global_scale(float amax) { return amax == 0.f ? 1.0f : amax / 2688.0f; }
PETIT_HD unsigned nv_scale_byte(float blk_amax, float gs) { return e4m3_rne_sat((blk_amax / 6.0f) / gs); }
// the e8m0 byte e + 127 of the smallest e with 6 x 2^e >= amax, e clipped to [-126, 127]: amax = f x 2^q, f in [1, 2), has e = q - 2 when
// f <= 1.5 and q - 1 above (an f32 subnormal reads q = -127 and clips; so does zero: byte 1)
PETIT_HD unsigned mx_scale_byte(float blk_amax) {
    const unsigned u = f32_bits(blk_amax);
    const int b = (int)(u >> 23) - 2 + ((u & 0x7fffffu) > 0x400000u ? 1 : 0);
    return (unsigned)(b < 1 ? 1 : b > 254 ? 254 : b);
}

// x >= 0 -> the largest f32 <= x / the smallest f32 >= x (the conversion rounds to nearest; a step of one bit pattern undoes a wrong direction)
PETIT_HD float f32_at_or_below(double x) {
    const float f = (float)x;
    return (double)f > x ? bits_f32(f32_bits(f) - 1u) : f;
}
PETIT_HD float f32_at_or_above(double x) {
    const float f = (float)x;
    return (double)f < x ? bits_f32(f32_bits(f) + 1u) : f;
}
// the seven thresholds of a block.  NVFP4: mid x s x gs exactly, then rounded down where the comparison is <, up where it is <=; a zero scale
// byte gives code 0 for the whole block (+inf thresholds).
PETIT_HD void nv_thresholds(unsigned sbyte, float gs, float (&t)[7]) {
    const double d = (double)e4m3_mag_f32(sbyte) * (double)gs; // (sbyte <= 0x7e: what e4m3_rne_sat returns)
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double x = sbyte ? (double)kE2m1Mid[i] * d : (double)INFINITY;
        t[i] = (i & 1) ? f32_at_or_above(x) : f32_at_or_below(x);
    }
}
PETIT_HD void mx_thresholds(unsigned sbyte, float (&t)[7]) {
#pragma unroll
    for (int i = 0; i < 7; ++i)
#if defined(__HIP_DEVICE_COMPILE__)
        t[i] = __builtin_ldexpf(kE2m1Mid[i], (int)sbyte - 127);
#else
        t[i] = std::ldexp(kE2m1Mid[i], (int)sbyte - 127);
#endif
}
// the e2m1 code of a 16-bit element: the number of thresholds below |w| (ties to the even code), the sign only on a non-zero magnitude
PETIT_HD unsigned fp4_code(float a, const float (&t)[7], unsigned sign) {
    const unsigned c = (unsigned)(t[0] < a) + (unsigned)(t[1] <= a) + (unsigned)(t[2] < a) + (unsigned)(t[3] <= a) + (unsigned)(t[4] < a) +
                       (unsigned)(t[5] <= a) + (unsigned)(t[6] < a);
    return c ? c | (sign << 3) : 0u;
}

// One lane's unit of work, shared by the kernel and the host twin: 32 consecutive k of one row (16 dwords of two elements) -> the 4 words of
// nibbles (word j nibble i = element 8 j + i) and the scale bytes (NV: byte 0 = group of k 0 .. 15, byte 1 = 16 .. 31; MX: byte 0).
template <bool MX, bool BF16> PETIT_HD unsigned quantize_lane(const unsigned (&d)[16], float gs, unsigned (&words)[4]) {
    unsigned mag_max[2] = {0u, 0u}; // the block maxima as 15-bit patterns: their order is the order of the values
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const unsigned lo = d[j] & 0x7fffu, hi = (d[j] >> 16) & 0x7fffu, m = lo > hi ? lo : hi;
        mag_max[j / 8] = m > mag_max[j / 8] ? m : mag_max[j / 8];
    }
    unsigned scales;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        words[j] = 0u;
    if constexpr (MX) {
        scales = mx_scale_byte(h16_f32<BF16>(mag_max[0] > mag_max[1] ? mag_max[0] : mag_max[1]));
        float t[7];
        mx_thresholds(scales, t);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned c0 = fp4_code(h16_f32<BF16>(d[j] & 0x7fffu), t, (d[j] >> 15) & 1u);
            const unsigned c1 = fp4_code(h16_f32<BF16>((d[j] >> 16) & 0x7fffu), t, d[j] >> 31);
            words[j / 4] |= (c0 | (c1 << 4)) << (8 * (j % 4));
        }
    } else {
        scales = 0u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned sbyte = nv_scale_byte(h16_f32<BF16>(mag_max[h]), gs);
            scales |= sbyte << (8 * h);
            float t[7];
            nv_thresholds(sbyte, gs, t);
#pragma unroll
            for (int j = 8 * h; j < 8 * h + 8; ++j) {
                const unsigned c0 = fp4_code(h16_f32<BF16>(d[j] & 0x7fffu), t, (d[j] >> 15) & 1u);
                const unsigned c1 = fp4_code(h16_f32<BF16>((d[j] >> 16) & 0x7fffu), t, d[j] >> 31);
                words[j / 4] |= (c0 | (c1 << 4)) << (8 * (j % 4));
            }
        }
    }
    return scales;
}

} // namespace

// how the quantise kernel gets an expert's global scale: MXFP4 has none (1.0), NVFP4 takes amax / 2688 of the amax pass or the caller's value
enum : int { kGsOne = 0, kGsFromAmax = 1, kGsSupplied = 2 };

#if defined(__HIP_DEVICE_COMPILE__)
// NB bytes of a lane's scale record (2, 4, 8 or 16), one vector store
template <int NB> __device__ __forceinline__ void store_record(unsigned char *p, const unsigned (&r)[(NB + 3) / 4]) {
    if constexpr (NB == 16) {
        *reinterpret_cast<u32x4 *>(p) = u32x4{r[0], r[1], r[2], r[3]};
    } else if constexpr (NB == 8) {
        uint2 v;
        v.x = r[0], v.y = r[1];
        *reinterpret_cast<uint2 *>(p) = v;
    } else if constexpr (NB == 4) {
        *reinterpret_cast<unsigned *>(p) = r[0];
    } else {
        *reinterpret_cast<unsigned short *>(p) = (unsigned short)r[0];
    }
}
#endif

// The amax pass: amax[e] = max |w_e| as the bit pattern of a non-negative float (unsigned order = float order), amax zeroed on the stream before.
// The tensor is `iters` wave-sized pieces of 1 KiB (64 lanes x 16 bytes; N K / 8 vectors per expert is a multiple of 512, so a piece lies in
// one expert); wave g of G takes pieces [g iters / G, (g + 1) iters / G) in order, four loads in flight, keeps the maximum of the 15-bit magnitude
// patterns in registers and leaves one vector atomic max per expert it has touched.  A maximum does not depend on arrival order.
template <bool BF16>
__global__ __launch_bounds__(256) void weight_amax_kernel(unsigned *__restrict__ amax, const u32x4 *__restrict__ w, unsigned iters,
                                                          unsigned iters_per_expert) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned lane = threadIdx.x % 64, wave = blockIdx.x * 4 + threadIdx.x / 64, waves = gridDim.x * 4;
    unsigned it = (unsigned)((uint64_t)iters * wave / waves);
    const unsigned end = (unsigned)((uint64_t)iters * (wave + 1) / waves);
    const auto fold = [](unsigned m, const u32x4 v) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned lo = v[i] & 0x7fffu, hi = (v[i] >> 16) & 0x7fffu;
            m = max(m, max(lo, hi));
        }
        return m;
    };
    while (it < end) {
        const unsigned e = it / iters_per_expert, stop = min(end, (e + 1) * iters_per_expert);
        unsigned m = 0u;
        for (; it + 4 <= stop; it += 4) {
            const u32x4 v0 = w[(size_t)it * 64 + lane], v1 = w[(size_t)(it + 1) * 64 + lane], v2 = w[(size_t)(it + 2) * 64 + lane],
                        v3 = w[(size_t)(it + 3) * 64 + lane];
            m = fold(fold(fold(fold(m, v0), v1), v2), v3);
        }
        for (; it < stop; ++it)
            m = fold(m, w[(size_t)it * 64 + lane]);
#pragma unroll
        for (int off = 32; off; off >>= 1)
            m = max(m, (unsigned)__shfl_xor((int)m, off));
        if (lane == 0)
            atomicMax(amax + e, f32_bits(h16_f32<BF16>(m)));
    }
#endif
}

// Quantise and pack, organised around the packed layout as nv6_image_kernel is: one wave = one (n-tile nt of the stacked [E N, K] matrix, span sp
// of KS k-tiles).  Lane 16 g + r reads row 16 nt + r, k 128 kt + 32 g .. + 31 (64 contiguous bytes, the next k-tile's in flight meanwhile), and
// stores its 16 bytes of tile (nt, kt) where petit_repack_nvfp4_weights would have put them; its scale bytes collect over the span and leave as
// one record of petit_repack_nvfp4_scales / petit_repack_mxfp4_scales.  No LDS, no barrier; vector stores only.  The wave of an expert's first
// tile and span also writes the expert's global scale.
template <int KS, bool MX, bool BF16>
__global__ __launch_bounds__(256) void quantize_pack_kernel(u32x4 *__restrict__ pw, unsigned char *__restrict__ ps, float *out_gs,
                                                            const u32x4 *__restrict__ w, const float *gs_src, int gs_mode, unsigned n, unsigned k,
                                                            unsigned items) { // (out_gs may be gs_src: the caller's scales written back in place)
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int kRecBytes = MX ? KS : 2 * KS;
    const unsigned lane = threadIdx.x % 64, g = lane / 16, r = lane % 16;
    const unsigned ktiles = k / kTileK, nspans = ktiles / KS, tiles_per_expert = n / kTileN, row_u4 = k / 8;
    for (unsigned item = blockIdx.x * 4 + threadIdx.x / 64; item < items; item += gridDim.x * 4) {
        const unsigned nt = item / nspans, sp = item % nspans, e = nt / tiles_per_expert;
        float gs = 1.0f;
        if (gs_mode == kGsFromAmax)
            gs = nv_global_scale(gs_src[e]);
        else if (gs_mode == kGsSupplied)
            gs = gs_src[e];
        if (lane == 0 && sp == 0 && nt % tiles_per_expert == 0)
            out_gs[e] = gs;
        const u32x4 *const row = w + (size_t)(nt * kTileN + r) * row_u4 + (size_t)sp * KS * 16 + g * 4;
        unsigned rec[(kRecBytes + 3) / 4];
#pragma unroll
        for (int i = 0; i < (kRecBytes + 3) / 4; ++i)
            rec[i] = 0u;
        u32x4 nxt[4] = {row[0], row[1], row[2], row[3]};
#pragma unroll
        for (int t = 0; t < KS; ++t) {
            unsigned d[16];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                d[i] = nxt[i / 4][i % 4];
            if (t + 1 < KS) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    nxt[i] = row[(t + 1) * 16 + i];
            }
            unsigned words[4];
            const unsigned scales = quantize_lane<MX, BF16>(d, gs, words);
            pw[((size_t)nt * ktiles + sp * KS + t) * 64 + lane] = u32x4{words[0], words[1], words[2], words[3]};
            if constexpr (MX)
                rec[t / 4] |= scales << (8 * (t % 4));
            else
                rec[t / 2] |= scales << (16 * (t % 2));
        }
        store_record<kRecBytes>(ps + (((size_t)nt * nspans + sp) * 64 + lane) * kRecBytes, rec);
    }
#endif
}

namespace {

// what both forms refuse, in one place: the element types, then the shape (every 32-bit quantity the kernels form stays in range)
int quantize_check(int a_type, int b_type, unsigned num_experts, unsigned n, unsigned k) {
    if ((a_type != kDataTypeBf16 && a_type != kDataTypeFp16) || (b_type != kDataTypeFp4e2m1 && !is_mx_type(b_type)))
        return kErrBadArgument;
    if (n % kTileN || k % 256)
        return kErrProblemShape;
    const uint64_t rows = (uint64_t)num_experts * n;
    if (rows >= (1ull << 32) || rows / kTileN * (k / 256) >= (1ull << 32) || rows * k / 512 >= (1ull << 32))
        return kErrProblemShape;
    return kOk;
}

template <int KS, bool MX> auto quantize_kernel_for(bool bf16) {
    return bf16 ? quantize_pack_kernel<KS, MX, true> : quantize_pack_kernel<KS, MX, false>;
}
template <bool MX> auto quantize_kernel_for(int ks, bool bf16) {
    return ks == 8 ? quantize_kernel_for<8, MX>(bf16) : ks == 4 ? quantize_kernel_for<4, MX>(bf16) : quantize_kernel_for<2, MX>(bf16);
}

template <bool MX, bool BF16>
void quantize_host(const uint16_t *w, unsigned rows, unsigned n, unsigned k, const float *gs, unsigned *pw, unsigned char *ps) {
    for (unsigned row = 0; row < rows; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            unsigned d[16], words[4];
            memcpy(d, w + (size_t)row * k + 32 * blk, 64);
            const unsigned scales = quantize_lane<MX, BF16>(d, gs[row / n], words);
            memcpy(pw + packed_weight_word_index(k, row, 4 * blk), words, 16);
            if constexpr (MX) {
                ps[packed_mxscale_byte_index(k, row, blk)] = (unsigned char)scales;
            } else {
                const size_t si = packed_nvscale_byte_index(k, row, 2 * blk);
                ps[si] = (unsigned char)scales, ps[si + 1] = (unsigned char)(scales >> 8);
            }
        }
}

} // namespace

uint64_t quantize_weights_workspace_bytes(int b_type, unsigned num_experts, bool gs_supplied) {
    return b_type == kDataTypeFp4e2m1 && !gs_supplied ? (uint64_t)num_experts * sizeof(float) : 0;
}

int quantize_weights(const void *w, int a_type, int b_type, unsigned num_experts, unsigned n, unsigned k, const float *gs_in, void *out_b,
                     void *out_scales, float *out_gs, void *workspace, uint64_t workspace_bytes, hipStream_t stream) {
    if (const int rc = quantize_check(a_type, b_type, num_experts, n, k))
        return rc;
    if (num_experts == 0 || n == 0 || k == 0)
        return kOk;
    if (!w || !out_b || !out_scales || !out_gs || (((uintptr_t)w | (uintptr_t)out_b | (uintptr_t)out_scales) & 15) || ((uintptr_t)out_gs & 3))
        return kErrBadArgument;
    const bool mx = is_mx_type(b_type), bf16 = a_type == kDataTypeBf16;
    const uint64_t need = quantize_weights_workspace_bytes(b_type, num_experts, gs_in != nullptr);
    if (need && !workspace)
        return kErrKernelShape; // (the code a call without the scratch it needs has everywhere: include/petit_amd.h "Scratch memory")
    if (need && (workspace_bytes < need || ((uintptr_t)workspace & 3)))
        return kErrBadArgument;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned cap = (unsigned)arch_info(dev).num_cus * 8u; // at most one full occupancy of the CUs; the waves stride over the rest
    const unsigned rows = num_experts * n;
    if (need) {
        if (hipMemsetAsync(workspace, 0, need, stream) != hipSuccess)
            return kErrLaunch;
        const unsigned iters = (unsigned)((uint64_t)rows * k / 512), iters_per_expert = (unsigned)((uint64_t)n * k / 512);
        const auto amax_kern = bf16 ? weight_amax_kernel<true> : weight_amax_kernel<false>;
        hipLaunchKernelGGL(amax_kern, dim3(std::min((iters + 15) / 16, cap)), dim3(256), 0, stream, (unsigned *)workspace, (const u32x4 *)w, iters,
                           iters_per_expert);
        if (hipGetLastError() != hipSuccess)
            return kErrLaunch;
    }
    const int ks = span_tiles_for_k(k);
    const unsigned items = rows / kTileN * (k / (kTileK * ks));
    const auto kern = mx ? quantize_kernel_for<true>(ks, bf16) : quantize_kernel_for<false>(ks, bf16);
    const float *const gs_src = mx ? nullptr : gs_in ? gs_in : (const float *)workspace;
    hipLaunchKernelGGL(kern, dim3(std::min((items + 3) / 4, cap)), dim3(256), 0, stream, (u32x4 *)out_b, (unsigned char *)out_scales, out_gs,
                       (const u32x4 *)w, gs_src, mx ? kGsOne : gs_in ? kGsSupplied : kGsFromAmax, n, k, items);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// host twin (offline conversion; bit-identical to the device kernels: tests/test_quantize_weights.py)
int quantize_weights_host(const void *w_, int a_type, int b_type, unsigned num_experts, unsigned n, unsigned k, const float *gs_in, void *out_b,
                          void *out_scales, float *out_gs) {
    if (const int rc = quantize_check(a_type, b_type, num_experts, n, k))
        return rc;
    if (num_experts == 0 || n == 0 || k == 0)
        return kOk;
    if (!w_ || !out_b || !out_scales || !out_gs)
        return kErrBadArgument;
    const bool mx = is_mx_type(b_type), bf16 = a_type == kDataTypeBf16;
    const uint16_t *const w = (const uint16_t *)w_;
    for (unsigned e = 0; e < num_experts; ++e) {
        float gs = 1.0f;
        if (!mx && gs_in) {
            gs = gs_in[e];
        } else if (!mx) {
            unsigned m = 0;
            for (size_t i = (size_t)e * n * k; i < (size_t)(e + 1) * n * k; ++i)
                m = std::max(m, w[i] & 0x7fffu);
            gs = nv_global_scale(bf16 ? h16_f32<true>(m) : h16_f32<false>(m));
        }
        out_gs[e] = gs;
    }
    const auto fn = mx ? (bf16 ? quantize_host<true, true> : quantize_host<true, false>) : (bf16 ? quantize_host<false, true> : quantize_host<false, false>);
    fn(w, num_experts * n, n, k, out_gs, (unsigned *)out_b, (unsigned char *)out_scales);
    return kOk;
}

} // namespace petit_amd
