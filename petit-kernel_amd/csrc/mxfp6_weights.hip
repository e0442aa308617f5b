// mxfp6_weights.hip -- MXFP6 (e2m3) weights straight into the MFMA-native image ("petit-cdna4-nv6/1", layout.h): quantised from 16-bit weights
// on the device, or ingested without rounding from an OCP MXFP6 tensor; bit-identical host twins.  The rule (scale, codes, zero blocks) is stated
// in include/petit_amd.h "MXFP6 weights on the native class": it is the activation quantiser's (act_scale_byte<6>, numfmt.h; the hardware's
// 32-element convert).  The image is what nvnative.hip builds from NVFP4 -- the same consumers read it -- but its elements never saw a 4-bit rounding.
//
// Why not nv6_image_kernel's organisation (lane 32 h + r owns weight row r): packed FP4 is lane-major already, a row-major 16-bit source is
// not -- the 32 rows of a block are 2 K bytes apart.  Here ONE WORKGROUP owns one (32-row block b, span sp of KS k-tiles), the unit at which both
// parts of the image are contiguous (3072 KS element bytes, one 64 x 2 KS scale record), and the transpose from "along K" to "lane = row" goes
// through LDS on the CONVERTED data (0.75 B per weight instead of 2):
//   load      thread t takes the 16-byte units t, t + 256, ... of the block's 32 x 16 KS units (row-major: a wave reads 1 KiB of one row, or of
//             two at KS = 2); all 2 KS loads are issued before the first use.  A quad of lanes is one 32-k block.  Rows >= N load nothing and
//             read as zeros.
//   quantise  where the data landed: the block maximum on the 15-bit magnitude patterns, across the quad by two DPP quad_perm moves; the scale
//             byte; the hardware convert on the lane's 8 elements (the 32-wide instruction on a vector that is zero elsewhere: 48 bits out).
//             Three more quad_perm moves collect the quad's 4 x 48 bits: lane 0 of the quad ends with registers 0-3 of the block, lane 2 with
//             registers 4-5.
//   stage     lo[j][r] (16 bytes: registers 0-3 of block j of the span, row r) and hi[j][r] (16 bytes: registers 4-5, the scale byte, 0), each
//             with 33 entries per j.  The writers of a wave are 16 lanes of consecutive j and equal r: 528 bytes apart, i.e. 4 banks apart --
//             without the 33rd entry they would all start in one bank.  The readers are consecutive r of one j: consecutive 16 bytes.
//   store     the span's 192 KS units of the image in image order, unit v by thread v % 256: unit (t, plane, lane 32 h + r) is lo[4 t + 2 plane + h][r]
//             for planes 0 / 1 and {hi[4 t + h][r].xy, hi[4 t + 2 + h][r].xy} for plane 2 -- a workgroup store is one contiguous run; the last
//             wave also gathers its lane's 2 KS scale bytes from hi[..][r].z and stores them as one record.  Vector stores only; every byte of
//             the image is written.
// The OCP ingest is the same kernel with another load stage: thread t takes whole 32-k blocks (24 bytes as three 8-byte loads, and the scale
// byte) and writes lo / hi directly.
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

// the source of the load stage
enum : int { kSrcBf16 = 0, kSrcFp16 = 1, kSrcOcp = 2 };

#if defined(__HIP_DEVICE_COMPILE__)
namespace {
template <int CTRL> __device__ __forceinline__ unsigned quad_mov(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false);
}
constexpr int kQuadXor1 = 0xB1; // quad_perm:[1,0,3,2]
constexpr int kQuadXor2 = 0x4E; // quad_perm:[2,3,0,1]
constexpr int kStageRows = 33;  // entries per block of the span in lo / hi: 32 rows and the pad (file comment)
} // namespace
#endif

template <int KS, int SRC>
__global__ __launch_bounds__(256) void mxfp6_image_kernel(unsigned char *__restrict__ images, const unsigned char *__restrict__ src,
                                                          const unsigned char *__restrict__ src_scales, unsigned n, unsigned k, unsigned per_expert,
                                                          unsigned items) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ u32x4 lo[4 * KS][kStageRows];
    __shared__ u32x4 hi[4 * KS][kStageRows];
    const unsigned tid = threadIdx.x;
    const unsigned ktiles = k / kTileK, nspans = ktiles / KS;
    const size_t image_bytes = nv6_image_bytes(n, k), elem_bytes = nv6_elem_bytes(n, k);
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned e = item / per_expert, rem = item % per_expert, b32 = rem / nspans, sp = rem % nspans;
        unsigned char *const img = images + e * image_bytes;
        if constexpr (SRC == kSrcOcp) {
            // ---- load stage, OCP MXFP6: whole blocks, no arithmetic
            constexpr int kBlocks = KS / 2 ? KS / 2 : 1; // 128 KS blocks per item, 256 threads
            const unsigned char *const el = src + (size_t)e * n * (k / 4 * 3);
            const unsigned char *const sc = src_scales + (size_t)e * n * (k / 32);
            uint2 w[kBlocks][3];
            unsigned sb[kBlocks];
#pragma unroll
            for (int i = 0; i < kBlocks; ++i) {
                const unsigned flat = i * 256 + tid, r = flat / (4 * KS), j = flat % (4 * KS), row = b32 * 32 + r;
                const bool live = flat < 128 * KS && row < n;
                const size_t blk = (size_t)row * (k / 32) + sp * KS * 4 + j;
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    w[i][d] = live ? reinterpret_cast<const uint2 *>(el + blk * 24)[d] : uint2{0u, 0u};
                sb[i] = live ? (unsigned)sc[blk] : 127u;
            }
#pragma unroll
            for (int i = 0; i < kBlocks; ++i) {
                const unsigned flat = i * 256 + tid, r = flat / (4 * KS), j = flat % (4 * KS);
                if (flat < 128 * KS) {
                    lo[j][r] = u32x4{w[i][0].x, w[i][0].y, w[i][1].x, w[i][1].y};
                    hi[j][r] = u32x4{w[i][2].x, w[i][2].y, sb[i], 0u};
                }
            }
        } else {
            // ---- load stage, 16-bit weights: 16-byte units along K, every load before the first use
            constexpr bool kBf16 = SRC == kSrcBf16;
            constexpr int kUnits = 2 * KS; // 512 KS units per item, 256 threads
            const unsigned char *const w16 = src + (size_t)e * n * k * 2;
            u32x4 raw[kUnits];
#pragma unroll
            for (int i = 0; i < kUnits; ++i) {
                const unsigned flat = i * 256 + tid, r = flat / (16 * KS), u = flat % (16 * KS), row = b32 * 32 + r;
                raw[i] = u32x4{0u, 0u, 0u, 0u};
                if (row < n)
                    raw[i] = *reinterpret_cast<const u32x4 *>(w16 + ((size_t)row * k + (size_t)sp * KS * kTileK + u * 8) * 2);
            }
#pragma unroll
            for (int i = 0; i < kUnits; ++i) {
                const unsigned flat = i * 256 + tid, r = flat / (16 * KS), u = flat % (16 * KS), j = u / 4, c = u % 4;
                // the block maximum: magnitudes order like their 15-bit patterns
                unsigned mx = 0;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned m2 = raw[i][d] & 0x7fff7fffu;
                    mx = max(mx, max(m2 & 0xffffu, m2 >> 16));
                }
                mx = max(mx, quad_mov<kQuadXor1>(mx));
                mx = max(mx, quad_mov<kQuadXor2>(mx));
                const unsigned sbyte = act_scale_byte<6>(h16_f32<kBf16>(mx));
                // the lane's 8 elements: bits [0, 48) of a 32-wide convert whose other 24 sources are zero (early-clobber form: device_common.hpp)
                const u32x16 packed = u32x16{raw[i][0], raw[i][1], raw[i][2], raw[i][3], 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                const u32x6 q = cvt_pk32_fp6_16bit<kBf16>(packed, bits_f32(sbyte << 23));
                const unsigned x = q[0], y = q[1] & 0xffffu;
                // the quad's 4 x 48 bits -> the block's 6 registers: lanes 0 / 2 take their neighbour's 48 bits and hold registers 0-2 / 3-5
                const unsigned x1 = quad_mov<kQuadXor1>(x), y1 = quad_mov<kQuadXor1>(y);
                const unsigned wa = x, wb = y | (x1 << 16), wc = (x1 >> 16) | (y1 << 16);
                const unsigned w3 = quad_mov<kQuadXor2>(wa); // (lane 0: register 3, from lane 2)
                if (c == 0)
                    lo[j][r] = u32x4{wa, wb, wc, w3};
                else if (c == 2)
                    hi[j][r] = u32x4{wb, wc, sbyte, 0u};
            }
        }
        __syncthreads();
        // ---- store stage: the span's units in image order
        unsigned char *const tiles = img + ((size_t)b32 * ktiles + (size_t)sp * KS) * kNv6TileBytes;
        for (unsigned v = tid; v < 192u * KS; v += 256) {
            const unsigned t = v / 192, plane = v % 192 / 64, lane = v % 64, h = lane / 32, r = lane % 32;
            u32x4 out;
            if (plane < 2) {
                out = lo[4 * t + 2 * plane + h][r];
            } else {
                const u32x4 p1 = hi[4 * t + h][r], p2 = hi[4 * t + 2 + h][r];
                out = u32x4{p1[0], p1[1], p2[0], p2[1]};
            }
            *reinterpret_cast<u32x4 *>(tiles + (size_t)v * 16) = out;
        }
        if (tid >= 192) { // the scale record of lane (r, h): byte [q][t] = the scale of block 4 t + 2 q + h of the span
            const unsigned lane = tid - 192, h = lane / 32, r = lane % 32;
            unsigned rec[KS / 2];
#pragma unroll
            for (int d = 0; d < KS / 2; ++d)
                rec[d] = 0u;
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int t = 0; t < KS; ++t)
                    rec[(q * KS + t) / 4] |= (hi[4 * t + 2 * q + h][r][2] & 0xffu) << (8 * ((q * KS + t) % 4));
            unsigned char *const p = img + elem_bytes + (((size_t)b32 * nspans + sp) * 64 + lane) * (2 * KS);
            if constexpr (KS == 8) {
                *reinterpret_cast<u32x4 *>(p) = u32x4{rec[0], rec[1], rec[2], rec[3]};
            } else if constexpr (KS == 4) {
                uint2 o;
                o.x = rec[0], o.y = rec[1];
                *reinterpret_cast<uint2 *>(p) = o;
            } else {
                *reinterpret_cast<unsigned *>(p) = rec[0];
            }
        }
        __syncthreads(); // (the next item's stage writes)
    }
#endif
}

namespace {

// what the device forms and their host twins refuse, in one place and in this order: the shape, then (by the callers) nothing-to-do, then pointers
int mxfp6_shape(unsigned num_experts, unsigned n, unsigned k) {
    if (num_experts == 0 || num_experts > kMoeMaxExperts)
        return kErrProblemShape;
    if (n % kTileN || k % 256)
        return kErrProblemShape;
    if (nv6_elem_bytes(n, k) >= (1ull << 32) || (uint64_t)num_experts * ((n + 31) / 32) * (k / 256) >= (1ull << 32))
        return kErrProblemShape; // (an image is what its consumers address through one 32-bit descriptor; the item count is 32-bit)
    return kOk;
}

template <int SRC> auto mxfp6_kernel_for(int ks) {
    return ks == 8 ? mxfp6_image_kernel<8, SRC> : ks == 4 ? mxfp6_image_kernel<4, SRC> : mxfp6_image_kernel<2, SRC>;
}

int mxfp6_launch(int src_kind, void *images, const void *src, const void *src_scales, unsigned num_experts, unsigned n, unsigned k,
                 hipStream_t stream) {
    const int ks = span_tiles_for_k(k);
    const unsigned per_expert = (n + 31) / 32 * (k / (kTileK * ks)), items = num_experts * per_expert;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned cap = (unsigned)arch_info(dev).num_cus * 4u; // what the stage's LDS lets a CU hold at KS = 8; the workgroups stride over the rest
    const auto kern = src_kind == kSrcBf16 ? mxfp6_kernel_for<kSrcBf16>(ks) : src_kind == kSrcFp16 ? mxfp6_kernel_for<kSrcFp16>(ks)
                                                                                                   : mxfp6_kernel_for<kSrcOcp>(ks);
    hipLaunchKernelGGL(kern, dim3(std::min(items, cap)), dim3(256), 0, stream, (unsigned char *)images, (const unsigned char *)src,
                       (const unsigned char *)src_scales, n, k, per_expert, items);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// one block of one row into an image (host): registers 0-3, registers 4-5 and the scale byte where the consumers read them
void mxfp6_place_host(unsigned char *img, unsigned n, unsigned k, unsigned row, unsigned blk, const unsigned (&words)[6], unsigned sbyte) {
    const unsigned kt = blk / 4, q = (blk % 4) >> 1, h = blk & 1u;
    memcpy(img + nv6_unit_offset(k, row, kt, q, h), words, 16);
    memcpy(img + nv6_unit_offset(k, row, kt, 2, h) + q * 8, words + 4, 8);
    img[nv6_elem_bytes(n, k) + nv6_scale_offset(k, row, blk)] = (unsigned char)sbyte;
}

} // namespace

int mxfp6_quantize_weights(const void *w, int a_type, unsigned num_experts, unsigned n, unsigned k, void *images, hipStream_t stream) {
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrBadArgument;
    if (const int rc = mxfp6_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (((uintptr_t)w & 15) || ((uintptr_t)images & 255) || !w || !images)
        return kErrBadArgument;
    return mxfp6_launch(a_type == kDataTypeBf16 ? kSrcBf16 : kSrcFp16, images, w, nullptr, num_experts, n, k, stream);
}

int mxfp6_native_images(void *images, const void *elems, const void *scales, unsigned num_experts, unsigned n, unsigned k, hipStream_t stream) {
    if (const int rc = mxfp6_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (((uintptr_t)elems & 15) || ((uintptr_t)images & 255) || !elems || !scales || !images)
        return kErrBadArgument;
    return mxfp6_launch(kSrcOcp, images, elems, scales, num_experts, n, k, stream);
}

// host twins (offline conversion; bit-identical to the device kernel: tests/test_mxfp6_weights.py)
int mxfp6_quantize_weights_host(const void *w_, int a_type, unsigned num_experts, unsigned n, unsigned k, void *images) {
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrBadArgument;
    if (const int rc = mxfp6_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (!w_ || !images)
        return kErrBadArgument;
    const bool bf16 = a_type == kDataTypeBf16;
    const unsigned n32 = (n + 31) / 32 * 32;
    for (unsigned e = 0; e < num_experts; ++e) {
        const uint16_t *const w = (const uint16_t *)w_ + (size_t)e * n * k;
        unsigned char *const img = (unsigned char *)images + e * nv6_image_bytes(n, k);
        for (unsigned row = 0; row < n32; ++row)
            for (unsigned blk = 0; blk < k / 32; ++blk) {
                unsigned words[6] = {0u, 0u, 0u, 0u, 0u, 0u}, sbyte = 127u;
                if (row < n) {
                    const uint16_t *const v = w + (size_t)row * k + 32 * blk;
                    unsigned mx = 0;
                    for (int i = 0; i < 32; ++i)
                        mx = std::max(mx, v[i] & 0x7fffu);
                    sbyte = act_scale_byte<6>(h16_f32(bf16, mx));
                    for (unsigned i = 0; i < 32; ++i) { // element i at bits [6 i, 6 i + 6); the quotient is exact in f64
                        const uint64_t code = e2m3_rne(std::ldexp((double)h16_f32(bf16, v[i]), 127 - (int)sbyte));
                        const unsigned bit = 6 * i;
                        words[bit / 32] |= (unsigned)(code << (bit % 32));
                        if (bit % 32 > 26)
                            words[bit / 32 + 1] |= (unsigned)(code >> (32 - bit % 32));
                    }
                }
                mxfp6_place_host(img, n, k, row, blk, words, sbyte);
            }
    }
    return kOk;
}

int mxfp6_native_images_host(void *images, const void *elems, const void *scales, unsigned num_experts, unsigned n, unsigned k) {
    if (const int rc = mxfp6_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (!elems || !scales || !images)
        return kErrBadArgument;
    const unsigned n32 = (n + 31) / 32 * 32;
    for (unsigned e = 0; e < num_experts; ++e) {
        const unsigned char *const el = (const unsigned char *)elems + (size_t)e * n * (k / 4 * 3);
        const unsigned char *const sc = (const unsigned char *)scales + (size_t)e * n * (k / 32);
        unsigned char *const img = (unsigned char *)images + e * nv6_image_bytes(n, k);
        for (unsigned row = 0; row < n32; ++row)
            for (unsigned blk = 0; blk < k / 32; ++blk) {
                unsigned words[6] = {0u, 0u, 0u, 0u, 0u, 0u}, sbyte = 127u;
                if (row < n) {
                    const size_t b = (size_t)row * (k / 32) + blk;
                    memcpy(words, el + b * 24, 24);
                    sbyte = sc[b];
                }
                mxfp6_place_host(img, n, k, row, blk, words, sbyte);
            }
    }
    return kOk;
}

} // namespace petit_amd
