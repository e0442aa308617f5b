// native_image_readback.hip -- the MFMA-native image ("petit-cdna4-nv6/1", layout.h) read back on the device: dequantised to f32 / bf16 / fp16
// row-major weights, or exported without rounding as an OCP MXFP6 (e2m3) tensor; bit-identical host twins.  The rule is stated in
// include/petit_amd.h "Reading an image back".  The mirror of mxfp6_weights.hip: the same unit of work, the same staging, the other direction.
//
// ONE WORKGROUP owns one (32-row block b, span sp of KS k-tiles), the unit at which both parts of the image are contiguous (3072 KS element
// bytes, one 64 x 2 KS scale record); the transpose from "lane = row" to "along K" goes through LDS on the 0.75-byte-per-weight data:
//   load      thread t takes the 16-byte units t, t + 256, ... of the span's 192 KS units in image order (one contiguous run per workgroup);
//             the last wave also takes its lane's 2 KS scale bytes.  Every load is issued before the first use.
//   stage     lo[j][r] (registers 0-3 of block j of the span, row r) and hi[j][r] (registers 4-5, the scale byte, unused), 33 entries per j.
//             The writers of a wave are one (k-tile, plane) and the 64 lanes (h, r): 32 consecutive 16-byte entries of lo[j], then of lo[j + 1]
//             (plane 2: 8 bytes into every entry of hi[j] and hi[j + 2]: two lanes per bank, once per k-tile).  The readers of a wave are the
//             16 consecutive j of one row r (two rows at KS = 2), each entry read by the four lanes of its quad (one address, broadcast):
//             528 bytes = 4 banks apart, so 16 entries x 4 banks cover the banks once -- without the 33rd entry all 16 would start in one bank.
//   expand    a quad of lanes owns one 32-k block of one row.  16-bit: lane c takes elements 8 c .. 8 c + 7 (bits [48 c, 48 c + 48) of the block's
//             192); f32: elements 4 c .. 4 c + 3 and 16 + 4 c .. 16 + 4 c + 3, so that both of its stores join the quad's into 64 contiguous bytes.
//             A code is decoded in integer arithmetic to its magnitude in eighths (0 .. 60), converted (exact) and scaled by v_ldexp_f32: the
//             result is the rule's f32 number for every scale byte, subnormal and infinite ends included.  The hardware's 32-wide scaled FP6
//             converts are not used: a lane holds 8 codes, not 32.
//   store     row-major: a wave writes 16 consecutive blocks of a row (1 KiB of bf16 / fp16, 2 KiB of f32) in 16-byte stores; rows >= N store
//             nothing.  OCP: thread t owns whole blocks (three 8-byte stores and the scale byte), no arithmetic.
// Vector stores only, no scratch.
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

// the destination of the store stage
enum : int { kDstF32 = 0, kDstBf16 = 1, kDstFp16 = 2, kDstOcp = 3 };
constexpr int kDataTypeFp32 = 100; // PETIT_DTYPE_FP32

namespace {

// the rule, per element: e2m3(code) x 2^(sbyte - 127) as an f32 number (exact; 2^128 and above: infinity), times the expert's global scale as one
// f32 multiply when there is one.  Scale byte 255 (E8M0's NaN): the quiet NaN 0x7fc00000, whatever the code and the global scale.
PETIT_HD float nv6_value(unsigned code, unsigned sbyte, bool scaled, float gs) {
    const unsigned t = code & 31u, m = t & 7u;
    const unsigned eighths = t < 8u ? m : (m | 8u) << ((t >> 3) - 1u); // subnormal codes: m / 8; normal: (8 + m) / 8 x 2^(e - 1)
    const float v = bits_f32(f32_bits(ldexpf((float)eighths, (int)sbyte - 130)) | (code & 32u) << 26);
    if (sbyte == 255u)
        return bits_f32(0x7fc00000u);
    return scaled ? v * gs : v;
}

// the value in the destination's bits: f32, or RNE to bf16 / fp16 (numfmt.h)
template <int DST> PETIT_HD unsigned nv6_out_bits(float p) {
    if constexpr (DST == kDstF32)
        return f32_bits(p);
    else
        return f32_h16<DST == kDstBf16>(p);
}

} // namespace

#if defined(__HIP_DEVICE_COMPILE__)
namespace {
constexpr int kStageRows = 33; // entries per block of the span in lo / hi: 32 rows and the pad (file comment)

// bits [off, off + 48) of the 96 bits (a, b, d), off < 96 a multiple of 8: two funnel shifts
__device__ __forceinline__ uint64_t bits96(unsigned a, unsigned b, unsigned d, unsigned off) {
    const unsigned w0 = off < 32 ? a : off < 64 ? b : d, w1 = off < 32 ? b : off < 64 ? d : 0u, w2 = off < 32 ? d : 0u;
    return (uint64_t)__builtin_amdgcn_alignbit(w1, w0, off & 31u) | (uint64_t)__builtin_amdgcn_alignbit(w2, w1, off & 31u) << 32;
}
} // namespace
#endif

template <int KS, int DST>
__global__ __launch_bounds__(256) void nv6_readback_kernel(unsigned char *__restrict__ out, unsigned char *__restrict__ out_scales,
                                                           const unsigned char *__restrict__ images, const float *__restrict__ global_scales,
                                                           unsigned n, unsigned k, unsigned per_expert, unsigned items) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ u32x4 lo[4 * KS][kStageRows];
    __shared__ u32x4 hi[4 * KS][kStageRows];
    const unsigned tid = threadIdx.x;
    const unsigned ktiles = k / kTileK, nspans = ktiles / KS;
    const size_t image_bytes = nv6_image_bytes(n, k), elem_bytes = nv6_elem_bytes(n, k);
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned e = item / per_expert, rem = item % per_expert, b32 = rem / nspans, sp = rem % nspans;
        const unsigned char *const img = images + e * image_bytes;
        // ---- load stage: the span's units in image order and its scale record, every load before the first use
        constexpr int kUnits = (192 * KS + 255) / 256; // 192 KS units per item, 256 threads
        const unsigned char *const tiles = img + ((size_t)b32 * ktiles + (size_t)sp * KS) * kNv6TileBytes;
        u32x4 raw[kUnits];
#pragma unroll
        for (int i = 0; i < kUnits; ++i) {
            const unsigned v = i * 256 + tid;
            raw[i] = u32x4{0u, 0u, 0u, 0u};
            if (v < 192u * KS)
                raw[i] = *reinterpret_cast<const u32x4 *>(tiles + (size_t)v * 16);
        }
        unsigned rec[KS / 2];
        if (tid >= 192) { // the scale record of lane (r, h): byte [q][t] = the scale of block 4 t + 2 q + h of the span
            const unsigned char *const p = img + elem_bytes + (((size_t)b32 * nspans + sp) * 64 + (tid - 192)) * (2 * KS);
            if constexpr (KS == 8) {
                const u32x4 s = *reinterpret_cast<const u32x4 *>(p);
                rec[0] = s[0], rec[1] = s[1], rec[2] = s[2], rec[3] = s[3];
            } else if constexpr (KS == 4) {
                const uint2 s = *reinterpret_cast<const uint2 *>(p);
                rec[0] = s.x, rec[1] = s.y;
            } else {
                rec[0] = *reinterpret_cast<const unsigned *>(p);
            }
        }
        const float gs = global_scales ? global_scales[e] : 1.0f;
        // ---- stage: unit (t, plane, lane 32 h + r) is lo[4 t + 2 plane + h][r], or the .xy of hi[4 t + h][r] and hi[4 t + 2 + h][r]
#pragma unroll
        for (int i = 0; i < kUnits; ++i) {
            const unsigned v = i * 256 + tid, t = v / 192, plane = v % 192 / 64, lane = v % 64, h = lane / 32, r = lane % 32;
            if (v < 192u * KS) {
                if (plane < 2) {
                    lo[4 * t + 2 * plane + h][r] = raw[i];
                } else {
                    *reinterpret_cast<u32x2 *>(&hi[4 * t + h][r]) = u32x2{raw[i][0], raw[i][1]};
                    *reinterpret_cast<u32x2 *>(&hi[4 * t + 2 + h][r]) = u32x2{raw[i][2], raw[i][3]};
                }
            }
        }
        if (tid >= 192) {
            const unsigned lane = tid - 192, h = lane / 32, r = lane % 32;
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int t = 0; t < KS; ++t)
                    reinterpret_cast<unsigned *>(&hi[4 * t + 2 * q + h][r])[2] = (rec[(q * KS + t) / 4] >> (8 * ((q * KS + t) % 4))) & 0xffu;
        }
        __syncthreads();
        if constexpr (DST == kDstOcp) {
            // ---- store stage, OCP MXFP6: whole blocks, no arithmetic
            constexpr int kBlocks = KS / 2; // 128 KS blocks per item, 256 threads
            unsigned char *const el = out + (size_t)e * n * (k / 4 * 3);
            unsigned char *const sc = out_scales + (size_t)e * n * (k / 32);
#pragma unroll
            for (int i = 0; i < kBlocks; ++i) {
                const unsigned flat = i * 256 + tid, r = flat / (4 * KS), j = flat % (4 * KS), row = b32 * 32 + r;
                if (row < n) {
                    const u32x4 l = lo[j][r], u = hi[j][r];
                    const size_t blk = (size_t)row * (k / 32) + sp * KS * 4 + j;
                    u32x2 *const dst = reinterpret_cast<u32x2 *>(el + blk * 24);
                    dst[0] = u32x2{l[0], l[1]};
                    dst[1] = u32x2{l[2], l[3]};
                    dst[2] = u32x2{u[0], u[1]};
                    sc[blk] = (unsigned char)u[2];
                }
            }
        } else {
            // ---- expand and store: quad tid / 4 of iteration i owns block j of row r; a wave is 16 consecutive j
            constexpr unsigned kElem = DST == kDstF32 ? 4u : 2u;
            unsigned char *const dst_e = out + (size_t)e * n * k * kElem;
            const unsigned c = tid & 3u;
            const bool scaled = global_scales != nullptr;
#pragma unroll
            for (int i = 0; i < 2 * KS; ++i) {
                const unsigned quad = i * 64 + tid / 4, r = quad / (4 * KS), j = quad % (4 * KS), row = b32 * 32 + r;
                if (row < n) {
                    const u32x4 l = lo[j][r], u = hi[j][r];
                    const unsigned sbyte = u[2];
                    unsigned char *const dst = dst_e + ((size_t)row * k + (size_t)sp * KS * kTileK + j * 32) * kElem;
                    if constexpr (DST == kDstF32) {
                        // elements 4 c .. 4 c + 3 (registers 0-2) and 16 + 4 c .. 16 + 4 c + 3 (registers 3-5)
                        const unsigned g0 = (unsigned)bits96(l[0], l[1], l[2], 24 * c), g1 = (unsigned)bits96(l[3], u[0], u[1], 24 * c);
                        u32x4 o0, o1;
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            o0[d] = nv6_out_bits<DST>(nv6_value((g0 >> (6 * d)) & 63u, sbyte, scaled, gs));
                            o1[d] = nv6_out_bits<DST>(nv6_value((g1 >> (6 * d)) & 63u, sbyte, scaled, gs));
                        }
                        *reinterpret_cast<u32x4 *>(dst + 16 * c) = o0;
                        *reinterpret_cast<u32x4 *>(dst + 64 + 16 * c) = o1;
                    } else {
                        // elements 8 c .. 8 c + 7: registers 0-2 for lanes 0 / 1 of the quad, 3-5 for lanes 2 / 3
                        const bool up = (c & 2u) != 0;
                        const uint64_t g = bits96(up ? l[3] : l[0], up ? u[0] : l[1], up ? u[1] : l[2], 48 * (c & 1u));
                        u32x4 o;
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            const unsigned x = nv6_out_bits<DST>(nv6_value((unsigned)(g >> (12 * d)) & 63u, sbyte, scaled, gs));
                            const unsigned y = nv6_out_bits<DST>(nv6_value((unsigned)(g >> (12 * d + 6)) & 63u, sbyte, scaled, gs));
                            o[d] = (x & 0xffffu) | y << 16;
                        }
                        *reinterpret_cast<u32x4 *>(dst + 16 * c) = o;
                    }
                }
            }
        }
        __syncthreads(); // (the next item's stage writes)
    }
#endif
}

namespace {

// what the device forms and their host twins refuse, in one place and in this order: the shape, then (by the callers) nothing-to-do, then
// pointers.  The rule of the entries that write an image (mxfp6_weights.hip).
int readback_shape(unsigned num_experts, unsigned n, unsigned k) {
    if (num_experts == 0 || num_experts > kMoeMaxExperts)
        return kErrProblemShape;
    if (n % kTileN || k % 256)
        return kErrProblemShape;
    if (nv6_elem_bytes(n, k) >= (1ull << 32) || (uint64_t)num_experts * ((n + 31) / 32) * (k / 256) >= (1ull << 32))
        return kErrProblemShape; // (an image is what its consumers address through one 32-bit descriptor; the item count is 32-bit)
    return kOk;
}

int dst_of(int out_type) { return out_type == kDataTypeFp32 ? kDstF32 : out_type == kDataTypeBf16 ? kDstBf16 : out_type == kDataTypeFp16 ? kDstFp16 : -1; }

template <int DST> auto readback_kernel_for(int ks) {
    return ks == 8 ? nv6_readback_kernel<8, DST> : ks == 4 ? nv6_readback_kernel<4, DST> : nv6_readback_kernel<2, DST>;
}

int readback_launch(int dst, void *out, void *out_scales, const void *images, const float *global_scales, unsigned num_experts, unsigned n,
                    unsigned k, hipStream_t stream) {
    const int ks = span_tiles_for_k(k);
    const unsigned per_expert = (n + 31) / 32 * (k / (kTileK * ks)), items = num_experts * per_expert;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned cap = (unsigned)arch_info(dev).num_cus * 4u; // what the stage's LDS lets a CU hold at KS = 8; the workgroups stride over the rest
    const auto kern = dst == kDstF32    ? readback_kernel_for<kDstF32>(ks)
                      : dst == kDstBf16 ? readback_kernel_for<kDstBf16>(ks)
                      : dst == kDstFp16 ? readback_kernel_for<kDstFp16>(ks)
                                        : readback_kernel_for<kDstOcp>(ks);
    hipLaunchKernelGGL(kern, dim3(std::min(items, cap)), dim3(256), 0, stream, (unsigned char *)out, (unsigned char *)out_scales,
                       (const unsigned char *)images, global_scales, n, k, per_expert, items);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// one block of one row out of an image (host): registers 0-3, registers 4-5 and the scale byte from where the consumers read them
unsigned readback_block_host(const unsigned char *img, unsigned n, unsigned k, unsigned row, unsigned blk, unsigned (&words)[6]) {
    const unsigned kt = blk / 4, q = (blk % 4) >> 1, h = blk & 1u;
    memcpy(words, img + nv6_unit_offset(k, row, kt, q, h), 16);
    memcpy(words + 4, img + nv6_unit_offset(k, row, kt, 2, h) + q * 8, 8);
    return img[nv6_elem_bytes(n, k) + nv6_scale_offset(k, row, blk)];
}

template <int DST>
void dequant_host(void *out, const unsigned char *images, const float *global_scales, unsigned num_experts, unsigned n, unsigned k) {
    for (unsigned e = 0; e < num_experts; ++e) {
        const unsigned char *const img = images + e * nv6_image_bytes(n, k);
        const float gs = global_scales ? global_scales[e] : 1.0f;
        for (unsigned row = 0; row < n; ++row)
            for (unsigned blk = 0; blk < k / 32; ++blk) {
                unsigned words[6];
                const unsigned sbyte = readback_block_host(img, n, k, row, blk, words);
                for (unsigned i = 0; i < 32; ++i) { // element i at bits [6 i, 6 i + 6)
                    const unsigned bit = 6 * i;
                    uint64_t wv = words[bit / 32];
                    if (bit / 32 + 1 < 6)
                        wv |= (uint64_t)words[bit / 32 + 1] << 32;
                    const unsigned bits = nv6_out_bits<DST>(nv6_value((unsigned)(wv >> (bit % 32)) & 63u, sbyte, global_scales != nullptr, gs));
                    const size_t at = ((size_t)e * n + row) * k + 32 * blk + i;
                    if constexpr (DST == kDstF32)
                        ((uint32_t *)out)[at] = bits;
                    else
                        ((uint16_t *)out)[at] = (uint16_t)bits;
                }
            }
    }
}

} // namespace

int native_images_dequant(void *out, int out_type, const void *images, const float *global_scales, unsigned num_experts, unsigned n, unsigned k,
                          hipStream_t stream) {
    const int dst = dst_of(out_type);
    if (dst < 0)
        return kErrBadArgument;
    if (const int rc = readback_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (((uintptr_t)out & 15) || ((uintptr_t)images & 255) || ((uintptr_t)global_scales & 3) || !out || !images)
        return kErrBadArgument;
    return readback_launch(dst, out, nullptr, images, global_scales, num_experts, n, k, stream);
}

int mxfp6_export_images(void *elems, void *scales, const void *images, unsigned num_experts, unsigned n, unsigned k, hipStream_t stream) {
    if (const int rc = readback_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (((uintptr_t)elems & 15) || ((uintptr_t)images & 255) || !elems || !scales || !images)
        return kErrBadArgument;
    return readback_launch(kDstOcp, elems, scales, images, nullptr, num_experts, n, k, stream);
}

// host twins (offline conversion; bit-identical to the device kernel: tests/test_native_image_readback.py)
int native_images_dequant_host(void *out, int out_type, const void *images, const float *global_scales, unsigned num_experts, unsigned n,
                               unsigned k) {
    const int dst = dst_of(out_type);
    if (dst < 0)
        return kErrBadArgument;
    if (const int rc = readback_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (!out || !images)
        return kErrBadArgument;
    const unsigned char *const img = (const unsigned char *)images;
    if (dst == kDstF32)
        dequant_host<kDstF32>(out, img, global_scales, num_experts, n, k);
    else if (dst == kDstBf16)
        dequant_host<kDstBf16>(out, img, global_scales, num_experts, n, k);
    else
        dequant_host<kDstFp16>(out, img, global_scales, num_experts, n, k);
    return kOk;
}

int mxfp6_export_images_host(void *elems, void *scales, const void *images, unsigned num_experts, unsigned n, unsigned k) {
    if (const int rc = readback_shape(num_experts, n, k))
        return rc;
    if (n == 0 || k == 0)
        return kOk;
    if (!elems || !scales || !images)
        return kErrBadArgument;
    for (unsigned e = 0; e < num_experts; ++e) {
        unsigned char *const el = (unsigned char *)elems + (size_t)e * n * (k / 4 * 3);
        unsigned char *const sc = (unsigned char *)scales + (size_t)e * n * (k / 32);
        const unsigned char *const img = (const unsigned char *)images + e * nv6_image_bytes(n, k);
        for (unsigned row = 0; row < n; ++row)
            for (unsigned blk = 0; blk < k / 32; ++blk) {
                unsigned words[6];
                const size_t b = (size_t)row * (k / 32) + blk;
                sc[b] = (unsigned char)readback_block_host(img, n, k, row, blk, words);
                memcpy(el + b * 24, words, 24);
            }
    }
    return kOk;
}

} // namespace petit_amd
