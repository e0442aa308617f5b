// nvnative.hip -- the MFMA-native image of NVFP4 weights ("petit-cdna4-nv6/1", layout.h), built from the packed tensors the exact kernels read
// (petit_repack_nvfp4_weights / _scales) once at load time, or per call into the call's workspace (petit_gemm_nvfp4_native_transient: then the builder
// is on the hot path), consumed by the WF = 6 instances of gemm_native32.hpp.
//
// Why an image and not a conversion inside the GEMM (VERDICT r05 item 1 asked for the in-kernel form first): NVFP4 is
//   w[n][k] = fp4(q[n][k]) x e4m3(s[n][k / 16]) x global_scale
// and the block-scaled MFMA takes ONE power-of-two scale per 32 k.  The e4m3 mantissa has to be multiplied into the elements, which the hardware
// converts cannot do (v_cvt_scalef32_pk_*_fp4 reads the scale's exponent only): fp4 -> f32 (1 op / 2 weights), x scale (1 / 2), -> fp6 (the
// 32-wide convert: ~1 / 16) plus the block maximum and the exponent arithmetic -- the ISA of nv6_image_kernel below is ~1.3 VALU lane-ops per weight.
// A 256 x 256 workgroup tile would spend ~340 wave-instructions per SIMD and k-tile on it next to 1024 (FP4 rate) / 2048 (FP8 rate) cycles of
// MFMA -- 0.7-1.3 of the MFMA time at ~4-8 cycles per instruction, under the same 1400 W cap that already holds the exact kernels (12 VALU per
// 8 weights, per WAVE) at 0.46 of the bf16 peak; gemm_shared.hpp is that organisation (unpack once per workgroup into LDS) for bf16 and gains
// only on gate_up.  Prefill is compute-bound, so the bytes of the image cost nothing there, and 288 GB of HBM3E hold it easily
// (Llama-3-70B at TP = 8: 4.9 GB packed NVFP4 + 6.8 GB image per GPU); decode (M <= 16) keeps reading the 4.5-bit packed tensors.
//
// Encoding of one 32-k block of one weight row (v_e = fp4 x e4m3, exact in f32):
//   E = floor(log2(max |v_e|)) - 2,  scale byte = E + 127 (127 for an all-zero block),  element_e = RNE_e2m3(v_e / 2^E)  (hardware:
//   v_cvt_scalef32_2xpk16_fp6_f32; host twin below, bit-identical).  The block maximum lands in [4, 8) and every product of an fp4
//   significand {1, 1.5} with an e4m3 significand {1 .. 1.875} below 8 is <= 7.5: the maximum never saturates.  What is lost: fp4 x e4m3 has
//   up to 6 significant bits, e2m3 keeps 4 (and a group whose own scale is 2^-d of the block's larger one keeps 4 - d): on weights quantised
//   by the checkpoint recipe 22-38 % of the elements move, by 2.3 % rms of the weight -- the weight's total quantisation error goes from 9.51 %
//   to 9.79 % of its rms (profiles/r06_nv6_reencode.md; FP8 e4m3 elements: 9.73 %, at 8 bits and the FP8 rate for every activation format).
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

// the block's values and its E8M0 byte from the lane's 16 bytes of nibbles (word j nibble i = element 8 j + i) and its two group scales
PETIT_HD unsigned block_values(const unsigned w[4], unsigned s_lo, unsigned s_hi, float v[32]) {
    const bool nan_lo = e4m3_is_nan(s_lo);
    const float sl = e4m3_finite_f32(s_lo);
    const bool nan_hi = e4m3_is_nan(s_hi);
    const float sh = e4m3_finite_f32(s_hi);
    float amax = 0.f;
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 8; ++i) {
            const float x = e2m1_f32((w[j] >> (4 * i)) & 15u) * (j < 2 ? sl : sh);
            v[8 * j + i] = x;
            const float ax = x < 0.f ? -x : x;
            amax = ax > amax ? ax : amax;
        }
    if (nan_lo || nan_hi) { // outside the class's contract (the reference: "scales positive", README.md:25): the block reads as NaN-scaled zeros
        for (int e = 0; e < 32; ++e)
            v[e] = 0.f;
        return 0xffu;
    }
    return act_scale_byte_nv6(amax); // (amax >= 2^-10: never an f32 subnormal; the byte is in 115 .. 136 for every e4m3 scale)
}

} // namespace

#if defined(__HIP_DEVICE_COMPILE__)
// 2 KS bytes (a scale record of one lane for one span) as KS / 2 dwords, one vector load / store
template <int KS> __device__ __forceinline__ void load_rec(unsigned (&d)[KS / 2], const unsigned char *p) {
    if constexpr (KS == 8) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(p);
        d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
    } else if constexpr (KS == 4) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        d[0] = v.x, d[1] = v.y;
    } else {
        d[0] = *reinterpret_cast<const unsigned *>(p);
    }
}
template <int KS> __device__ __forceinline__ void store_rec(unsigned char *p, const unsigned (&d)[KS / 2]) {
    if constexpr (KS == 8) {
        *reinterpret_cast<u32x4 *>(p) = u32x4{d[0], d[1], d[2], d[3]};
    } else if constexpr (KS == 4) {
        uint2 v;
        v.x = d[0], v.y = d[1];
        *reinterpret_cast<uint2 *>(p) = v;
    } else {
        *reinterpret_cast<unsigned *>(p) = d[0];
    }
}

// One 32-k block: its 6 FP6 words and its E8M0 byte from the lane's 16 bytes of nibbles and the two group scale bytes -- block_values + the
// hardware convert, bit for bit.  The nibbles go through the hardware E2M1 convert (exact, sign of zero kept) and the exact products are the
// values block_values forms; their maximum is taken with abs-modifier max3 (products are canonical floats: no canonicalising moves).
__device__ __forceinline__ unsigned nv6_block(const u32x4 w, unsigned s_lo, unsigned s_hi, unsigned (&words)[6]) {
    const bool nan_lo = e4m3_is_nan(s_lo);
    const float sl = e4m3_finite_f32(s_lo);
    const bool nan_hi = e4m3_is_nan(s_hi);
    const float sh = e4m3_finite_f32(s_hi);
    f32x16v ea, eb; // element 2 t = ea[t], 2 t + 1 = eb[t] (tools/probes/mfma32_fp6_probe.hip); word j, byte sel = elements 8 j + 2 sel, + 1
    float amax = 0.f;
    static_for<0, 16>([&](auto T) {
        constexpr int t = decltype(T)::value;
        const f32x2 p = cvt_fp4_f32<t % 4>(w[t / 4], 1.0f);
        const float s = t < 8 ? sl : sh;
        const float x = p[0] * s, y = p[1] * s;
        ea[t] = x, eb[t] = y;
        amax = fmaxf(amax, fmaxf(fabsf(x), fabsf(y)));
    });
    const unsigned sbyte = act_scale_byte_nv6(amax);
    const u32x6 qv = cvt_2xpk16_fp6_f32(ea, eb, bits_f32(sbyte << 23)); // (early-clobber form: device_common.hpp)
    const bool nan = nan_lo || nan_hi; // (block_values: NaN-scaled zeros, scale byte 0xff)
#pragma unroll
    for (int d = 0; d < 6; ++d)
        words[d] = nan ? 0u : (unsigned)qv[d];
    return nan ? 0xffu : sbyte;
}

// The builder, organised around the packed layout (layout.h): one wave = one (32-row block b, span sp of KS k-tiles).  Lane l = 32 h + r owns row
// 32 b + r and, of every k-tile of the span, the blocks g = h (image plane 0) and g = 2 + h (plane 1) -- exactly its lane of the image tile.  Its
// weight reads are one dwordx4 per block, contiguous across lanes within the two 1 KiB packed tiles of the block; its NV scales for the span are
// one 2 KS-byte record per block (the packed scale layout's own record); its E8M0 bytes for the span collect in registers and leave as one
// 2 KS-byte store (the image's scale record); the planes leave as three 16-byte stores per k-tile.  Rows >= N (N % 32 == 16: the upper half of
// the last block) read nothing and produce what the host twin writes (zero elements, scale byte 127).  Vector stores only.
template <int KS>
__device__ __forceinline__ void nv6_item(unsigned char *__restrict__ img, const u32x4 *__restrict__ pw, const unsigned char *__restrict__ ps, unsigned n,
                                         unsigned k, unsigned item) {
    const unsigned lane = threadIdx.x % 64, h = lane / 32, r = lane % 32;
    const unsigned ktiles = k / kTileK, nspans = ktiles / KS;
    unsigned char *const sc = img + nv6_elem_bytes(n, k);
    const unsigned b32 = item / nspans, sp = item % nspans;
    const unsigned row = b32 * 32 + r, nt = row / 16, rr = row % 16;
    const bool live = row < n;
    // packed inputs: tile (nt, kt) lane 16 g + rr (weights), record (nt, sp) lane 16 g + rr (scales), for g = h (q = 0) and g = 2 + h (q = 1)
    unsigned rec[2][KS / 2];
    u32x4 w[KS][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned g = 2 * q + h;
        if (live) {
            load_rec<KS>(rec[q], ps + (((size_t)nt * nspans + sp) * 64 + g * 16 + rr) * (2 * KS));
#pragma unroll
            for (int t = 0; t < KS; ++t)
                w[t][q] = pw[((size_t)nt * ktiles + sp * KS + t) * 64 + g * 16 + rr];
        } else {
#pragma unroll
            for (int d = 0; d < KS / 2; ++d)
                rec[q][d] = 0u;
#pragma unroll
            for (int t = 0; t < KS; ++t)
                w[t][q] = u32x4{0u, 0u, 0u, 0u};
        }
    }
    unsigned out_rec[KS / 2];
#pragma unroll
    for (int d = 0; d < KS / 2; ++d)
        out_rec[d] = 0u;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
        unsigned words[2][6];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const unsigned sw = rec[q][t / 2] >> (16 * (t % 2)); // bytes [t][0 .. 1] of the record: the block's two group scales
            const unsigned sbyte = nv6_block(w[t][q], sw & 0xffu, (sw >> 8) & 0xffu, words[q]);
            out_rec[(q * KS + t) / 4] |= sbyte << (8 * ((q * KS + t) % 4)); // image record byte [q][t]
        }
        unsigned char *const tile = img + ((size_t)b32 * ktiles + sp * KS + t) * kNv6TileBytes + lane * 16;
        *reinterpret_cast<u32x4 *>(tile) = u32x4{words[0][0], words[0][1], words[0][2], words[0][3]};
        *reinterpret_cast<u32x4 *>(tile + 1024) = u32x4{words[1][0], words[1][1], words[1][2], words[1][3]};
        *reinterpret_cast<u32x4 *>(tile + 2048) = u32x4{words[0][4], words[0][5], words[1][4], words[1][5]};
    }
    store_rec<KS>(sc + (((size_t)b32 * nspans + sp) * 64 + lane) * (2 * KS), out_rec);
}
#endif

template <int KS>
__global__ __launch_bounds__(256) void nv6_image_kernel(unsigned char *__restrict__ img, const u32x4 *__restrict__ pw, const unsigned char *__restrict__ ps,
                                                        unsigned n, unsigned k, unsigned items) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (unsigned item = blockIdx.x * 4 + threadIdx.x / 64; item < items; item += gridDim.x * 4)
        nv6_item<KS>(img, pw, ps, n, k, item);
#endif
}

// The images of E stacked experts in ONE launch (petit_nvfp4_native_images; the front of petit_gemm_native_moe_transient's workspace): the same
// work item, the item index running over E x per_expert -- item / per_expert is the expert, whose packed slice starts n k / 2 (weights) and
// n k / 16 (scales) bytes after its predecessor's and whose image starts nv6_image_bytes(n, k) after it: the layout gemm_moe_native.hpp reads.
// With `offsets` (the MoE launch's expert_offsets, a device array the host never reads) an item of an expert WITHOUT ROWS returns before any load
// or store: its image region stays as it was, and the MoE launch never reads it (its slots map to experts with rows only).  "Without rows" is
// moe_expert_rows (petit_internal.h) == 0, the predicate of moe_locate (gemm_moe.hpp).  Its lower end is a running maximum over every earlier
// offset, so two loads per item decide only well-formed offsets; to agree with the MoE launch on malformed ones as well, the wave keeps the
// running maximum along its (ascending) items: each offset is loaded once per wave, 64 at a time, and reduced across the lanes.  Wave-uniform:
// the expert of an item is, so every lane takes the same side.
template <int KS>
__global__ __launch_bounds__(256) void nv6_images_kernel(unsigned char *__restrict__ img, const unsigned char *__restrict__ pw,
                                                         const unsigned char *__restrict__ ps, unsigned n, unsigned k, unsigned per_expert, unsigned items,
                                                         const int *__restrict__ offsets, unsigned m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned lane = threadIdx.x % 64;
    const size_t image_bytes = nv6_image_bytes(n, k), w_bytes = (size_t)n * k / 2, s_bytes = (size_t)n * k / 16;
    unsigned seen = 0, lo = 0; // lo = the maximum of the clamped offsets[0 .. seen - 1]
    for (unsigned item = blockIdx.x * 4 + threadIdx.x / 64; item < items; item += gridDim.x * 4) {
        const unsigned e = __builtin_amdgcn_readfirstlane(item / per_expert);
        if (offsets) {
            for (; seen <= e; seen += 64) { // (the last chunk stops at e: the lanes past it add nothing)
                unsigned v = seen + lane <= e ? moe_offset_clamped(offsets[seen + lane], m) : 0u;
#pragma unroll
                for (unsigned d = 32; d >= 1; d /= 2)
                    v = max(v, (unsigned)__shfl_xor(v, d));
                lo = max(lo, (unsigned)__builtin_amdgcn_readfirstlane(v));
            }
            seen = e + 1;
            if (moe_expert_rows(lo, offsets[e + 1], m) == 0)
                continue;
        }
        nv6_item<KS>(img + e * image_bytes, reinterpret_cast<const u32x4 *>(pw + e * w_bytes), ps + e * s_bytes, n, k, item - e * per_expert);
    }
#endif
}

namespace {
// the shapes the image takes (0: nothing to do)
int nv6_shape(unsigned n, unsigned k) {
    if (n % kTileN || k % 256)
        return kErrProblemShape;
    if (nv6_elem_bytes(n, k) >= (1ull << 32))
        return kErrProblemShape; // (the kernels address the element part through one 32-bit buffer descriptor)
    return kOk;
}
// a grid-stride loop over the waves' items: at most one full occupancy of the device's CUs (4 waves per workgroup, 32 waves per CU)
unsigned nv6_blocks(unsigned items) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned cap = (unsigned)arch_info(dev).num_cus * 8u;
    return std::min((items + 3) / 4, cap);
}
} // namespace

int nv6_image(void *image, const void *pw, const void *ps, unsigned n, unsigned k, hipStream_t stream) {
    if (n == 0 || k == 0)
        return kOk;
    if (const int rc = nv6_shape(n, k))
        return rc;
    const int ks = span_tiles_for_k(k);
    const unsigned items = (n + 31) / 32 * (k / (kTileK * ks)); // (< 2^32 / 3072: the element bytes above)
    const auto kern = ks == 8 ? nv6_image_kernel<8> : ks == 4 ? nv6_image_kernel<4> : nv6_image_kernel<2>;
    hipLaunchKernelGGL(kern, dim3(nv6_blocks(items)), dim3(256), 0, stream, (unsigned char *)image, (const u32x4 *)pw, (const unsigned char *)ps, n, k,
                       items);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// E images back to back from the stacked packed tensors, one launch; offsets (device, may be null: every expert) / m: the routing skip above
int nv6_images(void *images, const void *pw, const void *ps, unsigned num_experts, unsigned n, unsigned k, const int32_t *offsets, unsigned m,
               hipStream_t stream) {
    if (num_experts == 0 || num_experts > kMoeMaxExperts)
        return kErrProblemShape;
    if (n == 0 || k == 0 || (offsets && m == 0))
        return kOk;
    if (const int rc = nv6_shape(n, k))
        return rc;
    const int ks = span_tiles_for_k(k);
    const unsigned per_expert = (n + 31) / 32 * (k / (kTileK * ks));
    const unsigned items = num_experts * per_expert; // (< 2^10 x 2^32 / 3072)
    const auto kern = ks == 8 ? nv6_images_kernel<8> : ks == 4 ? nv6_images_kernel<4> : nv6_images_kernel<2>;
    hipLaunchKernelGGL(kern, dim3(nv6_blocks(items)), dim3(256), 0, stream, (unsigned char *)images, (const unsigned char *)pw,
                       (const unsigned char *)ps, n, k, per_expert, items, (const int *)offsets, m);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// host twin (offline conversion; bit-identical to the device kernel: tests/test_gpu_parity.py::test_nv6_image_device_equals_host)
int nv6_image_host(void *image, const void *pw_, const void *ps_, unsigned n, unsigned k) {
    if (n == 0 || k == 0)
        return kOk;
    if (const int rc = nv6_shape(n, k))
        return rc;
    unsigned char *const img = (unsigned char *)image;
    const unsigned *const pw = (const unsigned *)pw_;
    const unsigned char *const ps = (const unsigned char *)ps_;
    unsigned char *const sc = img + nv6_elem_bytes(n, k);
    memset(img, 0, nv6_elem_bytes(n, k));
    const unsigned n32 = (n + 31) / 32 * 32;
    for (unsigned row = 0; row < n32; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            const unsigned kt = blk / 4, q = (blk % 4) >> 1, h = blk & 1u;
            unsigned words[6] = {0u, 0u, 0u, 0u, 0u, 0u}, sbyte = 127u;
            if (row < n) {
                const unsigned *const w = pw + packed_weight_word_index(k, row, 4 * blk);
                const size_t si = packed_nvscale_byte_index(k, row, 2 * blk);
                float v[32];
                sbyte = block_values(w, ps[si], ps[si + 1], v);
                const float inv = std::ldexp(1.0f, 127 - (int)(sbyte == 0xffu ? 127u : sbyte));
                for (int e = 0; e < 32; ++e) {
                    const unsigned code = e2m3_rne(v[e] * inv); // (the hardware convert's rounding: numfmt.h)
                    const unsigned bit = 6u * (unsigned)e;
                    const uint64_t bits = (uint64_t)code << (bit % 32);
                    words[bit / 32] |= (unsigned)bits;
                    if (bit % 32 > 26)
                        words[bit / 32 + 1] |= (unsigned)(bits >> 32);
                }
            }
            unsigned char *const tile_base = img + ((size_t)(row / 32) * (k / kTileK) + kt) * kNv6TileBytes;
            const unsigned lane_img = h * 32 + row % 32;
            memcpy(tile_base + q * 1024 + lane_img * 16, words, 16);
            memcpy(tile_base + 2048 + lane_img * 16 + q * 8, words + 4, 8);
            sc[nv6_scale_offset(k, row, blk)] = (unsigned char)sbyte;
        }
    return kOk;
}

// host twin of nv6_images: the same images, the same skip (offsets: HOST memory here) -- the regions of experts without rows are not touched
int nv6_images_host(void *images, const void *pw, const void *ps, unsigned num_experts, unsigned n, unsigned k, const int32_t *offsets, unsigned m) {
    if (num_experts == 0 || num_experts > kMoeMaxExperts)
        return kErrProblemShape;
    if (n == 0 || k == 0 || (offsets && m == 0))
        return kOk;
    if (const int rc = nv6_shape(n, k))
        return rc;
    unsigned lo = offsets ? moe_offset_clamped(offsets[0], m) : 0u;
    for (unsigned e = 0; e < num_experts; ++e) {
        if (offsets) {
            const unsigned rows = moe_expert_rows(lo, offsets[e + 1], m);
            lo += rows; // (the running maximum: the clamped upper end of expert e)
            if (rows == 0)
                continue;
        }
        if (const int rc = nv6_image_host((unsigned char *)images + e * nv6_image_bytes(n, k), (const unsigned char *)pw + (size_t)e * n * k / 2,
                                          (const unsigned char *)ps + (size_t)e * n * k / 16, n, k))
            return rc;
    }
    return kOk;
}

// Dense expansion of an image (test / debug aid, host): out[n][k] f32 = e2m3(element) x 2^(scale byte - 127), WITHOUT the global scale
int nv6_image_dequant_host(float *out, const void *image, unsigned n, unsigned k) {
    if (n % kTileN || k % 256)
        return kErrProblemShape;
    const unsigned char *const img = (const unsigned char *)image;
    const unsigned char *const sc = img + nv6_elem_bytes(n, k);
    for (unsigned row = 0; row < n; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            const unsigned kt = blk / 4, q = (blk % 4) >> 1, h = blk & 1u;
            const unsigned char *const tile_base = img + ((size_t)(row / 32) * (k / kTileK) + kt) * kNv6TileBytes;
            const unsigned lane_img = h * 32 + row % 32;
            unsigned words[6];
            memcpy(words, tile_base + q * 1024 + lane_img * 16, 16);
            memcpy(words + 4, tile_base + 2048 + lane_img * 16 + q * 8, 8);
            const unsigned sb = sc[nv6_scale_offset(k, row, blk)];
            const float scale = sb == 0xffu ? NAN : std::ldexp(1.0f, (int)sb - 127);
            for (unsigned e = 0; e < 32; ++e) {
                const unsigned bit = 6 * e;
                uint64_t wv = words[bit / 32];
                if (bit / 32 + 1 < 6)
                    wv |= (uint64_t)words[bit / 32 + 1] << 32;
                out[(size_t)row * k + 32 * blk + e] = e2m3_f32((unsigned)(wv >> (bit % 32)) & 63u) * scale;
            }
        }
    return kOk;
}

} // namespace petit_amd
