// gemm_native_invariant_host.h -- the host side of the batch-invariant GEMM on the native class (include/petit_amd.h "Batch-invariant GEMM on
// the native class") that needs no GPU: the form switch, the workspace arithmetic, the argument checks, the decode of "petit-qact/1" bytes and the
// CPU twin.  Plain C++ (no HIP) next to gemm_invariant_host.h, whose geometry and 16-bit / e2m1 / e8m0 helpers it uses: the same lines build into
// libpetit_amd.so (gemm_native_invariant.hip) and into a stand-alone program for sanitizer runs (tools/native_invariant_hostcheck.cc).
#pragma once

#include <stdlib.h>

#include "gemm_invariant_host.h"

namespace petit_amd {
namespace native_invariant {

namespace inv = invariant;

constexpr unsigned kSplitMaxM = 64;      // the largest M of the split form: two m-tiles of 32 (a constant of the library, measured: profiles/native_invariant.md)
constexpr unsigned kMaxQuantRows = 65535; // the library's own quantiser takes one grid row per activation row

// The form switch.  PETIT_NATIVE_INV_MEASURE_FORMS: a measurement-only build (tools/native_invariant_bench.py --forms-lib) reads it from the
// environment per call, so that one session can time both forms at one M; never defined in a shipped library, where it is the constant.
inline unsigned split_max_m() {
#ifdef PETIT_NATIVE_INV_MEASURE_FORMS
    if (const char *e = getenv("PETIT_NATIVE_INV_SPLIT_MAX_M"))
        return (unsigned)atoi(e);
#endif
    return kSplitMaxM;
}

inline bool format_ok(int act_format) { return act_format == 8 || act_format == 6 || act_format == 4; }

// bytes of the "petit-qact/1" image of (m, k, format): elements, then one E8M0 byte per 32 k (native32_ws_bytes, gemm_native32.hpp)
inline uint64_t qact_bytes(unsigned m, unsigned k, int act_format) { return (uint64_t)m * (k / 8 * (unsigned)act_format) + (uint64_t)m * (k / 32); }
inline uint64_t round256(uint64_t x) { return (x + 255) / 256 * 256; }

// every refusal that depends on shape, types and formats alone (kRcOk: the call can run): the dense invariant entry's rules for MXFP4 weights,
// without its refusal of fp16 activations -- the instruction takes any E8M0 byte
inline int shape_rc(unsigned m, unsigned n, unsigned k, int a_type, int act_format, int a_is_quantized, int activation) {
    if ((a_type != inv::kTypeBf16 && a_type != inv::kTypeFp16) || !format_ok(act_format) || activation < 0 || activation > 2)
        return inv::kRcBadArgument;
    if (n == 0 || k == 0 || n % 32 != 0 || k % 256 != 0 || m >= inv::kMaxRows || (activation && n % 64 != 0) || (uint64_t)k * 128 >= (1ull << 31))
        return inv::kRcProblemShape;
    if (!a_is_quantized && m > kMaxQuantRows)
        return inv::kRcKernelShape; // (quantise such a matrix in pieces and pass the bytes)
    return inv::kRcOk;
}

inline unsigned slabs(unsigned m, unsigned n, unsigned k, int a_type) {
    unsigned S, L;
    inv::geometry(n, k, a_type, inv::kTypeMx, &S, &L);
    return m <= split_max_m() ? S : 1u;
}

// the two parts of the workspace, each rounded up to 256: the quantised bytes (16-bit input only), then the slabs (split form only)
inline uint64_t quant_part_bytes(unsigned m, unsigned k, int act_format, int a_is_quantized) {
    return a_is_quantized ? 0 : round256(qact_bytes(m, k, act_format));
}
inline uint64_t slab_part_bytes(unsigned m, unsigned n, unsigned k, int a_type) {
    return m <= split_max_m() ? round256((uint64_t)slabs(m, n, k, a_type) * m * n * 4) : 0;
}
inline uint64_t workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int act_format, int a_is_quantized) {
    if (shape_rc(m, n, k, a_type, act_format, a_is_quantized, 0) != inv::kRcOk || m == 0)
        return 0;
    return quant_part_bytes(m, k, act_format, a_is_quantized) + slab_part_bytes(m, n, k, a_type);
}

// ---- "petit-qact/1" ------------------------------------------------------------------------------------------------------------------------

inline float e4m3_elem(unsigned b) { return inv::e4m3_f32(b); }
inline float e2m3_elem(unsigned c) { // sign, 2 exponent bits (bias 1), 3 mantissa bits; subnormal step 1/8
    const unsigned e = (c >> 3) & 3u, m = c & 7u;
    const float v = e == 0 ? (float)m * 0.125f : (1.0f + (float)m * 0.125f) * (float)(1u << (e - 1));
    return (c & 32u) ? -v : v;
}

// element (row, kk) of the image, WITHOUT its block scale, and the block's E8M0 byte (layouts: gemm_native32.hpp)
inline float qact_element(const uint8_t *qa, unsigned m, unsigned k, int act_format, unsigned row, unsigned kk) {
    const unsigned kt = kk / 128, b = (kk % 128) / 32, i = kk % 32;
    const size_t tile_row = (size_t)kt * m + row;
    if (act_format == 8) {
        const unsigned col16 = (kk % 128) / 8, u16 = col16 >> 1, half = col16 & 1u;
        const unsigned pos = (u16 & 4u) | ((u16 & 1u) << 1) | ((u16 >> 1) & 1u);
        return e4m3_elem(qa[tile_row * 128 + pos * 16 + half * 8 + kk % 8]);
    }
    if (act_format == 4) {
        const unsigned byte = qa[tile_row * 64 + 16 * b + i / 2];
        return inv::e2m1_f32((byte >> (4 * (i & 1u))) & 15u);
    }
    // MXFP6: the block's 24 bytes = 16 in the first image, 8 in the second (blocks 0, 2, 1, 3); element i at bits [6 i, 6 i + 6)
    const uint8_t *const lo = qa + tile_row * 64 + 16 * b;
    const uint8_t *const hi = qa + (size_t)m * (k / 2) + tile_row * 32 + 8 * ((b & 1u) * 2 + (b >> 1));
    const unsigned bit = 6 * i;
    auto byte_at = [&](unsigned j) -> unsigned { return j < 16 ? lo[j] : hi[j - 16]; };
    unsigned v = byte_at(bit / 8) >> (bit % 8);
    if (bit % 8 > 2)
        v |= byte_at(bit / 8 + 1) << (8 - bit % 8);
    return e2m3_elem(v & 63u);
}
inline unsigned qact_scale_byte(const uint8_t *qa, unsigned m, unsigned k, int act_format, unsigned row, unsigned blk) {
    return qa[(size_t)m * (k / 8 * (unsigned)act_format) + ((size_t)(blk / 4) * m + row) * 4 + blk % 4];
}
// 2^(b - 127) as a double (exact for every byte; byte 0 as e8m0_f32 reads it, 2^-127)
inline double e8m0_f64(unsigned b) { return (double)inv::e8m0_f32(b); }

// ---- the CPU twin --------------------------------------------------------------------------------------------------------------------------
// c = round16(((p_0 + p_1) + ... + p_{S-1}) * gs + bias) on HOST "petit-qact/1" bytes; p_s a sequential fp32 sum of a_q * w over the slice's k
// ascending, every product formed exactly (f64) and rounded once to fp32 (the device's p_s is a chain of the block-scaled MFMA: the same value
// whenever the partial sums are exact).  Activation none; global_scale and bias may be null.
inline int gemm_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scale, const void *bias, unsigned m, unsigned n,
                     unsigned k, int a_type, int act_format) {
    const int rc = shape_rc(m, n, k, a_type, act_format, 1, 0);
    if (rc != inv::kRcOk)
        return rc;
    if (m == 0)
        return inv::kRcOk;
    if (!c || !qa || !b || !scales)
        return inv::kRcProblemShape;
    const bool bf16 = a_type == inv::kTypeBf16;
    unsigned S, L;
    inv::geometry(n, k, a_type, inv::kTypeMx, &S, &L);
    const uint8_t *const q8 = (const uint8_t *)qa;
    const uint16_t *const b16 = (const uint16_t *)bias;
    uint16_t *const c16 = (uint16_t *)c;
    std::vector<double> wrow(k), arow((size_t)m * k);
    for (unsigned row = 0; row < m; ++row)
        for (unsigned kk = 0; kk < k; ++kk)
            arow[(size_t)row * k + kk] =
                (double)qact_element(q8, m, k, act_format, row, kk) * e8m0_f64(qact_scale_byte(q8, m, k, act_format, row, kk / 32));
    for (unsigned col = 0; col < n; ++col) {
        for (unsigned kk = 0; kk < k; ++kk) {
            const uint32_t word = ((const uint32_t *)b)[packed_weight_word_index(k, col, kk / 8)];
            wrow[kk] = (double)inv::e2m1_f32((word >> (4 * (kk % 8))) & 15u) *
                       e8m0_f64(((const uint8_t *)scales)[packed_mxscale_byte_index(k, col, kk / kMxGroup)]);
        }
        for (unsigned row = 0; row < m; ++row) {
            const double *const ar = &arow[(size_t)row * k];
            float y = 0.f;
            for (unsigned s = 0; s < S; ++s) {
                const unsigned k_end = (s + 1) * L < k ? (s + 1) * L : k;
                volatile float p = 0.f; // (volatile: one rounding per step, whatever the compiler's contraction setting)
                for (unsigned kk = s * L; kk < k_end; ++kk) {
                    volatile float t = (float)(ar[kk] * wrow[kk]);
                    p = p + t;
                }
                y = s ? y + p : p;
            }
            if (global_scale) {
                volatile float t = y * *global_scale;
                y = t;
            }
            if (bias)
                y = y + inv::h16_f32(bf16, b16[col]);
            c16[(size_t)row * n + col] = (uint16_t)inv::f32_h16(bf16, y);
        }
    }
    return inv::kRcOk;
}

} // namespace native_invariant
} // namespace petit_amd
