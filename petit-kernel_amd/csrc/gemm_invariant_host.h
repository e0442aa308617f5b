// gemm_invariant_host.h -- the host side of the batch-invariant GEMM (include/petit_amd.h "Batch-invariant GEMM") that needs no GPU: the
// geometry, the form switch, the workspace arithmetic, the argument checks and the CPU twin.  Plain C++ (no HIP), so that the same lines build
// into libpetit_amd.so (gemm_invariant.hip, gemm_invariant_moe.hip) and into stand-alone programs for sanitizer runs
// (tools/gemm_invariant_hostcheck.cc, tools/moe_invariant_hostcheck.cc).  The routed-expert (MoE) launch's part is at the end.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "layout.h"

namespace petit_amd {
namespace invariant {

// (values of include/petit_amd.h, restated so that this header stands alone; gemm_invariant.hip static_asserts them against petit_internal.h)
enum : int { kRcOk = 0, kRcProblemShape = 1, kRcKernelShape = 2, kRcBadArgument = 4 };
enum : int { kTypeNv = 3, kTypeFp16 = 4, kTypeBf16 = 5, kTypeMx = 7, kTypeMxF16Range = 8 };
constexpr unsigned kMaxRows = 1u << 20;     // kMaxM of petit_internal.h
constexpr unsigned kMaxSlices = 16;         // S <= 16
constexpr unsigned kSliceStep = 256;        // L is a multiple of it: the packed scale layout exists for k % 256 == 0 only (layout.h)
constexpr unsigned kTargetWaves = 2048;     // the split form's waves at M <= 16: 8 per CU of a 256-CU chip (n-tiles x S of them)
constexpr unsigned kSplitMaxM = 32;         // the largest M of the split form

inline bool is_mx(int b_type) { return b_type == kTypeMx || b_type == kTypeMxF16Range; }

// S and L from (n, k): enough slices that the n-tiles x S waves of a decode call reach kTargetWaves, no more than kMaxSlices, none shorter
// than kSliceStep.  The types do not enter today; they are arguments so that they may.
inline void geometry(unsigned n, unsigned k, int /*a_type*/, int /*b_type*/, unsigned *slices, unsigned *slice_k) {
    const unsigned ntiles = n / 16 ? n / 16 : 1;
    unsigned want = (kTargetWaves + ntiles - 1) / ntiles;
    want = want > kMaxSlices ? kMaxSlices : want;
    const unsigned per = (k + want - 1) / want;
    unsigned L = (per + kSliceStep - 1) / kSliceStep * kSliceStep;
    L = L ? L : kSliceStep;
    *slice_k = L;
    *slices = k ? (k + L - 1) / L : 1u;
}

// every refusal that depends on shape and types alone (kRcOk: the call can run)
inline int shape_rc(unsigned m, unsigned n, unsigned k, int a_type, int b_type, int activation) {
    if ((a_type != kTypeBf16 && a_type != kTypeFp16) || (b_type != kTypeNv && !is_mx(b_type)) || activation < 0 || activation > 2)
        return kRcBadArgument;
    // (MXFP4: n % 32 == 0, as the routed-expert launches ask -- its processed scale tensor comes in rows of 32 weight rows)
    if (n == 0 || k == 0 || n % 16 != 0 || (is_mx(b_type) && n % 32 != 0) || k % 256 != 0 || m >= kMaxRows || (activation && n % 32 != 0) ||
        (uint64_t)k * 128 >= (1ull << 31))
        return kRcProblemShape;
    if (a_type == kTypeFp16 && is_mx(b_type))
        return kRcKernelShape; // out-of-range scale bytes need the hi / lo fallback body: a second chain, a definition of its own
    return kRcOk;
}

inline unsigned slabs(unsigned m, unsigned n, unsigned k, int a_type, int b_type, unsigned split_max_m = kSplitMaxM) {
    unsigned S, L;
    geometry(n, k, a_type, b_type, &S, &L);
    return m <= split_max_m ? S : 1u;
}

inline uint64_t workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int b_type, unsigned split_max_m = kSplitMaxM) {
    if (shape_rc(m, n, k, a_type, b_type, 0) != kRcOk || m == 0 || m > split_max_m)
        return 0;
    return ((uint64_t)slabs(m, n, k, a_type, b_type, split_max_m) * m * n * 4 + 255) / 256 * 256;
}

// the pointer checks of a call that passed shape_rc and has m > 0
inline int pointers_rc(const void *c, const void *a, const void *b, const void *scales, const void *bias, const void *workspace,
                       uint64_t workspace_need) {
    if (!c || !a || !b || !scales || (workspace_need && !workspace))
        return kRcProblemShape;
    if ((((uintptr_t)c | (uintptr_t)a | (uintptr_t)b | (uintptr_t)scales) & 15u) || ((uintptr_t)bias & 7u) ||
        (workspace_need && ((uintptr_t)workspace & 255u)))
        return kRcProblemShape;
    return kRcOk;
}

// ---- the CPU twin --------------------------------------------------------------------------------------------------------------------------

inline float bits_f32(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline uint32_t f32_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
inline float h16_f32(bool bf16, uint32_t h) {
    if (bf16)
        return bits_f32(h << 16);
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 0)
        return bits_f32(sign | f32_bits((float)m * (1.0f / 16777216.0f)));
    return bits_f32(sign | (e == 31 ? 0x7f800000u : (e + 112u) << 23) | (m << 13));
}
inline uint32_t f32_h16(bool bf16, float x) { // round to nearest even
    const uint32_t u = f32_bits(x);
    if (bf16) {
        if ((u & 0x7fffffffu) > 0x7f800000u)
            return (u >> 16) | 0x40u;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    }
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u)
        return sign | 0x7e00u;
    if (a >= 0x477ff000u)
        return sign | 0x7c00u;
    if (a < 0x38800000u)
        return sign | (f32_bits(bits_f32(a) * 16777216.0f + 8388608.0f) & 0x7fffffu);
    const uint32_t r = a - 0x38000000u;
    return sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);
}
inline float e2m1_f32(unsigned code) {
    static const float mag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    return (code & 8u) ? -mag[code & 7u] : mag[code & 7u];
}
inline float e4m3_f32(unsigned b) { // OCP e4m3 (fn): no infinities, 0x7f / 0xff are NaN
    const unsigned e = (b >> 3) & 15u, m = b & 7u;
    float v;
    if (e == 0)
        v = (float)m * (1.0f / 512.0f);
    else if (e == 15 && m == 7)
        v = bits_f32(0x7fc00000u);
    else
        v = bits_f32(((e + 120u) << 23) | (m << 20));
    return (b & 0x80u) ? -v : v;
}
// 2^(b - 127), as the kernels decode it (the hardware convert): byte 0 is 2^-127, an fp32 subnormal -- not the 0.0 of `b << 23`, which is what
// dequant.hip and the oracle restate from the reference --, byte 255 is `b << 23` = inf, whose product with any code or activation ends as NaN
inline float e8m0_f32(unsigned b) { return bits_f32((b & 0xffu) ? (b & 0xffu) << 23 : 0x00400000u); }

// the weight operand of the definition: fp4 x group scale, exact in the activation type for every (type, format) pair the entry accepts
inline float weight_value(const uint32_t *pw, const uint8_t *ps, bool mx, unsigned k_total, unsigned n, unsigned kk) {
    const uint32_t word = pw[packed_weight_word_index(k_total, n, kk / 8)];
    const float q = e2m1_f32((word >> (4 * (kk % 8))) & 15u);
    const float sc = mx ? e8m0_f32(ps[packed_mxscale_byte_index(k_total, n, kk / kMxGroup)])
                        : e4m3_f32(ps[packed_nvscale_byte_index(k_total, n, kk / kNvGroup)]);
    return q * sc;
}

// c = round16(((p_0 + p_1) + ... + p_{S-1}) * gs + bias), p_s a sequential fp32 sum over the slice's k ascending (the device's p_s is an MFMA
// chain: the same value whenever the partial sums are exact, a few ulp apart otherwise).  Host pointers; global_scale and bias may be null.
inline int gemm_host(void *c, const void *a, const void *b, const void *scales, const float *global_scale, const void *bias, unsigned m, unsigned n,
                     unsigned k, int a_type, int b_type) {
    const int rc = shape_rc(m, n, k, a_type, b_type, 0);
    if (rc != kRcOk)
        return rc;
    if (m == 0)
        return kRcOk;
    if (!c || !a || !b || !scales)
        return kRcProblemShape;
    const bool bf16 = a_type == kTypeBf16, mx = is_mx(b_type);
    unsigned S, L;
    geometry(n, k, a_type, b_type, &S, &L);
    const uint16_t *a16 = (const uint16_t *)a, *b16 = (const uint16_t *)bias;
    uint16_t *c16 = (uint16_t *)c;
    std::vector<float> wrow(k), arow(k);
    for (unsigned col = 0; col < n; ++col) {
        for (unsigned kk = 0; kk < k; ++kk)
            wrow[kk] = weight_value((const uint32_t *)b, (const uint8_t *)scales, mx, k, col, kk);
        for (unsigned row = 0; row < m; ++row) {
            float y = 0.f;
            for (unsigned s = 0; s < S; ++s) {
                const unsigned k_end = (s + 1) * L < k ? (s + 1) * L : k;
                volatile float p = 0.f; // (volatile: one rounding per step, whatever the compiler's contraction setting)
                for (unsigned kk = s * L; kk < k_end; ++kk) {
                    volatile float t = h16_f32(bf16, a16[(size_t)row * k + kk]) * wrow[kk];
                    p = p + t;
                }
                y = s ? y + p : p;
            }
            if (global_scale) {
                volatile float t = y * *global_scale;
                y = t;
            }
            if (bias)
                y = y + h16_f32(bf16, b16[col]);
            c16[(size_t)row * n + col] = (uint16_t)f32_h16(bf16, y);
        }
    }
    return kRcOk;
}

// ---- the routed-expert (MoE) launch (include/petit_amd.h "Batch-invariant MoE launch") -----------------------------------------------------

constexpr unsigned kMoeMaxExperts = 1024;      // kMoeMaxExperts of petit_internal.h
// The form switch's two constants, measured (profiles/moe_invariant.md): the whole form wins wherever the routing gives it workgroups enough to
// fill the chip -- from about 8 to 13 grouped rows on -- and by 2x and more from 64 rows; the split form wins at a decode step's 4 to 8 rows.
constexpr unsigned kMoeSplitMaxRowsPer = 8;    // split form: ceil(m / min(E, m)) <= this (the rows-per-active-expert estimate of the MoE pick) ...
constexpr unsigned kMoeSplitMaxM = 8;          // ... and m <= this (also the cap of the slab workspace S * m * n * 4); at 8 the first is implied

// the form switch: a function of (m, num_experts) alone.  Either form gives the same bits, so it is a speed choice only.
inline bool moe_split(unsigned m, unsigned num_experts) {
    const unsigned active = num_experts < m ? num_experts : m;
    if (active == 0)
        return true;
    return (m + active - 1) / active <= kMoeSplitMaxRowsPer && m <= kMoeSplitMaxM;
}

// workgroups of the larger launch of a call (one linear index in grid x)
inline uint64_t moe_grid(unsigned m, unsigned n, unsigned num_experts, unsigned slices, bool split, int activation) {
    const uint64_t active = num_experts < m ? num_experts : m, ntiles = n / 16;
    if (split)
        return ((m + 15ull) / 16 + active) * slices * ((ntiles + 3) / 4);
    const uint64_t pairs = activation ? ntiles / 2 : (ntiles + 1) / 2;
    return ((m + 63ull) / 64 + active) * ((pairs + 3) / 4);
}

// every refusal that depends on shape, types and counts alone
inline int moe_shape_rc(unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index, unsigned a_rows,
                        const int32_t *c_row_index, unsigned c_rows, int a_type, int b_type, int activation) {
    const int rc = shape_rc(m, n, k, a_type, b_type, activation);
    if (rc != kRcOk)
        return rc;
    if (num_experts == 0 || num_experts > kMoeMaxExperts)
        return kRcProblemShape;
    // a null index is the identity: the rows it would name must exist
    if ((!a_row_index && a_rows < m) || (!c_row_index && c_rows < m))
        return kRcProblemShape;
    // one descriptor bounds every A load, and the kernels' out-of-range voffset (2^31) must lie past its end
    if ((uint64_t)a_rows * k * 2 > (1ull << 31))
        return kRcProblemShape;
    unsigned S, L;
    geometry(n, k, a_type, b_type, &S, &L);
    if (moe_grid(m, n, num_experts, S, moe_split(m, num_experts), activation) >= (1ull << 31))
        return kRcProblemShape;
    return kRcOk;
}

inline uint64_t moe_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    if (shape_rc(m, n, k, a_type, b_type, 0) != kRcOk || num_experts == 0 || num_experts > kMoeMaxExperts || m == 0 || !moe_split(m, num_experts))
        return 0;
    unsigned S, L;
    geometry(n, k, a_type, b_type, &S, &L);
    return ((uint64_t)S * m * n * 4 + 255) / 256 * 256;
}

// the pointer checks of a MoE call that passed moe_shape_rc and has m > 0
inline int moe_pointers_rc(const void *c, const void *a, const void *b, const void *scales, const void *global_scales, const void *expert_offsets,
                           const void *a_row_index, const void *c_row_index, const void *bias, const void *workspace, uint64_t workspace_need) {
    if (!global_scales || !expert_offsets || (((uintptr_t)global_scales | (uintptr_t)expert_offsets | (uintptr_t)a_row_index | (uintptr_t)c_row_index) & 3u))
        return kRcProblemShape;
    return pointers_rc(c, a, b, scales, bias, workspace, workspace_need);
}

// The CPU twin: gemm_host per expert under the clamp rule (each offset clamped into [its predecessor, m], a running maximum), with HOST offsets
// and indices.  Plain epilogue.  An A index outside [0, a_rows) reads a zero row, a C index outside [0, c_rows) stores nothing, rows of no
// expert are left untouched.  bias: [num_experts][n] or null.
inline int moe_gemm_host(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const void *bias,
                         const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index,
                         unsigned a_rows, const int32_t *c_row_index, unsigned c_rows, int a_type, int b_type) {
    const int rc = moe_shape_rc(num_experts, m, n, k, a_row_index, a_rows, c_row_index, c_rows, a_type, b_type, 0);
    if (rc != kRcOk)
        return rc;
    if (m == 0)
        return kRcOk;
    if (!c || !a || !b || !scales || !global_scales || !expert_offsets)
        return kRcProblemShape;
    const size_t w_bytes = (size_t)n * k / 2, s_bytes = (size_t)n * k / (is_mx(b_type) ? 32 : 16);
    auto clamp = [&](int32_t v, unsigned lo) {
        const unsigned u = v < 0 ? 0u : (unsigned)v;
        return u < lo ? lo : (u > m ? m : u);
    };
    unsigned lo = clamp(expert_offsets[0], 0);
    std::vector<uint16_t> rows_a, rows_c;
    for (unsigned e = 0; e < num_experts; ++e) {
        const unsigned hi = clamp(expert_offsets[e + 1], lo), rows = hi - lo;
        if (rows) {
            rows_a.assign((size_t)rows * k, 0), rows_c.assign((size_t)rows * n, 0);
            for (unsigned r = 0; r < rows; ++r) {
                const unsigned src = a_row_index ? (unsigned)a_row_index[lo + r] : lo + r;
                if (src < a_rows)
                    memcpy(&rows_a[(size_t)r * k], (const uint16_t *)a + (size_t)src * k, (size_t)k * 2);
            }
            const int grc = gemm_host(rows_c.data(), rows_a.data(), (const char *)b + e * w_bytes, (const char *)scales + e * s_bytes,
                                      global_scales + e, bias ? (const uint16_t *)bias + (size_t)e * n : nullptr, rows, n, k, a_type, b_type);
            if (grc != kRcOk)
                return grc;
            for (unsigned r = 0; r < rows; ++r) {
                const unsigned dst = c_row_index ? (unsigned)c_row_index[lo + r] : lo + r;
                if (dst < c_rows)
                    memcpy((uint16_t *)c + (size_t)dst * n, &rows_c[(size_t)r * n], (size_t)n * 2);
            }
        }
        lo = hi;
    }
    return kRcOk;
}

} // namespace invariant
} // namespace petit_amd
