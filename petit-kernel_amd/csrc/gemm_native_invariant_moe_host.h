// gemm_native_invariant_moe_host.h -- the host side of the batch-invariant MoE launch on the native class (include/petit_amd.h "Batch-invariant
// MoE launch on the native class") that needs no GPU: the form switch, the workspace arithmetic, the argument checks and the CPU twin.  Plain
// C++ (no HIP) on top of gemm_native_invariant_host.h (the dense entry's checks, the "petit-qact/1" decode, its twin) and gemm_invariant_host.h
// (geometry, the MoE entry's pointer checks): the same lines build into libpetit_amd.so (gemm_native_invariant_moe.hip) and into a stand-alone
// program for sanitizer runs (tools/native_moe_invariant_hostcheck.cc).
#pragma once

#include "gemm_native_invariant_host.h"

namespace petit_amd {
namespace native_invariant {

// The form switch's two constants (profiles/native_moe_invariant.md): the exact MoE entry's rule, whose reasoning carries over -- the whole form
// wins wherever the routing gives it workgroups enough, the split form pays at a decode step's few rows only.
constexpr unsigned kMoeSplitMaxRowsPer = 8; // split form: ceil(m / min(E, m)) <= this (the rows-per-active-expert estimate of the MoE pick) ...
constexpr unsigned kMoeSplitMaxM = 8;       // ... and m <= this (also the cap of the slab workspace S * m * n * 4); at 8 the first is implied

// The form switch: a function of (m, num_experts) alone.  Either form gives the same bits, so it is a speed choice only.
// PETIT_NATIVE_MOE_INV_MEASURE_FORMS: a measurement-only build (tools/native_moe_invariant_bench.py --forms-lib) reads the two constants from the
// environment per call, so that one session can time both forms at one (m, E); never defined in a shipped library, where they are constants.
inline bool moe_split(unsigned m, unsigned num_experts) {
    unsigned rows_per = kMoeSplitMaxRowsPer, max_m = kMoeSplitMaxM;
#ifdef PETIT_NATIVE_MOE_INV_MEASURE_FORMS
    if (const char *e = getenv("PETIT_NATIVE_MOE_INV_SPLIT_ROWS_PER"))
        rows_per = (unsigned)atoi(e);
    if (const char *e = getenv("PETIT_NATIVE_MOE_INV_SPLIT_MAX_M"))
        max_m = (unsigned)atoi(e);
#endif
    const unsigned active = num_experts < m ? num_experts : m;
    if (active == 0)
        return true;
    return (m + active - 1) / active <= rows_per && m <= max_m;
}

// workgroups of the largest launch of a call (one linear index in grid x): the GEMM launch, and in the split form the fold over 16-row slots
inline uint64_t moe_grid(unsigned m, unsigned n, unsigned num_experts, unsigned slices, bool split, int activation) {
    const uint64_t active = num_experts < m ? num_experts : m, pairs = n / 32;
    if (split) {
        const uint64_t gemm = ((m + 31ull) / 32 + active) * slices * ((pairs + 3) / 4);
        const uint64_t n_out = activation ? n / 2 : n, fold = ((m + 15ull) / 16 + active) * ((16 * (n_out / 4) + 1023) / 1024);
        return gemm > fold ? gemm : fold;
    }
    const uint64_t nslots = activation ? pairs / 2 : (pairs + 1) / 2;
    return ((m + 63ull) / 64 + active) * ((nslots + 3) / 4);
}

// every refusal that depends on shape, types, formats and counts alone.  a_rows is read for a 16-bit A only; there is no 65535-row limit on it
// (the gathering quantiser takes any row count).
inline int moe_shape_rc(unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index, unsigned a_rows,
                        const int32_t *c_row_index, unsigned c_rows, int a_type, int act_format, int a_is_quantized, int activation) {
    const int rc = shape_rc(m, n, k, a_type, act_format, 1, activation);
    if (rc != inv::kRcOk)
        return rc;
    if (a_is_quantized && a_row_index)
        return inv::kRcBadArgument; // quantised bytes are the grouped rows already
    if (num_experts == 0 || num_experts > inv::kMoeMaxExperts)
        return inv::kRcProblemShape;
    // a null index is the identity: the rows it would name must exist
    if ((!a_is_quantized && !a_row_index && a_rows < m) || (!c_row_index && c_rows < m))
        return inv::kRcProblemShape;
    if (qact_bytes(m, k, act_format) >= (1ull << 32))
        return inv::kRcProblemShape; // (the quantiser's limit, kept for quantised input: one image, 32-bit offsets)
    unsigned S, L;
    inv::geometry(n, k, a_type, inv::kTypeMx, &S, &L);
    if (moe_grid(m, n, num_experts, S, moe_split(m, num_experts), activation) >= (1ull << 31))
        return inv::kRcProblemShape;
    return inv::kRcOk;
}

// the two parts of the workspace, each rounded up to 256: the quantised bytes (16-bit input only), then the slabs (split form only)
inline uint64_t moe_quant_part_bytes(unsigned m, unsigned k, int act_format, int a_is_quantized) {
    return a_is_quantized ? 0 : round256(qact_bytes(m, k, act_format));
}
inline uint64_t moe_slab_part_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type) {
    if (!moe_split(m, num_experts))
        return 0;
    unsigned S, L;
    inv::geometry(n, k, a_type, inv::kTypeMx, &S, &L);
    return round256((uint64_t)S * m * n * 4);
}
inline uint64_t moe_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int act_format, int a_is_quantized) {
    if (shape_rc(m, n, k, a_type, act_format, 1, 0) != inv::kRcOk || num_experts == 0 || num_experts > inv::kMoeMaxExperts || m == 0 ||
        qact_bytes(m, k, act_format) >= (1ull << 32))
        return 0;
    return moe_quant_part_bytes(m, k, act_format, a_is_quantized) + moe_slab_part_bytes(num_experts, m, n, k, a_type);
}

// rows [row0, row0 + rows) of the m-row image as an image of their own (the k-tile-major layout of gemm_native32.hpp: the addresses depend on
// the row count, the bytes of a row do not)
inline void qact_extract_rows(std::vector<uint8_t> &out, const uint8_t *qa, unsigned m, unsigned k, int act_format, unsigned row0, unsigned rows) {
    const unsigned row_b = act_format == 8 ? 128u : 64u, ktiles = k / 128;
    out.assign((size_t)qact_bytes(rows, k, act_format), 0);
    const size_t src_scale = (size_t)m * (k / 8 * (unsigned)act_format), dst_scale = (size_t)rows * (k / 8 * (unsigned)act_format);
    const size_t src_hi = (size_t)m * (k / 2), dst_hi = (size_t)rows * (k / 2);
    for (unsigned kt = 0; kt < ktiles; ++kt) {
        const size_t src = (size_t)kt * m + row0, dst = (size_t)kt * rows;
        memcpy(&out[dst * row_b], qa + src * row_b, (size_t)rows * row_b);
        if (act_format == 6)
            memcpy(&out[dst_hi + dst * 32], qa + src_hi + src * 32, (size_t)rows * 32);
        memcpy(&out[dst_scale + dst * 4], qa + src_scale + src * 4, (size_t)rows * 4);
    }
}

// The CPU twin: gemm_host per expert under the clamp rule (each offset clamped into [its predecessor, m], a running maximum), on HOST
// "petit-qact/1" bytes of the m grouped rows, HOST offsets and a HOST C index.  Plain epilogue.  A C index outside [0, c_rows) stores nothing,
// rows of no expert are left untouched.  bias: [num_experts][n] or null.
inline int moe_gemm_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scales, const void *bias,
                         const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *c_row_index,
                         unsigned c_rows, int a_type, int act_format) {
    const int rc = moe_shape_rc(num_experts, m, n, k, nullptr, m, c_row_index, c_rows, a_type, act_format, 1, 0);
    if (rc != inv::kRcOk)
        return rc;
    if (m == 0)
        return inv::kRcOk;
    if (!c || !qa || !b || !scales || !global_scales || !expert_offsets)
        return inv::kRcProblemShape;
    const size_t w_bytes = (size_t)n * k / 2, s_bytes = (size_t)n * k / 32;
    auto clamp = [&](int32_t v, unsigned lo) {
        const unsigned u = v < 0 ? 0u : (unsigned)v;
        return u < lo ? lo : (u > m ? m : u);
    };
    unsigned lo = clamp(expert_offsets[0], 0);
    std::vector<uint8_t> rows_q;
    std::vector<uint16_t> rows_c;
    for (unsigned e = 0; e < num_experts; ++e) {
        const unsigned hi = clamp(expert_offsets[e + 1], lo), rows = hi - lo;
        if (rows) {
            qact_extract_rows(rows_q, (const uint8_t *)qa, m, k, act_format, lo, rows);
            rows_c.assign((size_t)rows * n, 0);
            const int grc = gemm_host(rows_c.data(), rows_q.data(), (const char *)b + e * w_bytes, (const char *)scales + e * s_bytes,
                                      global_scales + e, bias ? (const uint16_t *)bias + (size_t)e * n : nullptr, rows, n, k, a_type, act_format);
            if (grc != inv::kRcOk)
                return grc;
            for (unsigned r = 0; r < rows; ++r) {
                const unsigned dst = c_row_index ? (unsigned)c_row_index[lo + r] : lo + r;
                if (dst < c_rows)
                    memcpy((uint16_t *)c + (size_t)dst * n, &rows_c[(size_t)r * n], (size_t)n * 2);
            }
        }
        lo = hi;
    }
    return inv::kRcOk;
}

} // namespace native_invariant
} // namespace petit_amd
