// gemm_invariant_host.h -- the host side of the batch-invariant GEMM family (include/petit_amd.h "Batch-invariant GEMM", "Batch-invariant MoE
// launch" and their two "... on the native class" sections) that needs no GPU: ONE description of a call of any entry (Call), ONE
// function from it to a plan (return code, S and L, the form, the workspace parts, every launch's grid), the pointer checks, the decode of
// "petit-qact/1" bytes and the CPU twins.  Plain C++ (no HIP), so that the same lines build into libpetit_amd.so (gemm_invariant_api.hip, and
// the launch functions of gemm_invariant*.hpp / gemm_native_invariant*.hpp, which take their grids from the plan) and into a stand-alone
// program for sanitizer runs (tools/invariant_hostcheck.cc).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "layout.h"
#include "numfmt.h"

namespace petit_amd {
namespace invariant {

// (values of include/petit_amd.h, restated so that this header stands alone; gemm_invariant_api.hip static_asserts them against petit_internal.h)
enum : int { kRcOk = 0, kRcProblemShape = 1, kRcKernelShape = 2, kRcBadArgument = 4 };
enum : int { kTypeNv = 3, kTypeFp16 = 4, kTypeBf16 = 5, kTypeMx = 7, kTypeMxF16Range = 8 };
constexpr unsigned kMaxRows = 1u << 20;     // kMaxM of petit_internal.h
constexpr unsigned kMaxSlices = 16;         // S <= 16
constexpr unsigned kSliceStep = 256;        // L is a multiple of it: the packed scale layout exists for k % 256 == 0 only (layout.h)
constexpr unsigned kTargetWaves = 2048;     // the split form's waves at M <= 16: 8 per CU of a 256-CU chip (n-tiles x S of them)
constexpr unsigned kSplitMaxM = 32;         // the largest M of the dense exact entry's split form
constexpr unsigned kNativeSplitMaxM = 64;   // ... of the dense native entry's: two m-tiles of 32 (measured: profiles/native_invariant.md)
constexpr unsigned kMaxQuantRows = 65535;   // the library's own dense quantiser takes one grid row per activation row
constexpr unsigned kMoeMaxExperts = 1024;   // kMoeMaxExperts of petit_internal.h
// The MoE form switch's two constants, measured for the exact entry (profiles/moe_invariant.md) and kept for the native one
// (profiles/native_moe_invariant.md): the whole form wins wherever the routing gives it workgroups enough to fill the chip -- from about 8 to 13
// grouped rows on -- and by 2x and more from 64 rows; the split form wins at a decode step's 4 to 8 rows.
constexpr unsigned kMoeSplitMaxRowsPer = 8; // split form: ceil(m / min(E, m)) <= this (the rows-per-active-expert estimate of the MoE pick) ...
constexpr unsigned kMoeSplitMaxM = 8;       // ... and m <= this (also the cap of the slab workspace S * m * n * 4); at 8 the first is implied

inline bool is_mx(int b_type) { return b_type == kTypeMx || b_type == kTypeMxF16Range; }
inline bool format_ok(int act_format) { return act_format == 8 || act_format == 6 || act_format == 4; }
inline uint64_t round256(uint64_t x) { return (x + 255) / 256 * 256; }
// (bytes of the "petit-qact/1" image of (m, k, format): qact_bytes, layout.h)

// One call of any entry.  The exact class reads b_type (act_format and a_is_quantized are 0); the native class reads act_format and
// a_is_quantized, and its b_type names the weight operand: kTypeMx, raw MXFP4 tensors, or kTypeNv, the "petit-cdna4-nv6/1" image(s) of NVFP4
// weights (layout.h) -- whose address enters the refusals (image_misaligned: it is no multiple of 256).  The five fields before it are the MoE
// entries'.
struct Call {
    bool native, moe;
    int a_type, b_type, act_format, a_is_quantized, activation;
    unsigned m, n, k;
    unsigned num_experts, a_rows, c_rows;
    bool has_a_index, has_c_index;
    bool image_misaligned;
};
inline Call dense_call(unsigned m, unsigned n, unsigned k, int a_type, int b_type, int activation) {
    return Call{false, false, a_type, b_type, 0, 0, activation, m, n, k, 0, 0, 0, false, false, false};
}
inline Call native_call(unsigned m, unsigned n, unsigned k, int a_type, int act_format, int a_is_quantized, int activation, int b_type = kTypeMx,
                        const void *image = nullptr) {
    return Call{true, false, a_type, b_type, act_format, a_is_quantized, activation, m, n, k, 0, 0, 0, false, false, ((uintptr_t)image & 255u) != 0};
}
inline Call moe_call(Call c, unsigned num_experts, bool has_a_index, unsigned a_rows, bool has_c_index, unsigned c_rows) {
    c.moe = true, c.num_experts = num_experts, c.has_a_index = has_a_index, c.a_rows = a_rows, c.has_c_index = has_c_index, c.c_rows = c_rows;
    return c;
}

// One launch of a call: tile_m rows per m-tile, `slots` m-tiles (MoE: sized for every routing, ceil(m / tile_m) + min(E, m)), `nblocks`
// workgroups along n per (slot[, slice]).  Dense launches use a 3-D grid; MoE launches ONE linear index in x (y / z stop at 65535).
struct Launch {
    unsigned tile_m, slots, nblocks;
    uint64_t grid_x;
    unsigned grid_y, grid_z;
};
struct Plan {
    int rc;                   // kRcOk: the call can run
    unsigned slices, slice_k; // S, L
    bool split;               // the form: split (GEMM into slabs, then the fold) or whole (one launch)
    uint64_t quant_bytes, slab_bytes, workspace_bytes; // the two parts, each rounded up to 256, and their sum; all 0 for a refused call or m == 0
    Launch gemm, fold;        // (fold: the split form only)
};

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

// The form switch: a function of m (dense) or (m, num_experts) (MoE) alone.  Either form gives the same bits, so it is a speed choice only.
// PETIT_NATIVE_INV_MEASURE_FORMS / PETIT_NATIVE_MOE_INV_MEASURE_FORMS: a measurement-only build (tools/native_invariant_bench.py and
// tools/native_moe_invariant_bench.py --forms-lib) reads the native entries' constants from the environment per call, so that one session can
// time both forms at one cell; never defined in a shipped library, where they are the constants.
inline bool is_split(const Call &c) {
    if (!c.moe) {
        unsigned max_m = c.native ? kNativeSplitMaxM : kSplitMaxM;
#ifdef PETIT_NATIVE_INV_MEASURE_FORMS
        if (const char *e = c.native ? getenv("PETIT_NATIVE_INV_SPLIT_MAX_M") : nullptr)
            max_m = (unsigned)atoi(e);
#endif
        return c.m <= max_m;
    }
    unsigned rows_per = kMoeSplitMaxRowsPer, max_m = kMoeSplitMaxM;
#ifdef PETIT_NATIVE_MOE_INV_MEASURE_FORMS
    if (const char *e = c.native ? getenv("PETIT_NATIVE_MOE_INV_SPLIT_ROWS_PER") : nullptr)
        rows_per = (unsigned)atoi(e);
    if (const char *e = c.native ? getenv("PETIT_NATIVE_MOE_INV_SPLIT_MAX_M") : nullptr)
        max_m = (unsigned)atoi(e);
#endif
    const unsigned active = c.num_experts < c.m ? c.num_experts : c.m;
    if (active == 0)
        return true;
    return (c.m + active - 1) / active <= rows_per && c.m <= max_m;
}

// Every refusal that depends on shape, types, formats and counts alone, but the grid bound (plan).  The ORDER of the tests decides which code
// an ill-formed call returns and is each entry's own.
inline int shape_rc(const Call &c) {
    const bool mx = is_mx(c.b_type), image = c.native && c.b_type == kTypeNv;
    if ((c.a_type != kTypeBf16 && c.a_type != kTypeFp16) || (c.b_type != kTypeNv && !mx) || (c.native && !format_ok(c.act_format)) ||
        c.activation < 0 || c.activation > 2)
        return kRcBadArgument;
    // (MXFP4: n % 32 == 0 -- its processed scale tensor comes in rows of 32 weight rows; the image: whole blocks of 32 weight rows, so that its
    // zero-padded last block never arises.  Gated: the halves are whole tiles / tile pairs / blocks.  The image's elements: 32-bit offsets.)
    if (c.n == 0 || c.k == 0 || c.n % 16 != 0 || ((mx || image) && c.n % 32 != 0) || c.k % 256 != 0 || c.m >= kMaxRows ||
        (c.activation && c.n % (c.native ? 64u : 32u) != 0) || (uint64_t)c.k * 128 >= (1ull << 31) ||
        (image && (uint64_t)nv6_elem_bytes(c.n, c.k) >= (1ull << 32)))
        return kRcProblemShape;
    if (image && c.image_misaligned)
        return kRcProblemShape;
    if (!c.native && c.a_type == kTypeFp16 && mx)
        return kRcKernelShape; // out-of-range scale bytes need the hi / lo fallback body: a second chain, a definition of its own
    if (c.native && !c.moe && !c.a_is_quantized && c.m > kMaxQuantRows)
        return kRcKernelShape; // (quantise such a matrix in pieces and pass the bytes; the MoE entry's gathering quantiser takes any row count)
    if (!c.moe)
        return kRcOk;
    const bool grouped = c.native && c.a_is_quantized; // quantised bytes are the grouped rows already: a_rows is not read
    if (grouped && c.has_a_index)
        return kRcBadArgument;
    if (c.num_experts == 0 || c.num_experts > kMoeMaxExperts)
        return kRcProblemShape;
    // a null index is the identity: the rows it would name must exist
    if ((!grouped && !c.has_a_index && c.a_rows < c.m) || (!c.has_c_index && c.c_rows < c.m))
        return kRcProblemShape;
    // exact: one descriptor bounds every A load, and the kernels' out-of-range voffset (2^31) must lie past its end.  native: the quantiser's
    // limit, kept for quantised input (one image, 32-bit offsets)
    if (c.native ? qact_bytes(c.m, c.k, c.act_format) >= (1ull << 32) : (uint64_t)c.a_rows * c.k * 2 > (1ull << 31))
        return kRcProblemShape;
    return kRcOk;
}

// The plan of a call.  S, L and the form are functions of the numbers alone and are set for a refused call too (the geometry, slab and form
// queries read them); the launches and the workspace are set once shape_rc passes.  The last refusal reads the launches: a MoE launch has one
// linear workgroup index, which must stay below 2^31.
inline Plan plan(const Call &c) {
    Plan p{};
    geometry(c.n, c.k, c.a_type, c.b_type, &p.slices, &p.slice_k);
    p.split = is_split(c);
    p.rc = shape_rc(c);
    if (p.rc != kRcOk)
        return p;
    // a column unit: one n-tile of 16 (exact) or a pair of them (native); a wave of the split form owns one unit, of the whole form two
    const unsigned unit = c.native ? 32u : 16u, units = c.n / unit, n_out = c.activation ? c.n / 2 : c.n;
    const unsigned routed = c.moe ? (c.num_experts < c.m ? c.num_experts : c.m) : 0u; // (a partial m-tile per active expert)
    Launch &g = p.gemm, &f = p.fold;
    g.tile_m = p.split ? unit : 64u;
    g.slots = (c.m + g.tile_m - 1) / g.tile_m + routed;
    g.nblocks = p.split ? (units + 3) / 4 : ((c.activation ? units / 2 : (units + 1) / 2) + 3) / 4;
    if (c.moe)
        g.grid_x = (uint64_t)g.slots * (p.split ? p.slices : 1u) * g.nblocks, g.grid_y = g.grid_z = 1;
    else
        g.grid_x = g.nblocks, g.grid_y = p.split ? p.slices : g.slots, g.grid_z = p.split ? g.slots : 1u;
    if (p.split) { // a thread folds 4 consecutive output columns of one row
        f.tile_m = 16, f.slots = (c.m + 15) / 16 + routed, f.grid_y = f.grid_z = 1;
        if (c.moe) { // over its own 16-row slot map; a thread folds at most 4 units of its m-tile
            f.nblocks = (16u * (n_out / 4) + 1023) / 1024;
            f.grid_x = (uint64_t)f.slots * f.nblocks;
        } else {
            const uint64_t blocks = ((uint64_t)c.m * (n_out / 4) + 255) / 256;
            f.nblocks = (unsigned)(blocks < 4096 ? blocks : 4096);
            f.grid_x = f.nblocks;
        }
    }
    if (c.m) {
        p.quant_bytes = c.native && !c.a_is_quantized ? round256(qact_bytes(c.m, c.k, c.act_format)) : 0;
        p.slab_bytes = p.split ? round256((uint64_t)p.slices * c.m * c.n * 4) : 0;
        p.workspace_bytes = p.quant_bytes + p.slab_bytes;
    }
    if (c.moe && (g.grid_x >= (1ull << 31) || f.grid_x >= (1ull << 31)))
        p.rc = kRcProblemShape;
    return p;
}

// the pointer checks of a call that passed the plan and has m > 0
inline int pointers_rc(const void *c, const void *a, const void *b, const void *scales, const void *bias, const void *workspace,
                       uint64_t workspace_need) {
    if (!c || !a || !b || !scales || (workspace_need && !workspace))
        return kRcProblemShape;
    if ((((uintptr_t)c | (uintptr_t)a | (uintptr_t)b | (uintptr_t)scales) & 15u) || ((uintptr_t)bias & 7u) ||
        (workspace_need && ((uintptr_t)workspace & 255u)))
        return kRcProblemShape;
    return kRcOk;
}
inline int moe_pointers_rc(const void *c, const void *a, const void *b, const void *scales, const void *global_scales, const void *expert_offsets,
                           const void *a_row_index, const void *c_row_index, const void *bias, const void *workspace, uint64_t workspace_need) {
    if (!global_scales || !expert_offsets || (((uintptr_t)global_scales | (uintptr_t)expert_offsets | (uintptr_t)a_row_index | (uintptr_t)c_row_index) & 3u))
        return kRcProblemShape;
    return pointers_rc(c, a, b, scales, bias, workspace, workspace_need);
}

// (number formats: numfmt.h.  The 16-bit results of this family round as the kernels' epilogues do, f32_h16_quiet_nan; e8m0_f32 reads byte 0 as
// 2^-127, as the kernels do.)

// the weight operand of the definition: fp4 x group scale, exact in the activation type for every (type, format) pair the entries accept
inline float weight_value(const uint32_t *pw, const uint8_t *ps, bool mx, unsigned k_total, unsigned n, unsigned kk) {
    const uint32_t word = pw[packed_weight_word_index(k_total, n, kk / 8)];
    const float q = e2m1_f32((word >> (4 * (kk % 8))) & 15u);
    const float sc = mx ? e8m0_f32(ps[packed_mxscale_byte_index(k_total, n, kk / kMxGroup)])
                        : e4m3_f32(ps[packed_nvscale_byte_index(k_total, n, kk / kNvGroup)]);
    return q * sc;
}

// ---- "petit-qact/1" (layout.h) -----------------------------------------------------------------------------------------------------------------

// element (row, kk) of the image, WITHOUT its block scale, and the block's E8M0 byte
inline float qact_element(const uint8_t *qa, unsigned m, unsigned k, int act_format, unsigned row, unsigned kk) {
    const unsigned kt = kk / 128, b = (kk % 128) / 32, i = kk % 32;
    const size_t tile_row = qact_tile_row(m, kt, row), row_b = qact_row_bytes(act_format);
    if (act_format == 8) {
        const unsigned col16 = (kk % 128) / 8, u16 = col16 >> 1, half = col16 & 1u;
        return e4m3_f32(qa[tile_row * row_b + qact_fp8_unit_pos(u16) * 16 + half * 8 + kk % 8]);
    }
    if (act_format == 4) {
        const unsigned byte = qa[tile_row * row_b + 16 * b + i / 2];
        return e2m1_f32((byte >> (4 * (i & 1u))) & 15u);
    }
    // MXFP6: the block's 24 bytes = 16 in the first image, 8 in the second; element i at bits [6 i, 6 i + 6)
    const uint8_t *const lo = qa + tile_row * row_b + 16 * b;
    const uint8_t *const hi = qa + qact_hi_offset(m, k) + tile_row * kQactHiRowBytes + 8 * qact_fp6_hi_slot(b);
    const unsigned bit = 6 * i;
    auto byte_at = [&](unsigned j) -> unsigned { return j < 16 ? lo[j] : hi[j - 16]; };
    unsigned v = byte_at(bit / 8) >> (bit % 8);
    if (bit % 8 > 2)
        v |= byte_at(bit / 8 + 1) << (8 - bit % 8);
    return e2m3_f32(v & 63u);
}
inline unsigned qact_scale_byte(const uint8_t *qa, unsigned m, unsigned k, int act_format, unsigned row, unsigned blk) {
    return qa[qact_elem_bytes(m, k, act_format) + qact_scale_dword(m, blk / 4, row) * kQactScaleRowBytes + blk % 4];
}
// rows [row0, row0 + rows) of the m-row image as an image of their own (k-tile-major: the addresses depend on the row count, the bytes of a
// row do not)
inline void qact_extract_rows(std::vector<uint8_t> &out, const uint8_t *qa, unsigned m, unsigned k, int act_format, unsigned row0, unsigned rows) {
    const unsigned row_b = qact_row_bytes(act_format), ktiles = k / 128;
    out.assign(qact_bytes(rows, k, act_format), 0);
    const size_t src_scale = qact_elem_bytes(m, k, act_format), dst_scale = qact_elem_bytes(rows, k, act_format);
    const size_t src_hi = qact_hi_offset(m, k), dst_hi = qact_hi_offset(rows, k);
    for (unsigned kt = 0; kt < ktiles; ++kt) {
        const size_t src = qact_tile_row(m, kt, row0), dst = qact_tile_row(rows, kt, 0);
        memcpy(&out[dst * row_b], qa + src * row_b, (size_t)rows * row_b);
        if (act_format == 6)
            memcpy(&out[dst_hi + dst * kQactHiRowBytes], qa + src_hi + src * kQactHiRowBytes, (size_t)rows * kQactHiRowBytes);
        memcpy(&out[dst_scale + dst * kQactScaleRowBytes], qa + src_scale + src * kQactScaleRowBytes, (size_t)rows * kQactScaleRowBytes);
    }
}

// ---- the CPU twins -------------------------------------------------------------------------------------------------------------------------

// The definition's sum and finish, for both classes: c = round16(((p_0 + p_1) + ... + p_{S-1}) * gs + bias), p_s a sequential fp32 sum over
// the slice's k ascending of product(row, kk) -- ONE fp32 value per (row, kk) -- after load_column(col) has brought out column col's weights.
// (The device's p_s is an MFMA chain: the same value whenever the partial sums are exact, a few ulp apart otherwise.)  Host pointers;
// global_scale and bias may be null.
template <class LoadColumn, class Product>
inline void sliced_sum_finish(void *c, const float *global_scale, const void *bias, unsigned m, unsigned n, unsigned k, const Plan &p, bool bf16,
                              LoadColumn load_column, Product product) {
    const unsigned S = p.slices, L = p.slice_k;
    const uint16_t *const b16 = (const uint16_t *)bias;
    uint16_t *const c16 = (uint16_t *)c;
    for (unsigned col = 0; col < n; ++col) {
        load_column(col);
        for (unsigned row = 0; row < m; ++row) {
            float y = 0.f;
            for (unsigned s = 0; s < S; ++s) {
                const unsigned k_end = (s + 1) * L < k ? (s + 1) * L : k;
                volatile float acc = 0.f; // (volatile: one rounding per step, whatever the compiler's contraction setting)
                for (unsigned kk = s * L; kk < k_end; ++kk) {
                    volatile float t = product(row, kk);
                    acc = acc + t;
                }
                y = s ? y + acc : acc;
            }
            if (global_scale) {
                volatile float t = y * *global_scale;
                y = t;
            }
            if (bias)
                y = y + h16_f32(bf16, b16[col]);
            c16[(size_t)row * n + col] = (uint16_t)f32_h16_quiet_nan(bf16, y);
        }
    }
}

// the exact class: 16-bit activations, the weight dequantised exactly; a product is one fp32 multiply.  Activation none.
inline int gemm_host(void *c, const void *a, const void *b, const void *scales, const float *global_scale, const void *bias, unsigned m, unsigned n,
                     unsigned k, int a_type, int b_type) {
    const Plan p = plan(dense_call(m, n, k, a_type, b_type, 0));
    if (p.rc != kRcOk || m == 0)
        return p.rc;
    if (!(c && a && b && scales))
        return kRcProblemShape;
    const bool bf16 = a_type == kTypeBf16, mx = is_mx(b_type);
    const uint16_t *const a16 = (const uint16_t *)a;
    std::vector<float> wrow(k);
    sliced_sum_finish(
        c, global_scale, bias, m, n, k, p, bf16,
        [&](unsigned col) {
            for (unsigned kk = 0; kk < k; ++kk)
                wrow[kk] = weight_value((const uint32_t *)b, (const uint8_t *)scales, mx, k, col, kk);
        },
        [&](unsigned row, unsigned kk) -> float { return h16_f32(bf16, a16[(size_t)row * k + kk]) * wrow[kk]; });
    return kRcOk;
}

// the native class, on HOST "petit-qact/1" bytes: every product formed exactly (f64) and rounded once to fp32 (the device's chain is the
// block-scaled MFMA's).  Activation none.
inline int native_gemm_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scale, const void *bias, unsigned m,
                            unsigned n, unsigned k, int a_type, int act_format) {
    const Plan p = plan(native_call(m, n, k, a_type, act_format, 1, 0));
    if (p.rc != kRcOk || m == 0)
        return p.rc;
    if (!(c && qa && b && scales))
        return kRcProblemShape;
    const uint8_t *const q8 = (const uint8_t *)qa;
    std::vector<double> wrow(k), arow((size_t)m * k);
    for (unsigned row = 0; row < m; ++row)
        for (unsigned kk = 0; kk < k; ++kk)
            arow[(size_t)row * k + kk] =
                (double)qact_element(q8, m, k, act_format, row, kk) * e8m0_f64(qact_scale_byte(q8, m, k, act_format, row, kk / 32));
    sliced_sum_finish(
        c, global_scale, bias, m, n, k, p, a_type == kTypeBf16,
        [&](unsigned col) {
            for (unsigned kk = 0; kk < k; ++kk) {
                const uint32_t word = ((const uint32_t *)b)[packed_weight_word_index(k, col, kk / 8)];
                wrow[kk] = (double)e2m1_f32((word >> (4 * (kk % 8))) & 15u) *
                           e8m0_f64(((const uint8_t *)scales)[packed_mxscale_byte_index(k, col, kk / kMxGroup)]);
            }
        },
        [&](unsigned row, unsigned kk) -> float { return (float)(arow[(size_t)row * k + kk] * wrow[kk]); });
    return kRcOk;
}

// the native class on an NVFP4 image: element (col, kk) of the HOST "petit-cdna4-nv6/1" image -- the e2m3 code at bits [6 e, 6 e + 6) of the
// lane's 192 (planes 0 / 1: registers 0-3 of P1 / P2, plane 2: registers 4-5 of both; nv6_unit_offset) -- times 2^(byte - 127) of its block's
// E8M0 byte (nv6_scale_offset): what petit_nvfp4_native_image_dequant_host expands, as an exact double
inline double nv6_weight_f64(const uint8_t *image, unsigned n, unsigned k, unsigned col, unsigned kk) {
    const unsigned blk = kk / 32, e = kk % 32, kt = blk / 4, q = (blk % 4) >> 1, h = blk & 1u;
    uint32_t words[6];
    memcpy(words, image + nv6_unit_offset(k, col, kt, q, h), 16);
    memcpy(words + 4, image + nv6_unit_offset(k, col, kt, 2, h) + q * 8, 8);
    const unsigned bit = 6 * e;
    uint64_t wv = words[bit / 32];
    if (bit / 32 + 1 < 6)
        wv |= (uint64_t)words[bit / 32 + 1] << 32;
    const unsigned sb = image[nv6_elem_bytes(n, k) + nv6_scale_offset(k, col, blk)];
    return (double)e2m3_f32((unsigned)(wv >> (bit % 32)) & 63u) * e8m0_f64(sb);
}

// the twin of the entries on images, on HOST "petit-qact/1" bytes and a HOST image: native_gemm_host with the image's weights.  Activation none.
inline int nv_native_gemm_host(void *c, const void *qa, const void *image, const float *global_scale, const void *bias, unsigned m, unsigned n,
                               unsigned k, int a_type, int act_format) {
    const Plan p = plan(native_call(m, n, k, a_type, act_format, 1, 0, kTypeNv));
    if (p.rc != kRcOk || m == 0)
        return p.rc;
    if (!(c && qa && image))
        return kRcProblemShape;
    const uint8_t *const q8 = (const uint8_t *)qa;
    std::vector<double> wrow(k), arow((size_t)m * k);
    for (unsigned row = 0; row < m; ++row)
        for (unsigned kk = 0; kk < k; ++kk)
            arow[(size_t)row * k + kk] =
                (double)qact_element(q8, m, k, act_format, row, kk) * e8m0_f64(qact_scale_byte(q8, m, k, act_format, row, kk / 32));
    sliced_sum_finish(
        c, global_scale, bias, m, n, k, p, a_type == kTypeBf16,
        [&](unsigned col) {
            for (unsigned kk = 0; kk < k; ++kk)
                wrow[kk] = nv6_weight_f64((const uint8_t *)image, n, k, col, kk);
        },
        [&](unsigned row, unsigned kk) -> float { return (float)(arow[(size_t)row * k + kk] * wrow[kk]); });
    return kRcOk;
}

// The MoE twins' driver: a dense twin per expert under the clamp rule (each offset clamped into [its predecessor, m], a running maximum), with
// HOST offsets and a HOST C index.  run_expert(e, lo, rows, rows_c) computes grouped rows [lo, lo + rows) of expert e into rows_c and returns
// the dense twin's code.  A C index outside [0, c_rows) stores nothing, rows of no expert are left untouched.
template <class RunExpert>
inline int moe_twin(void *c, const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, const int32_t *c_row_index, unsigned c_rows,
                    RunExpert run_expert) {
    auto clamp = [&](int32_t v, unsigned lo) {
        const unsigned u = v < 0 ? 0u : (unsigned)v;
        return u < lo ? lo : (u > m ? m : u);
    };
    unsigned lo = clamp(expert_offsets[0], 0);
    std::vector<uint16_t> rows_c;
    for (unsigned e = 0; e < num_experts; ++e) {
        const unsigned hi = clamp(expert_offsets[e + 1], lo), rows = hi - lo;
        if (rows) {
            rows_c.assign((size_t)rows * n, 0);
            const int grc = run_expert(e, lo, rows, rows_c.data());
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

// the exact class: an expert's rows are gathered 16-bit rows; an A index outside [0, a_rows) reads a zero row.  bias: [num_experts][n] or null.
inline int moe_gemm_host(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const void *bias,
                         const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index,
                         unsigned a_rows, const int32_t *c_row_index, unsigned c_rows, int a_type, int b_type) {
    const Plan p = plan(moe_call(dense_call(m, n, k, a_type, b_type, 0), num_experts, a_row_index != nullptr, a_rows, c_row_index != nullptr, c_rows));
    if (p.rc != kRcOk || m == 0)
        return p.rc;
    if (!(c && a && b && scales && global_scales && expert_offsets))
        return kRcProblemShape;
    const size_t w_bytes = (size_t)n * k / 2, s_bytes = (size_t)n * k / (is_mx(b_type) ? 32 : 16);
    std::vector<uint16_t> rows_a;
    return moe_twin(c, expert_offsets, num_experts, m, n, c_row_index, c_rows, [&](unsigned e, unsigned lo, unsigned rows, uint16_t *rows_c) {
        rows_a.assign((size_t)rows * k, 0);
        for (unsigned r = 0; r < rows; ++r) {
            const unsigned src = a_row_index ? (unsigned)a_row_index[lo + r] : lo + r;
            if (src < a_rows)
                memcpy(&rows_a[(size_t)r * k], (const uint16_t *)a + (size_t)src * k, (size_t)k * 2);
        }
        return gemm_host(rows_c, rows_a.data(), (const char *)b + e * w_bytes, (const char *)scales + e * s_bytes, global_scales + e,
                         bias ? (const uint16_t *)bias + (size_t)e * n : nullptr, rows, n, k, a_type, b_type);
    });
}

// the native class: HOST "petit-qact/1" bytes of the m grouped rows; an expert's rows are an image of their own
inline int native_moe_gemm_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scales, const void *bias,
                                const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *c_row_index,
                                unsigned c_rows, int a_type, int act_format) {
    const Plan p = plan(moe_call(native_call(m, n, k, a_type, act_format, 1, 0), num_experts, false, m, c_row_index != nullptr, c_rows));
    if (p.rc != kRcOk || m == 0)
        return p.rc;
    if (!(c && qa && b && scales && global_scales && expert_offsets))
        return kRcProblemShape;
    const size_t w_bytes = (size_t)n * k / 2, s_bytes = (size_t)n * k / 32;
    std::vector<uint8_t> rows_q;
    return moe_twin(c, expert_offsets, num_experts, m, n, c_row_index, c_rows, [&](unsigned e, unsigned lo, unsigned rows, uint16_t *rows_c) {
        qact_extract_rows(rows_q, (const uint8_t *)qa, m, k, act_format, lo, rows);
        return native_gemm_host(rows_c, rows_q.data(), (const char *)b + e * w_bytes, (const char *)scales + e * s_bytes, global_scales + e,
                                bias ? (const uint16_t *)bias + (size_t)e * n : nullptr, rows, n, k, a_type, act_format);
    });
}

// the native class on the experts' images: expert e's image starts e * nv6_image_bytes(n, k) into `images`
inline int nv_native_moe_gemm_host(void *c, const void *qa, const void *images, const float *global_scales, const void *bias,
                                   const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                   const int32_t *c_row_index, unsigned c_rows, int a_type, int act_format) {
    const Plan p =
        plan(moe_call(native_call(m, n, k, a_type, act_format, 1, 0, kTypeNv), num_experts, false, m, c_row_index != nullptr, c_rows));
    if (p.rc != kRcOk || m == 0)
        return p.rc;
    if (!(c && qa && images && global_scales && expert_offsets))
        return kRcProblemShape;
    std::vector<uint8_t> rows_q;
    return moe_twin(c, expert_offsets, num_experts, m, n, c_row_index, c_rows, [&](unsigned e, unsigned lo, unsigned rows, uint16_t *rows_c) {
        qact_extract_rows(rows_q, (const uint8_t *)qa, m, k, act_format, lo, rows);
        return nv_native_gemm_host(rows_c, rows_q.data(), (const char *)images + e * nv6_image_bytes(n, k), global_scales + e,
                                   bias ? (const uint16_t *)bias + (size_t)e * n : nullptr, rows, n, k, a_type, act_format);
    });
}

} // namespace invariant
} // namespace petit_amd
