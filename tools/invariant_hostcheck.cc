// tools/invariant_hostcheck.cc -- a stand-alone program around the host side of the batch-invariant GEMM family
// (petit-kernel_amd/csrc/gemm_invariant_host.h: the call description and its plan -- return codes, geometry, form rules, workspace and grid
// arithmetic --, the pointer checks, the decode of "petit-qact/1" bytes and the CPU twins), for sanitizer runs on the CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipetit-kernel_amd/csrc \
//         tools/invariant_hostcheck.cc -o invariant_hostcheck && ./invariant_hostcheck
//
// Every buffer has exactly the bytes the layouts declare (an index outside them is a heap overflow the sanitizer sees).
//   dense, both classes: small exact problems of every accepted (type, format) pair -- the native class's quantised image written element by
//     element with an encoder of its own that mirrors the layout notes of gemm_native32.hpp, and read back through the header's decode --, the
//     twin with and without global scale and bias, for a batch and for each row alone, against a double-precision reference.
//   MoE, both classes: random experts under well-formed and malformed offsets, gathers and scatters that go out of range, poisoned outputs;
//     every row against the dense twin on that row alone and its owner (the clamp rule, restated here; the native row's image copied out here
//     by the layout notes, not by the header's own helper).
//   the native entries on NVFP4 images: the same, on "petit-cdna4-nv6/1" images written element by element from the layout notes of layout.h.
//   then every refusal, the form rules, the workspace arithmetic written out by hand, and the plan's grids against literals.
//   first of all: the encoders and decoders of numfmt.h and the "petit-qact/1" functions of layout.h on their edge values (zero, subnormals,
//     ties, the saturation points, infinity, NaN, scale bytes 0 / 254 / 255, the last row and k-tile of an image).
// Exit status 0 and "ok" when everything holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gemm_invariant_host.h"

using namespace petit_amd;
using namespace petit_amd::invariant;

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// ---- the plan, read entry by entry -----------------------------------------------------------------------------------------------------------

static Call moe_of(Call c, unsigned E, const int32_t *a_idx, unsigned a_rows, const int32_t *c_idx, unsigned c_rows) {
    return moe_call(c, E, a_idx != nullptr, a_rows, c_idx != nullptr, c_rows);
}
static int shape_rc(unsigned m, unsigned n, unsigned k, int a_type, int b_type, int act) { return plan(dense_call(m, n, k, a_type, b_type, act)).rc; }
static int native_shape_rc(unsigned m, unsigned n, unsigned k, int a_type, int fmt, int quantized, int act) {
    return plan(native_call(m, n, k, a_type, fmt, quantized, act)).rc;
}
static int moe_shape_rc(unsigned E, unsigned m, unsigned n, unsigned k, const int32_t *a_idx, unsigned a_rows, const int32_t *c_idx, unsigned c_rows,
                        int a_type, int b_type, int act) {
    return plan(moe_of(dense_call(m, n, k, a_type, b_type, act), E, a_idx, a_rows, c_idx, c_rows)).rc;
}
static int native_moe_shape_rc(unsigned E, unsigned m, unsigned n, unsigned k, const int32_t *a_idx, unsigned a_rows, const int32_t *c_idx,
                               unsigned c_rows, int a_type, int fmt, int quantized, int act) {
    return plan(moe_of(native_call(m, n, k, a_type, fmt, quantized, act), E, a_idx, a_rows, c_idx, c_rows)).rc;
}
// (the queries of the C ABI: no activation, no indices, matrices of m rows)
static Plan dense_plan(unsigned m, unsigned n, unsigned k, int a_type, int b_type) { return plan(dense_call(m, n, k, a_type, b_type, 0)); }
static Plan native_plan(unsigned m, unsigned n, unsigned k, int a_type, int fmt, int quantized) { return plan(native_call(m, n, k, a_type, fmt, quantized, 0)); }
static Plan moe_plan(unsigned E, unsigned m, unsigned n, unsigned k, int a_type, int b_type, int act = 0) {
    return plan(moe_call(dense_call(m, n, k, a_type, b_type, act), E, false, m, false, m));
}
static Plan native_moe_plan(unsigned E, unsigned m, unsigned n, unsigned k, int a_type, int fmt, int quantized, int act = 0) {
    return plan(moe_call(native_call(m, n, k, a_type, fmt, quantized, act), E, false, m, false, m));
}
static unsigned slabs(const Plan &p) { return p.split ? p.slices : 1u; }
static bool moe_split(unsigned m, unsigned E) { return moe_plan(E, m, 0, 0, 0, 0).split; }
static bool native_moe_split(unsigned m, unsigned E) { return native_moe_plan(E, m, 0, 0, 0, 8, 1).split; }
static uint64_t max_grid(const Plan &p) { return std::max(p.gemm.grid_x, p.fold.grid_x); }

// ---- shared pieces ---------------------------------------------------------------------------------------------------------------------------

// owner of every grouped row (-1: no expert): each offset clamped into [its predecessor, m], a running maximum
static std::vector<int> owners(const std::vector<int32_t> &off, unsigned m) {
    std::vector<int> own(m, -1);
    long lo = off[0] < 0 ? 0 : (off[0] > (long)m ? (long)m : off[0]);
    for (size_t e = 0; e + 1 < off.size(); ++e) {
        long hi = off[e + 1] < lo ? lo : (off[e + 1] > (long)m ? (long)m : off[e + 1]);
        for (long r = lo; r < hi; ++r)
            own[r] = (int)e;
        lo = hi;
    }
    return own;
}

// offsets of E experts over m rows, well formed and not
static std::vector<std::vector<int32_t>> routings(unsigned E, unsigned m) {
    std::vector<std::vector<int32_t>> list;
    auto frac = [&](std::initializer_list<double> f) {
        std::vector<int32_t> off(E + 1, (int32_t)m);
        unsigned i = 0;
        for (double x : f)
            if (i <= E)
                off[i++] = (int32_t)(x * m);
        list.push_back(off);
    };
    frac({0, 0.3, 0.3, 0.7, 1});       // well formed, an empty expert
    frac({0, 0, 0.5, 0.5, 0.5});       // an empty first expert; the last ones take the rest
    frac({0.1, 0.3, 0.5, 0.5, 0.9});   // rows before the first expert (and after the last when E == 4)
    frac({0, 0.6, 0.2, 0.8, 1});       // descending
    frac({-0.2, 0.4, -0.1, 3.0, 0.5}); // negative, beyond m
    return list;
}

// packed FP4 weights with power-of-two group scales (exact in every type), and their values.  MX: bytes byte0 + {0, 1, 2}; NV: e4m3 1, 2, 4.
static void fill_exact_weights(std::mt19937 &rng, unsigned n, unsigned k, bool mx, unsigned byte0, std::vector<uint32_t> &pw, std::vector<uint8_t> &ps,
                               std::vector<double> &w) {
    const unsigned group = mx ? kMxGroup : kNvGroup;
    static const uint8_t nv_bytes[3] = {0x38, 0x40, 0x48};
    pw.assign((size_t)n * k / 8, 0u), ps.assign((size_t)n * k / group, 0u), w.assign((size_t)n * k, 0.0);
    for (unsigned row = 0; row < n; ++row)
        for (unsigned g = 0; g < k / group; ++g) {
            const unsigned pick = rng() % 3;
            const size_t at = mx ? packed_mxscale_byte_index(k, row, g) : packed_nvscale_byte_index(k, row, g);
            ps.at(at) = mx ? (uint8_t)(byte0 + pick) : nv_bytes[pick];
            for (unsigned i = 0; i < group; ++i) {
                const unsigned kk = g * group + i, code = rng() & 15u;
                pw.at(packed_weight_word_index(k, row, kk / 8)) |= code << (4 * (kk % 8));
                w[(size_t)row * k + kk] = (double)e2m1_f32(code) * std::ldexp(1.0, mx ? (int)(byte0 + pick) - 127 : (int)pick);
            }
        }
}

// A dense twin on an exact problem: with and without global scale and bias, the batch and each row alone, against the f64 reference.
// twin(c, row, gs, bias): row < 0 the whole batch into c[m][n], else that row alone into c[n].
template <class Twin>
static void check_exact_problem(std::mt19937 &rng, unsigned m, unsigned n, unsigned k, bool bf16, const std::vector<double> &a64,
                                const std::vector<double> &w, Twin twin) {
    std::vector<uint16_t> bias(n), c((size_t)m * n, 0x7fc1u), c1(n);
    std::vector<double> b64(n);
    for (unsigned i = 0; i < n; ++i) {
        const int v = (int)(rng() % 17) - 8;
        bias[i] = (uint16_t)f32_h16_quiet_nan(bf16, (float)v), b64[i] = v;
    }
    for (int with_gs = 0; with_gs < 2; ++with_gs)
        for (int with_bias = 0; with_bias < 2; ++with_bias) {
            const float gs = 0.25f;
            EXPECT(twin(c.data(), -1, with_gs ? &gs : nullptr, with_bias ? bias.data() : nullptr) == kRcOk);
            for (unsigned row = 0; row < m; ++row) {
                EXPECT(twin(c1.data(), (int)row, with_gs ? &gs : nullptr, with_bias ? bias.data() : nullptr) == kRcOk);
                for (unsigned col = 0; col < n; ++col) {
                    double y = 0;
                    for (unsigned kk = 0; kk < k; ++kk)
                        y += a64[(size_t)row * k + kk] * w[(size_t)col * k + kk];
                    y = y * (with_gs ? 0.25 : 1.0) + (with_bias ? b64[col] : 0.0);
                    EXPECT(c[(size_t)row * n + col] == (uint16_t)f32_h16_quiet_nan(bf16, (float)y)); // exact inputs: one rounding is left
                    EXPECT(c1[col] == c[(size_t)row * n + col]);                           // the row alone: the same bits
                }
            }
        }
}

// ---- the dense exact entry -------------------------------------------------------------------------------------------------------------------

static void run_pair(int a_type, int b_type, unsigned m, unsigned n, unsigned k, unsigned seed) {
    const bool bf16 = a_type == kTypeBf16;
    std::mt19937 rng(seed);
    std::vector<uint32_t> pw;
    std::vector<uint8_t> ps;
    std::vector<double> w, a64((size_t)m * k);
    fill_exact_weights(rng, n, k, is_mx(b_type), 127, pw, ps, w);
    std::vector<uint16_t> a((size_t)m * k);
    for (size_t i = 0; i < a.size(); ++i) {
        const int v = (rng() & 1u) ? (int)(rng() % 7) - 3 : 0;
        a[i] = (uint16_t)f32_h16_quiet_nan(bf16, (float)v), a64[i] = v;
    }
    check_exact_problem(rng, m, n, k, bf16, a64, w, [&](uint16_t *c, int row, const float *gs, const uint16_t *bias) {
        return row < 0 ? gemm_host(c, a.data(), pw.data(), ps.data(), gs, bias, m, n, k, a_type, b_type)
                       : gemm_host(c, a.data() + (size_t)row * k, pw.data(), ps.data(), gs, bias, 1, n, k, a_type, b_type);
    });
}

// e8m0 scale byte 0 is 2^-127 (the hardware convert's reading, the kernels'), not 0.0: every weight +6 under byte 0, one activation of
// 2^120 per row -> 6 * 2^-127 * 2^120 = 1.5 * 2^-5 in every column, times gs 2, plus bias 1; byte 255 is not a number.
static void run_e8m0_ends() {
    const unsigned m = 2, n = 32, k = 512; // (two slices of 256)
    std::vector<uint32_t> pw((size_t)n * k / 8, 0x77777777u);
    std::vector<uint8_t> ps((size_t)n * k / kMxGroup, 0u);
    std::vector<uint16_t> a((size_t)m * k, 0u), bias(n, 0x3f80u), c((size_t)m * n, 0x7fc1u);
    a[5] = 0x7b80u, a[k + 300] = 0xfb80u; // +2^120 at k = 5 of row 0, -2^120 at k = 300 of row 1
    EXPECT(e8m0_f32(0) == 0x1p-127f && e8m0_f32(1) == 0x1p-126f && e8m0_f32(127) == 1.0f && e8m0_f32(254) == 0x1p127f && std::isinf(e8m0_f32(255)));
    EXPECT(gemm_host(c.data(), a.data(), pw.data(), ps.data(), nullptr, nullptr, m, n, k, kTypeBf16, kTypeMx) == kRcOk);
    for (unsigned col = 0; col < n; ++col)
        EXPECT(c[col] == 0x3d40u && c[n + col] == 0xbd40u); // +-1.5 * 2^-5
    const float gs = 2.0f;
    EXPECT(gemm_host(c.data(), a.data(), pw.data(), ps.data(), &gs, bias.data(), m, n, k, kTypeBf16, kTypeMx) == kRcOk);
    for (unsigned col = 0; col < n; ++col)
        EXPECT(c[col] == 0x3f8cu && c[n + col] == 0x3f68u); // 1 + 3 * 2^-5 = 1.09375, 1 - 3 * 2^-5 = 0.90625 = 1.8125 / 2
    ps.at(packed_mxscale_byte_index(k, 7, 3)) = 255u; // column 7 alone: NaN in every row
    EXPECT(gemm_host(c.data(), a.data(), pw.data(), ps.data(), &gs, bias.data(), m, n, k, kTypeBf16, kTypeMx) == kRcOk);
    for (unsigned col = 0; col < n; ++col)
        for (unsigned row = 0; row < m; ++row) {
            const uint16_t got = c[(size_t)row * n + col];
            EXPECT(col == 7 ? (got & 0x7fffu) > 0x7f80u : got == (row ? 0x3f68u : 0x3f8cu));
        }
}

// ---- the exact MoE entry ---------------------------------------------------------------------------------------------------------------------

static void run_moe_pair(int a_type, int b_type, unsigned E, unsigned m, unsigned n, unsigned k, const std::vector<int32_t> &off, unsigned seed) {
    const bool mx = is_mx(b_type), bf16 = a_type == kTypeBf16;
    const unsigned group = mx ? kMxGroup : kNvGroup, a_rows = m / 2 + 1, c_rows = m + 2;
    std::mt19937 rng(seed);
    const size_t w_words = (size_t)n * k / 8, s_bytes = (size_t)n * k / group;
    std::vector<uint32_t> pw(E * w_words);
    std::vector<uint8_t> ps(E * s_bytes);
    for (auto &w : pw)
        w = rng();
    for (auto &s : ps)
        s = mx ? (uint8_t)(126 + rng() % 3) : (uint8_t)(0x30 + rng() % 0x18);
    std::vector<uint16_t> a((size_t)a_rows * k), bias((size_t)E * n), c((size_t)c_rows * n, 0x7fc1u), ref(n), zero(k, 0);
    for (auto &v : a)
        v = (uint16_t)f32_h16_quiet_nan(bf16, (float)((int)(rng() % 9) - 4) * 0.25f);
    for (auto &v : bias)
        v = (uint16_t)f32_h16_quiet_nan(bf16, (float)((int)(rng() % 17) - 8));
    std::vector<float> gs(E);
    for (auto &g : gs)
        g = 0.125f * (float)(1 + rng() % 5);
    std::vector<int32_t> a_idx(m), c_idx(m);
    for (unsigned r = 0; r < m; ++r) {
        a_idx[r] = r % 5 == 4 ? (r % 2 ? -1 : (int32_t)a_rows) : (int32_t)(rng() % a_rows); // some out of range: zero rows
        c_idx[r] = r % 7 == 6 ? (int32_t)c_rows + 3 : (int32_t)(m - 1 - r);                 // a permutation, some out of range: skipped
    }
    EXPECT(moe_gemm_host(c.data(), a.data(), pw.data(), ps.data(), gs.data(), bias.data(), off.data(), E, m, n, k, a_idx.data(), a_rows,
                         c_idx.data(), c_rows, a_type, b_type) == kRcOk);
    const std::vector<int> own = owners(off, m);
    std::vector<char> written(c_rows, 0);
    for (unsigned r = 0; r < m; ++r) {
        if (own[r] < 0 || (unsigned)c_idx[r] >= c_rows)
            continue;
        const unsigned e = (unsigned)own[r];
        const uint16_t *row = (unsigned)a_idx[r] < a_rows ? a.data() + (size_t)a_idx[r] * k : zero.data();
        EXPECT(gemm_host(ref.data(), row, pw.data() + e * w_words, ps.data() + e * s_bytes, &gs[e], bias.data() + (size_t)e * n, 1, n, k, a_type,
                         b_type) == kRcOk);
        written[c_idx[r]] = 1;
        for (unsigned col = 0; col < n; ++col)
            EXPECT(c[(size_t)c_idx[r] * n + col] == ref[col]);
    }
    for (unsigned r = 0; r < c_rows; ++r)
        if (!written[r])
            for (unsigned col = 0; col < n; ++col)
                EXPECT(c[(size_t)r * n + col] == 0x7fc1u); // rows of no expert, and rows nothing names: untouched
}

// e8m0 scale byte 0 is 2^-127, as in the dense twin: expert 1 of 2 has every weight +6 under byte 0 (expert 0: -6 under byte 127), the one
// A row holds 2^120 once -> expert 1's rows hold 6 * 2^-127 * 2^120 * gs[1] = 1.5 * 2^-4, expert 0's -6 * 2^120.
static void run_moe_e8m0_byte0() {
    const unsigned E = 2, m = 3, n = 32, k = 256;
    const size_t w_words = (size_t)n * k / 8, s_bytes = (size_t)n * k / kMxGroup;
    std::vector<uint32_t> pw(E * w_words, 0xffffffffu);
    std::vector<uint8_t> ps(E * s_bytes, 127u);
    std::fill(pw.begin() + w_words, pw.end(), 0x77777777u);
    std::fill(ps.begin() + s_bytes, ps.end(), (uint8_t)0u);
    std::vector<uint16_t> a(k, 0u), c((size_t)m * n, 0x7fc1u);
    a[77] = 0x7b80u; // 2^120
    const std::vector<float> gs = {1.0f, 2.0f};
    const std::vector<int32_t> off = {0, 1, 3}, a_idx = {0, 0, 5}; // (grouped row 2 reads no row: zeros)
    EXPECT(moe_gemm_host(c.data(), a.data(), pw.data(), ps.data(), gs.data(), nullptr, off.data(), E, m, n, k, a_idx.data(), 1, nullptr, m,
                         kTypeBf16, kTypeMx) == kRcOk);
    for (unsigned col = 0; col < n; ++col)
        EXPECT(c[col] == 0xfcc0u && c[n + col] == 0x3dc0u && c[2 * n + col] == 0u); // -1.5 * 2^122, 1.5 * 2^-4, 0
}

// ---- the dense native entry ------------------------------------------------------------------------------------------------------------------

// the code of the integer v in {0, +-1, +-2, +-3, +-4, +-6}: e4m3 byte, e2m3 6 bits, e2m1 nibble
static unsigned code_of(int fmt, int v) {
    static const int mags[6] = {0, 1, 2, 3, 4, 6};
    static const unsigned c8[6] = {0x00, 0x38, 0x40, 0x44, 0x48, 0x4c}, c6[6] = {0, 8, 16, 20, 24, 28}, c4[6] = {0, 2, 4, 5, 6, 7};
    const int a = v < 0 ? -v : v;
    unsigned i = 0;
    while (mags[i] != a)
        ++i;
    const unsigned sign = v < 0 ? (fmt == 8 ? 0x80u : fmt == 6 ? 32u : 8u) : 0u;
    return sign | (fmt == 8 ? c8[i] : fmt == 6 ? c6[i] : c4[i]);
}

// writes element (row, kk) of the image: the inverse of qact_element, stated from the layout notes
static void put_element(std::vector<uint8_t> &qa, unsigned m, unsigned k, int fmt, unsigned row, unsigned kk, unsigned code) {
    const unsigned kt = kk / 128, b = (kk % 128) / 32, i = kk % 32;
    const size_t tile_row = (size_t)kt * m + row;
    if (fmt == 8) {
        const unsigned col16 = (kk % 128) / 8, u16 = col16 >> 1, half = col16 & 1u;
        const unsigned pos = (u16 & 4u) | ((u16 & 1u) << 1) | ((u16 >> 1) & 1u);
        qa.at(tile_row * 128 + pos * 16 + half * 8 + kk % 8) = (uint8_t)code;
    } else if (fmt == 4) {
        qa.at(tile_row * 64 + 16 * b + i / 2) |= (uint8_t)(code << (4 * (i & 1u)));
    } else {
        const size_t lo = tile_row * 64 + 16 * b, hi = (size_t)m * (k / 2) + tile_row * 32 + 8 * ((b & 1u) * 2 + (b >> 1));
        auto at = [&](unsigned j) -> uint8_t & { return j < 16 ? qa.at(lo + j) : qa.at(hi + j - 16); };
        const unsigned bit = 6 * i;
        at(bit / 8) |= (uint8_t)(code << (bit % 8));
        if (bit % 8 > 2)
            at(bit / 8 + 1) |= (uint8_t)(code >> (8 - bit % 8));
    }
}

// exact quantised activations: the m-row image, its values, and every row as an image of its own
static void fill_exact_qact(std::mt19937 &rng, unsigned m, unsigned k, int fmt, std::vector<uint8_t> &qa, std::vector<double> &a64,
                            std::vector<std::vector<uint8_t>> &alone) {
    a64.assign((size_t)m * k, 0.0);
    static const int vals[11] = {0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6};
    qa.assign((size_t)qact_bytes(m, k, fmt), 0u);
    for (unsigned row = 0; row < m; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            const unsigned sbyte = 125 + rng() % 5;
            qa.at((size_t)m * (k / 8 * (unsigned)fmt) + ((size_t)(blk / 4) * m + row) * 4 + blk % 4) = (uint8_t)sbyte;
            EXPECT(qact_scale_byte(qa.data(), m, k, fmt, row, blk) == sbyte);
            for (unsigned i = 0; i < 32; ++i) {
                const unsigned kk = 32 * blk + i;
                const int v = (rng() & 1u) ? vals[rng() % 11] : 0;
                put_element(qa, m, k, fmt, row, kk, code_of(fmt, v));
                a64[(size_t)row * k + kk] = v * std::ldexp(1.0, (int)sbyte - 127);
            }
        }
    for (unsigned row = 0; row < m; ++row) // every element reads back through the header's decode
        for (unsigned kk = 0; kk < k; ++kk)
            EXPECT((double)qact_element(qa.data(), m, k, fmt, row, kk) * e8m0_f64(qact_scale_byte(qa.data(), m, k, fmt, row, kk / 32)) ==
                   a64[(size_t)row * k + kk]);
    // a row alone is an image of its own (m = 1): the same elements at other addresses
    alone.assign(m, std::vector<uint8_t>((size_t)qact_bytes(1, k, fmt), 0u));
    for (unsigned row = 0; row < m; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            alone[row].at((size_t)(k / 8 * (unsigned)fmt) + (size_t)(blk / 4) * 4 + blk % 4) = (uint8_t)qact_scale_byte(qa.data(), m, k, fmt, row, blk);
            for (unsigned i = 0; i < 32; ++i) {
                const unsigned kk = 32 * blk + i;
                const double scale = e8m0_f64(qact_scale_byte(qa.data(), m, k, fmt, row, blk));
                put_element(alone[row], 1, k, fmt, 0, kk, code_of(fmt, (int)std::lround(a64[(size_t)row * k + kk] / scale)));
            }
        }
}

static void run_native_pair(int a_type, int fmt, unsigned m, unsigned n, unsigned k, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<uint32_t> pw;
    std::vector<uint8_t> ps, qa;
    std::vector<double> w, a64;
    std::vector<std::vector<uint8_t>> alone;
    fill_exact_weights(rng, n, k, true, 126, pw, ps, w);
    fill_exact_qact(rng, m, k, fmt, qa, a64, alone);
    check_exact_problem(rng, m, n, k, a_type == kTypeBf16, a64, w, [&](uint16_t *c, int row, const float *gs, const uint16_t *bias) {
        return row < 0 ? native_gemm_host(c, qa.data(), pw.data(), ps.data(), gs, bias, m, n, k, a_type, fmt)
                       : native_gemm_host(c, alone[row].data(), pw.data(), ps.data(), gs, bias, 1, n, k, a_type, fmt);
    });
}

// ---- the native MoE entry --------------------------------------------------------------------------------------------------------------------

// the image of grouped row `row` alone (m = 1): per k-tile the row's data bytes, MXFP6's second image, and its four scale bytes
static std::vector<uint8_t> row_image(const std::vector<uint8_t> &qa, unsigned m, unsigned k, int fmt, unsigned row) {
    const unsigned row_b = fmt == 8 ? 128u : 64u, per_row = k / 8 * (unsigned)fmt;
    std::vector<uint8_t> out((size_t)((uint64_t)per_row + k / 32), 0u);
    for (unsigned kt = 0; kt < k / 128; ++kt) {
        for (unsigned i = 0; i < row_b; ++i)
            out.at((size_t)kt * row_b + i) = qa.at(((size_t)kt * m + row) * row_b + i);
        if (fmt == 6)
            for (unsigned i = 0; i < 32; ++i)
                out.at((size_t)(k / 2) + (size_t)kt * 32 + i) = qa.at((size_t)m * (k / 2) + ((size_t)kt * m + row) * 32 + i);
        for (unsigned i = 0; i < 4; ++i)
            out.at((size_t)per_row + (size_t)kt * 4 + i) = qa.at((size_t)m * per_row + ((size_t)kt * m + row) * 4 + i);
    }
    return out;
}

static void run_native_moe_pair(int a_type, int fmt, unsigned E, unsigned m, unsigned n, unsigned k, unsigned seed) {
    const bool bf16 = a_type == kTypeBf16;
    std::mt19937 rng(seed);
    const size_t w_words = (size_t)n * k / 8, s_bytes = (size_t)n * k / kMxGroup;
    std::vector<uint32_t> pw(E * w_words);
    std::vector<uint8_t> ps(E * s_bytes);
    for (auto &x : pw)
        x = rng();
    for (auto &x : ps)
        x = (uint8_t)(124 + rng() % 7);
    std::vector<uint8_t> qa((size_t)qact_bytes(m, k, fmt));
    const size_t scale_at = (size_t)m * (k / 8 * (unsigned)fmt);
    for (size_t i = 0; i < qa.size(); ++i) // any element code (e4m3: not the two NaN codes); scale bytes around 2^0
        qa[i] = i < scale_at ? (uint8_t)((rng() & 0xffu) % 0x7fu | (rng() & 0x80u)) : (uint8_t)(122 + rng() % 9);
    std::vector<float> gs(E);
    std::vector<uint16_t> bias((size_t)E * n);
    for (auto &g : gs)
        g = 0.5f + (float)(rng() % 64) / 128.f;
    for (auto &b : bias)
        b = (uint16_t)f32_h16_quiet_nan(bf16, (float)((int)(rng() % 33) - 16) * 0.25f);

    const unsigned c_rows = m + 2;
    std::vector<int32_t> c_idx(m);
    for (unsigned r = 0; r < m; ++r)
        c_idx[r] = (int32_t)((r * 7 + 3) % c_rows);
    if (m > 3)
        c_idx[1] = (int32_t)c_rows, c_idx[3] = -2; // outside [0, c_rows): stores nothing
    for (const auto &off : routings(E, m))
        for (int with_idx = 0; with_idx < 2; ++with_idx)
            for (int with_bias = 0; with_bias < 2; ++with_bias) {
                const unsigned rows_out = with_idx ? c_rows : m;
                std::vector<uint16_t> c((size_t)rows_out * n, 0x7fc1u), want((size_t)rows_out * n, 0x7fc1u), c1(n);
                EXPECT(native_moe_gemm_host(c.data(), qa.data(), pw.data(), ps.data(), gs.data(), with_bias ? bias.data() : nullptr, off.data(), E, m,
                                            n, k, with_idx ? c_idx.data() : nullptr, rows_out, a_type, fmt) == kRcOk);
                const std::vector<int> own = owners(off, m);
                for (unsigned r = 0; r < m; ++r) {
                    if (own[r] < 0)
                        continue;
                    const unsigned e = (unsigned)own[r];
                    const std::vector<uint8_t> img = row_image(qa, m, k, fmt, r);
                    EXPECT(native_gemm_host(c1.data(), img.data(), pw.data() + e * w_words, ps.data() + e * s_bytes, &gs[e],
                                            with_bias ? bias.data() + (size_t)e * n : nullptr, 1, n, k, a_type, fmt) == kRcOk);
                    const unsigned dst = with_idx ? (unsigned)c_idx[r] : r;
                    if (dst < rows_out)
                        for (unsigned col = 0; col < n; ++col)
                            want[(size_t)dst * n + col] = c1[col];
                }
                EXPECT(c == want); // rows of an expert: the dense twin's bits; every other row: the poison
            }
}

// ---- the native entries on NVFP4 images ------------------------------------------------------------------------------------------------------

// writes weight (row, kk) of a "petit-cdna4-nv6/1" image and the E8M0 byte of its block, stated from the layout notes of layout.h: lane
// 32 h + r of block (row / 32, kt) holds row r; its 24 bytes of instruction q are 16 in plane q and 8 at [q] of its unit of plane 2, element e at
// bits [6 e, 6 e + 6); the scale bytes follow all the elements, [N / 32][K / (128 KS)][64 lanes][2][KS]
static void put_nv6(std::vector<uint8_t> &img, unsigned n, unsigned k, unsigned row, unsigned kk, unsigned code, unsigned sbyte) {
    const unsigned blk = kk / 32, e = kk % 32, kt = blk / 4, q = (blk % 4) >> 1, h = blk & 1u, lane = h * 32 + row % 32;
    const size_t tile = ((size_t)(row / 32) * (k / 128) + kt) * 3072;
    auto at = [&](unsigned j) -> uint8_t & { return j < 16 ? img.at(tile + q * 1024 + lane * 16 + j) : img.at(tile + 2048 + lane * 16 + q * 8 + j - 16); };
    const unsigned bit = 6 * e;
    at(bit / 8) |= (uint8_t)(code << (bit % 8));
    if (bit % 8 > 2)
        at(bit / 8 + 1) |= (uint8_t)(code >> (8 - bit % 8));
    const unsigned ks = k % 1024 == 0 ? 8 : k % 512 == 0 ? 4 : 2, sp = kt / ks, t = kt % ks;
    img.at((size_t)(n / 32) * (k / 128) * 3072 + (((size_t)(row / 32) * (k / (128 * ks)) + sp) * 64 + lane) * (2 * ks) + q * ks + t) = (uint8_t)sbyte;
}

static void run_nv_native_pair(int a_type, int fmt, unsigned m, unsigned n, unsigned k, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<uint8_t> image(nv6_image_bytes(n, k), 0u), qa;
    std::vector<double> w((size_t)n * k), a64;
    std::vector<std::vector<uint8_t>> alone;
    static const int vals[11] = {0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6};
    for (unsigned row = 0; row < n; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            const unsigned sbyte = 126 + rng() % 3;
            for (unsigned i = 0; i < 32; ++i) {
                const int v = vals[rng() % 11];
                put_nv6(image, n, k, row, 32 * blk + i, code_of(6, v), sbyte);
                w[(size_t)row * k + 32 * blk + i] = v * std::ldexp(1.0, (int)sbyte - 127);
            }
        }
    for (unsigned row = 0; row < n; ++row) // every weight reads back through the header's decode
        for (unsigned kk = 0; kk < k; ++kk)
            EXPECT(nv6_weight_f64(image.data(), n, k, row, kk) == w[(size_t)row * k + kk]);
    fill_exact_qact(rng, m, k, fmt, qa, a64, alone);
    check_exact_problem(rng, m, n, k, a_type == kTypeBf16, a64, w, [&](uint16_t *c, int row, const float *gs, const uint16_t *bias) {
        return row < 0 ? nv_native_gemm_host(c, qa.data(), image.data(), gs, bias, m, n, k, a_type, fmt)
                       : nv_native_gemm_host(c, alone[row].data(), image.data(), gs, bias, 1, n, k, a_type, fmt);
    });
}

static void run_nv_native_moe_pair(int a_type, int fmt, unsigned E, unsigned m, unsigned n, unsigned k, unsigned seed) {
    const bool bf16 = a_type == kTypeBf16;
    std::mt19937 rng(seed);
    const size_t per = nv6_image_bytes(n, k), elems = nv6_elem_bytes(n, k);
    std::vector<uint8_t> images(E * per);
    for (size_t i = 0; i < images.size(); ++i) // any element bits; scale bytes around 2^0
        images[i] = i % per < elems ? (uint8_t)rng() : (uint8_t)(124 + rng() % 7);
    std::vector<uint8_t> qa((size_t)qact_bytes(m, k, fmt));
    const size_t scale_at = (size_t)m * (k / 8 * (unsigned)fmt);
    for (size_t i = 0; i < qa.size(); ++i)
        qa[i] = i < scale_at ? (uint8_t)((rng() & 0xffu) % 0x7fu | (rng() & 0x80u)) : (uint8_t)(122 + rng() % 9);
    std::vector<float> gs(E);
    std::vector<uint16_t> bias((size_t)E * n);
    for (auto &g : gs)
        g = 0.5f + (float)(rng() % 64) / 128.f;
    for (auto &b : bias)
        b = (uint16_t)f32_h16_quiet_nan(bf16, (float)((int)(rng() % 33) - 16) * 0.25f);
    const unsigned c_rows = m + 2;
    std::vector<int32_t> c_idx(m);
    for (unsigned r = 0; r < m; ++r)
        c_idx[r] = (int32_t)((r * 7 + 3) % c_rows);
    if (m > 3)
        c_idx[1] = (int32_t)c_rows, c_idx[3] = -2; // outside [0, c_rows): stores nothing
    for (const auto &off : routings(E, m))
        for (int with_idx = 0; with_idx < 2; ++with_idx) {
            const unsigned rows_out = with_idx ? c_rows : m;
            std::vector<uint16_t> c((size_t)rows_out * n, 0x7fc1u), want((size_t)rows_out * n, 0x7fc1u), c1(n);
            EXPECT(nv_native_moe_gemm_host(c.data(), qa.data(), images.data(), gs.data(), bias.data(), off.data(), E, m, n, k,
                                           with_idx ? c_idx.data() : nullptr, rows_out, a_type, fmt) == kRcOk);
            const std::vector<int> own = owners(off, m);
            for (unsigned r = 0; r < m; ++r) {
                if (own[r] < 0)
                    continue;
                const unsigned e = (unsigned)own[r];
                const std::vector<uint8_t> img = row_image(qa, m, k, fmt, r);
                EXPECT(nv_native_gemm_host(c1.data(), img.data(), images.data() + e * per, &gs[e], bias.data() + (size_t)e * n, 1, n, k, a_type,
                                           fmt) == kRcOk);
                const unsigned dst = with_idx ? (unsigned)c_idx[r] : r;
                if (dst < rows_out)
                    for (unsigned col = 0; col < n; ++col)
                        want[(size_t)dst * n + col] = c1[col];
            }
            EXPECT(c == want);
        }
}

// ---- the cases -------------------------------------------------------------------------------------------------------------------------------

static void check_dense() {
    const int pairs[3][2] = {{kTypeBf16, kTypeNv}, {kTypeBf16, kTypeMx}, {kTypeFp16, kTypeNv}};
    run_e8m0_ends();
    for (const auto &p : pairs) {
        run_pair(p[0], p[1], 3, 32, 256, 1);
        run_pair(p[0], p[1], 2, 48 - (is_mx(p[1]) ? 16 : 0), 768, 2); // three slices
        run_pair(p[0], p[1], 1, is_mx(p[1]) ? 32 : 16, 4352, 3);      // L = 512, a last slice half as long
    }
    // geometry and workspace arithmetic
    const unsigned shapes[][2] = {{16, 256}, {208, 768}, {16, 4352}, {8192, 8192}, {57344, 8192}, {8192, 28672}, {16, 1u << 22}};
    for (const auto &s : shapes) {
        unsigned S = 0, L = 0;
        geometry(s[0], s[1], kTypeBf16, kTypeNv, &S, &L);
        EXPECT(L % 256 == 0 && S >= 1 && S <= kMaxSlices && (uint64_t)S * L >= s[1] && (uint64_t)(S - 1) * L < s[1]);
        for (unsigned m : {1u, 17u, kSplitMaxM, kSplitMaxM + 1, 4096u, kMaxRows - 1}) {
            const Plan p = dense_plan(m, s[0], s[1], kTypeBf16, kTypeNv);
            EXPECT(p.slices == S && p.slice_k == L && slabs(p) == (m <= kSplitMaxM ? S : 1u));
            const uint64_t want = m <= kSplitMaxM ? ((uint64_t)S * m * s[0] * 4 + 255) / 256 * 256 : 0;
            EXPECT(p.workspace_bytes == want && p.quant_bytes == 0);
        }
    }
    // the grids: n-tiles / 4 x S x m-tiles of 16 and the fold's min(ceil(count / 256), 4096); n-tile pairs / 4 x m-blocks of 64
    {
        const Plan s = dense_plan(17, 208, 768, kTypeBf16, kTypeNv), w = dense_plan(200, 208, 768, kTypeBf16, kTypeNv);
        const Plan g = plan(dense_call(200, 192, 768, kTypeBf16, kTypeNv, 1)), big = dense_plan(32, 57344, 8192, kTypeBf16, kTypeNv);
        EXPECT(s.split && s.slices == 3 && s.gemm.grid_x == 4 && s.gemm.grid_y == 3 && s.gemm.grid_z == 2 && s.gemm.tile_m == 16);
        EXPECT(s.fold.grid_x == 4 && s.fold.grid_y == 1 && s.fold.grid_z == 1); // ceil(17 * 52 / 256)
        EXPECT(!w.split && w.gemm.grid_x == 2 && w.gemm.grid_y == 4 && w.gemm.grid_z == 1 && w.gemm.tile_m == 64); // 7 pairs
        EXPECT(!g.split && g.gemm.grid_x == 2 && g.gemm.grid_y == 4);                                            // gated: 6 pairs
        EXPECT(big.split && big.gemm.grid_x == 896 && big.gemm.grid_z == 2 && big.fold.grid_x == 1792);          // 32 * 14336 / 256
        EXPECT(dense_plan(32, 1u << 20, 256, kTypeBf16, kTypeNv).fold.grid_x == 4096);
    }
    // refusals
    EXPECT(shape_rc(4, 32, 256, kTypeBf16, kTypeNv, 0) == kRcOk && shape_rc(0, 32, 256, kTypeFp16, kTypeNv, 2) == kRcOk);
    EXPECT(shape_rc(4, 24, 256, kTypeBf16, kTypeNv, 0) == kRcProblemShape && shape_rc(4, 32, 128, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(shape_rc(4, 0, 256, kTypeBf16, kTypeNv, 0) == kRcProblemShape && shape_rc(4, 32, 0, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(shape_rc(kMaxRows, 32, 256, kTypeBf16, kTypeNv, 0) == kRcProblemShape && shape_rc(4, 48, 256, kTypeBf16, kTypeNv, 1) == kRcProblemShape);
    EXPECT(shape_rc(4, 32, 256, 3, kTypeNv, 0) == kRcBadArgument && shape_rc(4, 32, 256, kTypeBf16, 5, 0) == kRcBadArgument);
    EXPECT(shape_rc(4, 32, 256, kTypeBf16, kTypeNv, 3) == kRcBadArgument && shape_rc(4, 32, 256, kTypeBf16, kTypeNv, -1) == kRcBadArgument);
    EXPECT(shape_rc(4, 32, 256, kTypeFp16, kTypeMx, 0) == kRcKernelShape && shape_rc(4, 32, 256, kTypeFp16, kTypeMxF16Range, 0) == kRcKernelShape);
    EXPECT(shape_rc(4, 48, 256, kTypeBf16, kTypeMx, 0) == kRcProblemShape && shape_rc(4, 48, 256, kTypeBf16, kTypeNv, 0) == kRcOk);
    EXPECT(dense_plan(4, 32, 256, kTypeFp16, kTypeMx).workspace_bytes == 0 && dense_plan(4, 24, 256, kTypeBf16, kTypeNv).workspace_bytes == 0);
    alignas(256) static char buf[512];
    void *ok = buf, *odd = buf + 8, *odd4 = buf + 4;
    EXPECT(pointers_rc(ok, ok, ok, ok, nullptr, ok, 256) == kRcOk && pointers_rc(ok, ok, ok, ok, odd, nullptr, 0) == kRcOk);
    EXPECT(pointers_rc(nullptr, ok, ok, ok, nullptr, ok, 256) == kRcProblemShape && pointers_rc(ok, nullptr, ok, ok, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(pointers_rc(ok, ok, nullptr, ok, nullptr, ok, 256) == kRcProblemShape && pointers_rc(ok, ok, ok, nullptr, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(pointers_rc(odd, ok, ok, ok, nullptr, ok, 256) == kRcProblemShape && pointers_rc(ok, ok, ok, odd, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(pointers_rc(ok, ok, ok, ok, odd4, ok, 256) == kRcProblemShape);
    EXPECT(pointers_rc(ok, ok, ok, ok, nullptr, nullptr, 256) == kRcProblemShape && pointers_rc(ok, ok, ok, ok, nullptr, odd, 256) == kRcProblemShape);
    EXPECT(gemm_host(nullptr, ok, ok, ok, nullptr, nullptr, 1, 32, 256, kTypeBf16, kTypeNv) == kRcProblemShape);
    EXPECT(gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 32, 256, kTypeBf16, kTypeNv) == kRcOk);
}

static void check_moe() {
    const int pairs[3][2] = {{kTypeBf16, kTypeNv}, {kTypeBf16, kTypeMx}, {kTypeFp16, kTypeNv}};
    run_moe_e8m0_byte0();
    for (const auto &p : pairs) {
        run_moe_pair(p[0], p[1], 3, 9, 32, 256, {0, 4, 4, 9}, 1);          // well formed, an empty expert
        run_moe_pair(p[0], p[1], 4, 11, 32, 768, {2, 7, 3, -5, 40}, 2);    // rows before offsets[0] unowned; descending, negative, beyond m
        run_moe_pair(p[0], p[1], 2, 5, 32, 256, {-3, 2, 2}, 3);            // rows past the last offset unowned
        for (const auto &off : routings(4, 10))                            // the native entry's list
            run_moe_pair(p[0], p[1], 4, 10, 32, 256, off, 4);
    }
    // the form switch: monotone in both constants, a function of (m, E) alone
    EXPECT(moe_split(1, 8) && moe_split(kMoeSplitMaxM, 1024) && !moe_split(kMoeSplitMaxM + 1, 1024));
    for (unsigned E : {1u, 2u, 8u, 130u, 1024u}) {
        const uint64_t by_rows = (uint64_t)kMoeSplitMaxRowsPer * E, last = by_rows < kMoeSplitMaxM ? by_rows : kMoeSplitMaxM;
        EXPECT(moe_split((unsigned)last, E) && !moe_split((unsigned)last + 1, E));
    }
    // workspace arithmetic
    for (unsigned m : {1u, 8u, 9u, 17u, 256u, 257u, 2048u, 2049u, kMaxRows - 1})
        for (unsigned E : {1u, 8u, 130u, 1024u}) {
            unsigned S = 0, L = 0;
            geometry(208, 768, kTypeBf16, kTypeNv, &S, &L);
            const Plan p = moe_plan(E, m, 208, 768, kTypeBf16, kTypeNv);
            const uint64_t want = moe_split(m, E) ? ((uint64_t)S * m * 208 * 4 + 255) / 256 * 256 : 0;
            EXPECT(p.rc == kRcOk && p.workspace_bytes == want && p.split == moe_split(m, E));
            EXPECT(max_grid(p) < (1ull << 31));
        }
    // the grids, one linear index: (ceil(m / 16) + min(E, m)) x S x n-tiles / 4 and the fold's slots x ceil(16 * (n_out / 4) / 1024);
    // (ceil(m / 64) + min(E, m)) x n-tile pairs / 4
    {
        const Plan s = moe_plan(3, 8, 208, 768, kTypeBf16, kTypeNv), w = moe_plan(3, 200, 208, 768, kTypeBf16, kTypeNv);
        const Plan g = moe_plan(130, 200, 192, 768, kTypeBf16, kTypeNv, 1), wide = moe_plan(3, 8, 2048, 768, kTypeBf16, kTypeNv, 1);
        EXPECT(s.split && s.slices == 3 && s.gemm.grid_x == (1 + 3) * 3 * 4 && s.gemm.nblocks == 4 && s.gemm.slots == 4 && s.gemm.tile_m == 16);
        EXPECT(s.fold.grid_x == (1 + 3) * 1 && s.fold.nblocks == 1 && s.gemm.grid_y == 1 && s.gemm.grid_z == 1 && s.fold.grid_y == 1);
        EXPECT(!w.split && w.gemm.grid_x == (4 + 3) * 2 && w.gemm.nblocks == 2 && w.gemm.tile_m == 64 && w.fold.grid_x == 0);
        EXPECT(!g.split && g.gemm.grid_x == (4 + 130) * 2);                                       // gated: 6 pairs
        EXPECT(wide.split && wide.gemm.grid_x == (1 + 3) * 3 * 32 && wide.fold.grid_x == (1 + 3) * 4); // n_out 1024: 4 chunks
    }
    EXPECT(moe_plan(0, 4, 32, 256, kTypeBf16, kTypeNv).workspace_bytes == 0 && moe_plan(1025, 4, 32, 256, kTypeBf16, kTypeNv).workspace_bytes == 0);
    EXPECT(moe_plan(4, 4, 32, 256, kTypeFp16, kTypeMx).workspace_bytes == 0 && moe_plan(4, 0, 32, 256, kTypeBf16, kTypeNv).workspace_bytes == 0);
    // refusals
    const int32_t idx[4] = {0, 1, 2, 3};
    EXPECT(moe_shape_rc(4, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, kTypeNv, 0) == kRcOk);
    EXPECT(moe_shape_rc(0, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(moe_shape_rc(1025, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(moe_shape_rc(4, kMaxRows, 32, 256, idx, 4, idx, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(moe_shape_rc(4, 4, 24, 256, nullptr, 4, nullptr, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(moe_shape_rc(4, 4, 48, 256, nullptr, 4, nullptr, 4, kTypeBf16, kTypeMx, 0) == kRcProblemShape);
    EXPECT(moe_shape_rc(4, 4, 48, 256, nullptr, 4, nullptr, 4, kTypeBf16, kTypeNv, 1) == kRcProblemShape);
    EXPECT(moe_shape_rc(4, 4, 32, 128, nullptr, 4, nullptr, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(moe_shape_rc(4, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeFp16, kTypeMx, 0) == kRcKernelShape);
    EXPECT(moe_shape_rc(4, 4, 32, 256, nullptr, 4, nullptr, 4, 3, kTypeNv, 0) == kRcBadArgument);
    EXPECT(moe_shape_rc(4, 4, 32, 256, nullptr, 3, nullptr, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape); // identity A index, too few rows
    EXPECT(moe_shape_rc(4, 4, 32, 256, idx, 3, nullptr, 3, kTypeBf16, kTypeNv, 0) == kRcProblemShape);     // identity C index, too few rows
    EXPECT(moe_shape_rc(4, 4, 32, 256, idx, 1, idx, 1, kTypeBf16, kTypeNv, 0) == kRcOk);
    EXPECT(moe_shape_rc(4, 4, 32, 256, idx, (1u << 22), idx, 4, kTypeBf16, kTypeNv, 0) == kRcOk);          // a_rows * k * 2 == 2^31
    EXPECT(moe_shape_rc(4, 4, 32, 256, idx, (1u << 22) + 1, idx, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape);
    EXPECT(moe_shape_rc(1024, kMaxRows - 1, 1u << 25, 256, idx, 4, idx, 4, kTypeBf16, kTypeNv, 0) == kRcProblemShape); // 2^31 workgroups
    alignas(256) static char buf[512];
    void *ok = buf, *odd2 = buf + 2, *odd8 = buf + 8;
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, ok, nullptr, nullptr, nullptr, ok, 256) == kRcOk);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, ok, ok, ok, odd8, nullptr, 0) == kRcOk);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, nullptr, ok, nullptr, nullptr, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, nullptr, nullptr, nullptr, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, odd2, ok, nullptr, nullptr, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, odd2, nullptr, nullptr, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, ok, odd2, nullptr, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, ok, nullptr, odd2, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(nullptr, ok, ok, ok, ok, ok, nullptr, nullptr, nullptr, ok, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, ok, nullptr, nullptr, nullptr, nullptr, 256) == kRcProblemShape);
    EXPECT(moe_pointers_rc(ok, ok, ok, ok, ok, ok, nullptr, nullptr, nullptr, odd8, 256) == kRcProblemShape);
    EXPECT(moe_gemm_host(nullptr, ok, ok, ok, (const float *)ok, nullptr, idx, 1, 1, 32, 256, nullptr, 1, nullptr, 1, kTypeBf16, kTypeNv) == kRcProblemShape);
    EXPECT(moe_gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0, 32, 256, nullptr, 0, nullptr, 0, kTypeBf16, kTypeNv) == kRcOk);
}

static void check_native() {
    for (int a_type : {kTypeBf16, kTypeFp16})
        for (int fmt : {8, 6, 4}) {
            run_native_pair(a_type, fmt, 3, 32, 256, 1);
            run_native_pair(a_type, fmt, 2, 64, 768, 2);  // three slices
            run_native_pair(a_type, fmt, 1, 32, 4352, 3); // L = 512, a last slice half as long
        }
    // element tables
    EXPECT(e2m3_f32(0) == 0.f && e2m3_f32(1) == 0.125f && e2m3_f32(7) == 0.875f && e2m3_f32(8) == 1.f);
    EXPECT(e2m3_f32(15) == 1.875f && e2m3_f32(16) == 2.f && e2m3_f32(31) == 7.5f && e2m3_f32(63) == -7.5f);
    EXPECT(e4m3_f32(0x38) == 1.f && e4m3_f32(0x7e) == 448.f && e4m3_f32(0x01) == 0x1p-9f && std::isnan(e4m3_f32(0x7f)));
    EXPECT(e8m0_f64(0) == 0x1p-127 && e8m0_f64(127) == 1.0 && e8m0_f64(254) == 0x1p127);
    // workspace arithmetic
    const unsigned shapes[][2] = {{64, 1024}, {4096, 2304}, {128, 256}, {8192, 8192}, {57344, 8192}, {8192, 28672}};
    for (const auto &s : shapes) {
        unsigned S = 0, L = 0;
        geometry(s[0], s[1], kTypeBf16, kTypeMx, &S, &L);
        for (unsigned m : {1u, 17u, kNativeSplitMaxM, kNativeSplitMaxM + 1, 4096u, 65535u})
            for (int fmt : {8, 6, 4}) {
                const bool split = m <= kNativeSplitMaxM;
                EXPECT(slabs(native_plan(m, s[0], s[1], kTypeFp16, fmt, 1)) == (split ? S : 1u));
                const uint64_t slab = split ? ((uint64_t)S * m * s[0] * 4 + 255) / 256 * 256 : 0;
                const uint64_t q = ((uint64_t)m * (s[1] / 8 * (unsigned)fmt) + (uint64_t)m * (s[1] / 32) + 255) / 256 * 256;
                EXPECT(native_plan(m, s[0], s[1], kTypeBf16, fmt, 1).workspace_bytes == slab);
                const Plan p = native_plan(m, s[0], s[1], kTypeBf16, fmt, 0);
                EXPECT(p.workspace_bytes == q + slab && p.quant_bytes == q && p.slab_bytes == slab);
            }
    }
    // the grids: pairs of n-tiles / 4 x S x m-tiles of 32 and the exact class's fold; slots of two pairs / 4 x m-blocks of 64
    {
        const Plan s = native_plan(33, 4096, 2304, kTypeBf16, 8, 0), w = native_plan(200, 4096, 2304, kTypeBf16, 8, 0);
        const Plan g = plan(native_call(200, 192, 768, kTypeBf16, 6, 1, 2));
        EXPECT(s.split && s.slices == 5 && s.gemm.grid_x == 32 && s.gemm.grid_y == 5 && s.gemm.grid_z == 2 && s.gemm.tile_m == 32);
        EXPECT(s.fold.grid_x == 132 && s.fold.grid_y == 1 && s.fold.grid_z == 1); // 33 * 1024 / 256
        EXPECT(!w.split && w.gemm.grid_x == 16 && w.gemm.grid_y == 4 && w.gemm.grid_z == 1 && w.gemm.tile_m == 64); // 128 pairs, 64 slots
        EXPECT(!g.split && g.gemm.grid_x == 1 && g.gemm.grid_y == 4);                                             // gated: 6 pairs, 3 slots
    }
    // refusals
    EXPECT(native_shape_rc(4, 32, 256, kTypeBf16, 8, 0, 0) == kRcOk && native_shape_rc(0, 64, 256, kTypeFp16, 4, 1, 2) == kRcOk);
    EXPECT(native_shape_rc(4, 48, 256, kTypeBf16, 8, 0, 0) == kRcProblemShape && native_shape_rc(4, 32, 128, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(native_shape_rc(4, 0, 256, kTypeBf16, 8, 0, 0) == kRcProblemShape && native_shape_rc(4, 32, 0, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(native_shape_rc(kMaxRows, 32, 256, kTypeBf16, 8, 1, 0) == kRcProblemShape && native_shape_rc(4, 96, 256, kTypeBf16, 8, 0, 1) == kRcProblemShape);
    EXPECT(native_shape_rc(4, 32, 256, 3, 8, 0, 0) == kRcBadArgument && native_shape_rc(4, 32, 256, kTypeBf16, 5, 0, 0) == kRcBadArgument);
    EXPECT(native_shape_rc(4, 32, 256, kTypeBf16, 8, 0, 3) == kRcBadArgument && native_shape_rc(4, 32, 256, kTypeBf16, 8, 0, -1) == kRcBadArgument);
    EXPECT(native_shape_rc(65536, 32, 256, kTypeBf16, 8, 0, 0) == kRcKernelShape && native_shape_rc(65536, 32, 256, kTypeBf16, 8, 1, 0) == kRcOk);
    EXPECT(native_plan(4, 48, 256, kTypeBf16, 8, 0).workspace_bytes == 0 && native_plan(0, 32, 256, kTypeBf16, 8, 0).workspace_bytes == 0);
    alignas(256) static char buf[512];
    void *ok = buf;
    EXPECT(native_gemm_host(nullptr, ok, ok, ok, nullptr, nullptr, 1, 32, 256, kTypeBf16, 8) == kRcProblemShape);
    EXPECT(native_gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 32, 256, kTypeBf16, 8) == kRcOk);
}

static void check_native_moe() {
    for (int a_type : {kTypeBf16, kTypeFp16})
        for (int fmt : {8, 6, 4}) {
            run_native_moe_pair(a_type, fmt, 4, 10, 32, 256, 1);
            run_native_moe_pair(a_type, fmt, 3, 7, 64, 768, 2);   // three slices
            run_native_moe_pair(a_type, fmt, 5, 6, 32, 4352, 3);  // L = 512, a last slice half as long
            run_native_moe_pair(a_type, fmt, 70, 9, 32, 256, 4);  // more experts than one 64-expert chunk, most of them empty
        }
    // the form rule: split iff ceil(m / min(E, m)) <= kMoeSplitMaxRowsPer and m <= kMoeSplitMaxM -- the exact entry's rule
    for (unsigned E : {1u, 3u, 8u, 65u, 130u, 1024u})
        for (unsigned m = 1; m < 300; ++m) {
            const unsigned active = E < m ? E : m;
            EXPECT(native_moe_split(m, E) == ((m + active - 1) / active <= kMoeSplitMaxRowsPer && m <= kMoeSplitMaxM));
            EXPECT(native_moe_split(m, E) == moe_split(m, E));
        }
    EXPECT(native_moe_split(0, 8) && moe_split(0, 8));
    // workspace arithmetic
    const unsigned shapes[][2] = {{64, 1024}, {64, 4352}, {128, 256}, {96, 512}, {6144, 3072}, {3072, 3072}};
    for (const auto &s : shapes) {
        unsigned S = 0, L = 0;
        geometry(s[0], s[1], kTypeBf16, kTypeMx, &S, &L);
        for (unsigned E : {3u, 128u})
            for (unsigned m : {1u, 8u, 9u, 64u, 4096u, 70000u})
                for (int fmt : {8, 6, 4}) {
                    const bool split = native_moe_split(m, E);
                    const uint64_t slab = split ? ((uint64_t)S * m * s[0] * 4 + 255) / 256 * 256 : 0;
                    const uint64_t q = ((uint64_t)m * (s[1] / 8 * (unsigned)fmt) + (uint64_t)m * (s[1] / 32) + 255) / 256 * 256;
                    EXPECT(native_moe_plan(E, m, s[0], s[1], kTypeFp16, fmt, 1).workspace_bytes == slab);
                    EXPECT(native_moe_plan(E, m, s[0], s[1], kTypeBf16, fmt, 0).workspace_bytes == q + slab);
                }
    }
    EXPECT(native_moe_plan(3, 4, 48, 256, kTypeBf16, 8, 0).workspace_bytes == 0 && native_moe_plan(3, 0, 32, 256, kTypeBf16, 8, 0).workspace_bytes == 0);
    EXPECT(native_moe_plan(0, 4, 32, 256, kTypeBf16, 8, 0).workspace_bytes == 0 && native_moe_plan(1025, 4, 32, 256, kTypeBf16, 8, 0).workspace_bytes == 0);
    // refusals
    alignas(256) static char buf[512];
    const int32_t *idx = (const int32_t *)buf;
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcOk);
    EXPECT(native_moe_shape_rc(3, 70000, 32, 256, nullptr, 70000, nullptr, 70000, kTypeFp16, 6, 0, 0) == kRcOk); // no 65535-row limit
    EXPECT(native_moe_shape_rc(3, 4, 48, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(native_moe_shape_rc(3, 4, 32, 128, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(native_moe_shape_rc(3, kMaxRows, 32, 256, idx, 4, idx, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(native_moe_shape_rc(3, 4, 96, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 1) == kRcProblemShape);
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, 3, 8, 0, 0) == kRcBadArgument);
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 5, 0, 0) == kRcBadArgument);
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 3) == kRcBadArgument);
    EXPECT(native_moe_shape_rc(0, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(native_moe_shape_rc(1025, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, nullptr, 3, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);  // a NULL A index, 3 rows
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, idx, 3, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcOk);
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 3, kTypeBf16, 8, 0, 0) == kRcProblemShape);  // a NULL C index, 3 rows
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, nullptr, 0, nullptr, 4, kTypeBf16, 8, 1, 0) == kRcOk);            // quantised: a_rows is not read
    EXPECT(native_moe_shape_rc(3, 4, 32, 256, idx, 4, nullptr, 4, kTypeBf16, 8, 1, 0) == kRcBadArgument);       // quantised with an A index
    EXPECT(native_moe_shape_rc(3, 1u << 19, 32, 8192, nullptr, 0, idx, 4, kTypeBf16, 8, 1, 0) == kRcProblemShape);  // 2^32 quantised bytes
    EXPECT(native_moe_shape_rc(1024, kMaxRows - 1, 1u << 25, 256, nullptr, 0, idx, 4, kTypeBf16, 4, 1, 0) == kRcProblemShape); // 2^31 workgroups
    // the grids, one linear index: (ceil(m / 32) + min(E, m)) x S x pairs / 4 and the exact MoE fold over 16-row slots;
    // (ceil(m / 64) + min(E, m)) x slots of two pairs / 4
    {
        const Plan s = native_moe_plan(3, 8, 64, 1024, kTypeBf16, 8, 0), w = native_moe_plan(3, 200, 192, 512, kTypeBf16, 4, 1, 1);
        const Plan wide = native_moe_plan(3, 8, 4096, 256, kTypeBf16, 8, 1);
        EXPECT(s.split && s.slices == 4 && s.gemm.grid_x == (1 + 3) * 4 * 1 && s.gemm.tile_m == 32 && s.gemm.slots == 4 && s.gemm.nblocks == 1);
        EXPECT(s.fold.grid_x == (1 + 3) * 1 && s.fold.tile_m == 16 && max_grid(s) == (1 + 3) * 4 * 1);
        EXPECT(!w.split && w.gemm.grid_x == (4 + 3) * 1 && max_grid(w) == (4 + 3) * 1 && w.gemm.tile_m == 64);
        EXPECT(wide.split && wide.slices == 1 && wide.gemm.grid_x == (1 + 3) * 1 * 32 && wide.fold.grid_x == (1 + 3) * 16); // 4096 / 256 chunks
    }
    void *ok = buf;
    EXPECT(native_moe_gemm_host(nullptr, ok, ok, ok, (const float *)ok, nullptr, idx, 3, 1, 32, 256, nullptr, 1, kTypeBf16, 8) == kRcProblemShape);
    EXPECT(native_moe_gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, 32, 256, nullptr, 0, kTypeBf16, 8) == kRcOk);
}

static void check_nv_native() {
    alignas(256) static char buf[512];
    const void *ok = buf, *odd = buf + 16;
    auto nv_plan = [&](unsigned m, unsigned n, unsigned k, int a_type, int fmt, int quantized, int act = 0, const void *image = nullptr) {
        return plan(native_call(m, n, k, a_type, fmt, quantized, act, kTypeNv, image));
    };
    auto nv_moe_plan = [&](unsigned E, unsigned m, unsigned n, unsigned k, int a_type, int fmt, int quantized, int act = 0,
                           const void *images = nullptr) {
        return plan(moe_call(native_call(m, n, k, a_type, fmt, quantized, act, kTypeNv, images), E, false, m, false, m));
    };
    for (int a_type : {kTypeBf16, kTypeFp16})
        for (int fmt : {8, 6, 4}) {
            run_nv_native_pair(a_type, fmt, 2, 64, 1024, 1); // spans of 8 k-tiles
            run_nv_native_pair(a_type, fmt, 2, 96, 768, 2);  // spans of 2, three blocks of 32 rows, three slices
        }
    run_nv_native_pair(kTypeBf16, 8, 1, 32, 4352, 3); // L = 512, a last slice half as long
    for (int fmt : {8, 6, 4}) {
        run_nv_native_moe_pair(kTypeBf16, fmt, 4, 10, 64, 1024, 4);
        run_nv_native_moe_pair(kTypeFp16, fmt, 3, 7, 96, 768, 5);
    }
    // the plans are the MXFP4 native entries': the same geometry, forms, workspace and grids (a block of 32 weight rows for a pair of n-tiles)
    for (unsigned m : {1u, 33u, kNativeSplitMaxM, kNativeSplitMaxM + 1, 200u})
        for (int fmt : {8, 6, 4})
            for (int q : {0, 1}) {
                const Plan a = nv_plan(m, 4096, 2304, kTypeBf16, fmt, q), b = native_plan(m, 4096, 2304, kTypeBf16, fmt, q);
                EXPECT(a.rc == kRcOk && a.split == b.split && a.slices == b.slices && a.slice_k == b.slice_k && a.workspace_bytes == b.workspace_bytes &&
                       a.quant_bytes == b.quant_bytes && a.gemm.grid_x == b.gemm.grid_x && a.gemm.grid_y == b.gemm.grid_y &&
                       a.gemm.grid_z == b.gemm.grid_z && a.fold.grid_x == b.fold.grid_x);
            }
    for (unsigned m : {1u, 8u, 9u, 70u})
        for (unsigned E : {1u, 4u, 16u}) {
            const Plan a = nv_moe_plan(E, m, 128, 1536, kTypeFp16, 6, 0), b = native_moe_plan(E, m, 128, 1536, kTypeFp16, 6, 0);
            EXPECT(a.rc == kRcOk && a.split == b.split && a.slices == b.slices && a.workspace_bytes == b.workspace_bytes &&
                   a.gemm.grid_x == b.gemm.grid_x && a.fold.grid_x == b.fold.grid_x && a.gemm.nblocks == b.gemm.nblocks);
        }
    {
        const Plan s = nv_plan(33, 4096, 2304, kTypeBf16, 8, 0), w = nv_plan(200, 4096, 2304, kTypeBf16, 8, 0), g = nv_plan(200, 192, 768, kTypeBf16, 6, 1, 2);
        EXPECT(s.split && s.slices == 5 && s.gemm.grid_x == 32 && s.gemm.grid_y == 5 && s.gemm.grid_z == 2 && s.fold.grid_x == 132);
        EXPECT(!w.split && w.gemm.grid_x == 16 && w.gemm.grid_y == 4 && w.gemm.grid_z == 1);
        EXPECT(!g.split && g.gemm.grid_x == 1 && g.gemm.grid_y == 4);
        EXPECT(s.workspace_bytes == s.quant_bytes + s.slab_bytes && s.slab_bytes == (5ull * 33 * 4096 * 4 + 255) / 256 * 256);
        EXPECT(s.quant_bytes == (33ull * 2304 + 33ull * 72 + 255) / 256 * 256);
    }
    // refusals, in their order: the formats, the shape, the image's address, the quantiser's row limit
    EXPECT(nv_plan(4, 32, 256, kTypeBf16, 8, 0).rc == kRcOk && nv_plan(0, 64, 256, kTypeFp16, 4, 1, 2).rc == kRcOk);
    EXPECT(nv_plan(4, 32, 256, 3, 8, 0).rc == kRcBadArgument && nv_plan(4, 32, 256, kTypeBf16, 5, 0).rc == kRcBadArgument);
    EXPECT(nv_plan(4, 48, 256, kTypeBf16, 5, 0, 0, odd).rc == kRcBadArgument && nv_plan(4, 32, 256, kTypeBf16, 8, 0, 3).rc == kRcBadArgument);
    EXPECT(nv_plan(4, 48, 256, kTypeBf16, 8, 0).rc == kRcProblemShape && nv_plan(4, 16, 256, kTypeBf16, 8, 0).rc == kRcProblemShape);
    EXPECT(nv_plan(4, 32, 128, kTypeBf16, 8, 0).rc == kRcProblemShape && nv_plan(4, 96, 256, kTypeBf16, 8, 0, 1).rc == kRcProblemShape);
    EXPECT(nv_plan(4, 0, 256, kTypeBf16, 8, 0).rc == kRcProblemShape && nv_plan(kMaxRows, 32, 256, kTypeBf16, 8, 1).rc == kRcProblemShape);
    EXPECT(nv_plan(4, 1u << 17, 1u << 15, kTypeBf16, 8, 1).rc == kRcOk);              // 3 * 2^30 element bytes
    EXPECT(nv_plan(4, 1u << 18, 21760, kTypeBf16, 8, 1).rc == kRcOk);                 // the last k below the limit
    EXPECT(nv_plan(4, 1u << 18, 22016, kTypeBf16, 8, 1).rc == kRcProblemShape);       // n * k * 3 / 4 >= 2^32
    EXPECT(native_plan(4, 1u << 18, 22016, kTypeBf16, 8, 1).rc == kRcOk);             // (the raw MXFP4 entry has no such limit)
    EXPECT(nv_plan(4, 32, 256, kTypeBf16, 8, 0, 0, ok).rc == kRcOk && nv_plan(4, 32, 256, kTypeBf16, 8, 0, 0, odd).rc == kRcProblemShape);
    EXPECT(nv_plan(70000, 32, 256, kTypeBf16, 8, 0, 0, odd).rc == kRcProblemShape && nv_plan(70000, 48, 256, kTypeBf16, 8, 0).rc == kRcProblemShape);
    EXPECT(nv_plan(70000, 32, 256, kTypeBf16, 8, 0, 0, ok).rc == kRcKernelShape && nv_plan(70000, 32, 256, kTypeBf16, 8, 1).rc == kRcOk);
    EXPECT(native_plan(4, 32, 256, kTypeBf16, 8, 0).rc == kRcOk); // (an MXFP4 call never reads the address)
    EXPECT(nv_moe_plan(3, 70000, 32, 256, kTypeFp16, 6, 0).rc == kRcOk && nv_moe_plan(3, 4, 32, 256, kTypeBf16, 8, 0, 0, odd).rc == kRcProblemShape);
    EXPECT(nv_moe_plan(0, 4, 32, 256, kTypeBf16, 8, 0).rc == kRcProblemShape && nv_moe_plan(3, 4, 96, 256, kTypeBf16, 8, 0, 1).rc == kRcProblemShape);
    EXPECT(nv_plan(4, 48, 256, kTypeBf16, 8, 0).workspace_bytes == 0 && nv_plan(0, 32, 256, kTypeBf16, 8, 0).workspace_bytes == 0);
    EXPECT(nv_native_gemm_host(nullptr, ok, ok, nullptr, nullptr, 1, 32, 256, kTypeBf16, 8) == kRcProblemShape);
    EXPECT(nv_native_gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 32, 256, kTypeBf16, 8) == kRcOk);
    EXPECT(nv_native_moe_gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, 32, 256, nullptr, 0, kTypeBf16, 8) == kRcOk);
}

// ---- numfmt.h and the "petit-qact/1" functions of layout.h on their edge values ----------------------------------------------------------------

template <bool BF16> static void check_h16() {
    for (unsigned h = 0; h < 0x10000u; ++h) { // every pattern survives the round trip (fp16: a NaN comes back as the quiet 0x7e00 with its sign)
        const bool nan = BF16 ? (h & 0x7fffu) > 0x7f80u : (h & 0x7fffu) > 0x7c00u;
        const float x = h16_f32<BF16>(h);
        EXPECT(std::isnan(x) == nan && (nan || h16_f32(BF16, h) == x));
        EXPECT(f32_h16<BF16>(x) == ((nan && !BF16) ? (h & 0x8000u) | 0x7e00u : h));
        EXPECT(f32_h16_quiet_nan<BF16>(x) == ((nan && BF16) ? h | 0x40u : f32_h16<BF16>(x)));
        EXPECT(f32_h16_quiet_nan(BF16, x) == f32_h16_quiet_nan<BF16>(x));
    }
}

static void check_numfmt() {
    const float inf = INFINITY, nan = NAN;
    EXPECT(f32_bits(1.0f) == 0x3f800000u && f32_bits(-0.0f) == 0x80000000u && bits_f32(0x7f800000u) == inf && f32_bits(bits_f32(0x7fc12345u)) == 0x7fc12345u);
    // the 16-bit types: decode, ties to even, the ends of the range, NaN under both rules
    check_h16<true>();
    check_h16<false>();
    EXPECT(h16_f32<true>(0x3f80u) == 1.0f && h16_f32<false>(0x3c00u) == 1.0f && h16_f32<false>(1u) == 0x1p-24f && h16_f32<false>(0x03ffu) == 1023 * 0x1p-24f);
    EXPECT(h16_f32<false>(0x7bffu) == 65504.0f && h16_f32<false>(0xfc00u) == -inf && std::signbit(h16_f32<false>(0x8000u)) && h16_f32<false>(0x8000u) == 0.0f);
    EXPECT(f32_h16<true>(bits_f32(0x3f808000u)) == 0x3f80u && f32_h16<true>(bits_f32(0x3f818000u)) == 0x3f82u && f32_h16<true>(bits_f32(0x3f808001u)) == 0x3f81u);
    EXPECT(f32_h16<true>(bits_f32(0x7f7fffffu)) == 0x7f80u && f32_h16<true>(inf) == 0x7f80u && f32_h16<true>(-0.0f) == 0x8000u);
    EXPECT(f32_h16<true>(bits_f32(0x7f800001u)) == 0x7f80u && f32_h16<true>(bits_f32(0x7fffffffu)) == 0x8000u); // the integer rule on a NaN
    EXPECT(f32_h16_quiet_nan<true>(bits_f32(0x7f800001u)) == 0x7fc0u && f32_h16_quiet_nan<true>(bits_f32(0xffffffffu)) == 0xffffu);
    EXPECT(f32_h16<false>(65519.0f) == 0x7bffu && f32_h16<false>(65520.0f) == 0x7c00u && f32_h16<false>(inf) == 0x7c00u && f32_h16<false>(-1e30f) == 0xfc00u);
    EXPECT(f32_h16<false>(0x1p-25f) == 0u && f32_h16<false>(0x1.000002p-25f) == 1u && f32_h16<false>(0x1.8p-24f) == 2u && f32_h16<false>(0x1p-14f) == 0x0400u);
    EXPECT(f32_h16<false>(bits_f32(1u)) == 0u && f32_h16<false>(-bits_f32(1u)) == 0x8000u && f32_h16<false>(nan) == (0x7e00u | (f32_bits(nan) >> 16 & 0x8000u)));
    EXPECT(f32_h16<false>(1.0f + 0x1p-11f) == 0x3c00u && f32_h16<false>(1.0f + 0x1.8p-10f) == 0x3c02u);
    // e2m1: the table, every midpoint to the even code, saturation, the sign of zero
    static const float mag4[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    for (unsigned c = 0; c < 16; ++c) {
        EXPECT(e2m1_f32(c) == ((c & 8u) ? -mag4[c & 7u] : mag4[c & 7u]) && std::signbit(e2m1_f32(c)) == ((c & 8u) != 0));
        EXPECT(e2m1_rne((double)e2m1_f32(c)) == c);
    }
    for (unsigned i = 0; i < 7; ++i) {
        const double mid = (mag4[i] + mag4[i + 1]) / 2;
        EXPECT((double)kE2m1Mid[i] == mid && e2m1_rne(mid) == (i % 2 ? i + 1 : i) && e2m1_rne(-mid) == (8u | (i % 2 ? i + 1 : i)));
        EXPECT(e2m1_rne(std::nextafter(mid, 0.0)) == i && e2m1_rne(std::nextafter(mid, 9.0)) == i + 1);
    }
    EXPECT(e2m1_rne(6.0) == 7u && e2m1_rne(1e300) == 7u && e2m1_rne((double)inf) == 7u && e2m1_rne(-(double)inf) == 15u && (e2m1_rne((double)nan) & 7u) == 0u);
    EXPECT(e2m1_rne(0x1p-1074) == 0u && e2m1_rne(-0x1p-1074) == 8u);
    // e4m3: every byte decodes and encodes back; subnormals, ties, saturation, NaN; the unsigned and the finite variants
    for (unsigned b = 0; b < 256; ++b) {
        const float x = e4m3_f32(b);
        EXPECT(std::isnan(x) == e4m3_is_nan(b) && std::signbit(x) == (b >= 128));
        if (e4m3_is_nan(b)) {
            EXPECT(e4m3_finite_f32(b) == (b & 0x80u ? -480.0f : 480.0f));
            continue;
        }
        EXPECT(e4m3_rne(x) == b && e4m3_finite_f32(b) == x && e4m3_mag_f32(b & 0x7fu) == std::fabs(x) && e4m3_rne_sat(std::fabs(x)) == (b & 0x7fu));
    }
    EXPECT(e4m3_f32(1) == 0x1p-9f && e4m3_f32(7) == 7 * 0x1p-9f && e4m3_f32(8) == 0x1p-6f && e4m3_f32(0x7e) == 448.0f && e4m3_f32(0xfe) == -448.0f);
    EXPECT(e4m3_rne(0x1p-10f) == 0u && e4m3_rne(0x1.8p-9f) == 2u && e4m3_rne(0x1.000002p-10f) == 1u && e4m3_rne(bits_f32(1u)) == 0u && e4m3_rne(-bits_f32(1u)) == 0x80u);
    EXPECT(e4m3_rne(1.0625f) == 0x38u && e4m3_rne(1.1875f) == 0x3au && e4m3_rne(0x1.fp-7f) == 0x08u && e4m3_rne(-0.0f) == 0x80u);
    EXPECT(e4m3_rne(448.0f) == 0x7eu && e4m3_rne(464.0f) == 0x7eu && e4m3_rne(1e30f) == 0x7eu && e4m3_rne(-inf) == 0xfeu && (e4m3_rne(nan) & 0x7fu) == 0x7eu);
    EXPECT(e4m3_rne_sat(nan) == 0x7eu && e4m3_rne_sat(inf) == 0x7eu && e4m3_rne_sat(447.9f) == 0x7eu && e4m3_rne_sat(431.9f) == 0x7du);
    // e2m3: every code decodes and encodes back; ties, saturation, the sign of zero
    for (unsigned c = 0; c < 64; ++c)
        EXPECT(e2m3_rne((double)e2m3_f32(c)) == c && std::signbit(e2m3_f32(c)) == (c >= 32));
    EXPECT(e2m3_f32(1) == 0.125f && e2m3_f32(7) == 0.875f && e2m3_f32(8) == 1.0f && e2m3_f32(31) == 7.5f && e2m3_f32(63) == -7.5f);
    EXPECT(e2m3_rne(0.0625) == 0u && e2m3_rne(0.1875) == 2u && e2m3_rne(0.9375) == 8u && e2m3_rne(1.0625) == 8u && e2m3_rne(1.9375) == 16u);
    EXPECT(e2m3_rne(7.25) == 30u && e2m3_rne(std::nextafter(7.25, 8.0)) == 31u && e2m3_rne(7.5) == 31u && e2m3_rne(7.75) == 31u && e2m3_rne(1e300) == 31u);
    EXPECT(e2m3_rne((double)inf) == 31u && e2m3_rne(-(double)inf) == 63u && e2m3_rne(0x1p-1074) == 0u && e2m3_rne(-0.0) == 32u && e2m3_rne((double)bits_f32(1u)) == 0u);
    // e8m0 as the kernels read it
    EXPECT(e8m0_f32(0) == 0x1p-127f && e8m0_f32(1) == 0x1p-126f && e8m0_f32(127) == 1.0f && e8m0_f32(254) == 0x1p127f && std::isinf(e8m0_f32(255)));
    EXPECT(e8m0_f64(0) == 0x1p-127 && e8m0_f64(254) == 0x1p127 && std::isinf(e8m0_f64(255)) && e8m0_f32(256 + 127) == 1.0f);
    // the activation block-scale rule: a zero block, subnormal and tiny maxima (byte 1), the largest, infinity and NaN (never 0 or 255)
    EXPECT(act_scale_byte<8>(0.f) == 127u && act_scale_byte<6>(0.f) == 127u && act_scale_byte<4>(-0.0f) == 127u);
    EXPECT(act_scale_byte<8>(1.0f) == 120u && act_scale_byte<8>(200.0f) == 127u && act_scale_byte<8>(255.9f) == 127u && act_scale_byte<8>(256.0f) == 128u);
    EXPECT(act_scale_byte<6>(1.0f) == 125u && act_scale_byte<6>(7.5f) == 127u && act_scale_byte<4>(6.0f) == 127u && act_scale_byte<4>(8.0f) == 128u);
    EXPECT(act_scale_byte<8>(bits_f32(1u)) == 1u && act_scale_byte<8>(0x1p-119f) == 1u && act_scale_byte<8>(0x1p-118f) == 2u && act_scale_byte<4>(0x1p-124f) == 1u);
    EXPECT(act_scale_byte<4>(0x1p-123f) == 2u && act_scale_byte<8>(bits_f32(0x7f7fffffu)) == 247u && act_scale_byte<4>(bits_f32(0x7f7fffffu)) == 252u);
    EXPECT(act_scale_byte<8>(inf) == 248u && act_scale_byte<6>(inf) == 253u && act_scale_byte<4>(nan) == 253u);
    for (int e = -10; e <= 9; ++e) // the image builder's variant on its whole domain
        for (float f : {1.0f, 1.5f, 1.9999999f})
            EXPECT(act_scale_byte_nv6(std::ldexp(f, e)) == act_scale_byte<6>(std::ldexp(f, e)) && act_scale_byte_nv6(std::ldexp(f, e)) == (unsigned)(e + 125));
    EXPECT(act_scale_byte_nv6(0.f) == 127u);
}

// every bit of the element regions and every byte of the scale region is named by exactly one (row, k), the last row and k-tile included; the
// sizes against the formula written out
static void check_qact_layout() {
    static const unsigned pos8[8] = {0, 2, 1, 3, 4, 6, 5, 7}, slot6[4] = {0, 2, 1, 3};
    for (unsigned u = 0; u < 8; ++u) // the order [0-15][32-47][16-31][48-63][64-79][96-111][80-95][112-127]
        EXPECT(qact_fp8_unit_pos(u) == pos8[u]);
    for (unsigned b = 0; b < 4; ++b) // blocks 0, 2, 1, 3
        EXPECT(qact_fp6_hi_slot(b) == slot6[b]);
    EXPECT(qact_row_bytes(8) == 128u && qact_row_bytes(6) == 64u && qact_row_bytes(4) == 64u && kQactHiRowBytes == 32u && kQactScaleRowBytes == 4u);
    const unsigned shapes[][2] = {{1, 128}, {1, 256}, {5, 768}, {33, 256}, {130, 384}};
    for (const auto &s : shapes)
        for (int act : {8, 6, 4}) {
            const unsigned m = s[0], k = s[1];
            const size_t elems = qact_elem_bytes(m, k, act), total = qact_bytes(m, k, act);
            EXPECT(elems == (size_t)m * k * act / 8 && qact_scale_bytes(m, k) == (size_t)m * k / 32 && total == elems + (size_t)m * k / 32);
            EXPECT(qact_lo_bytes(m, k, act) == (act == 6 ? (size_t)m * k / 2 : elems) && qact_hi_offset(m, k) == qact_lo_bytes(m, k, 6));
            std::vector<uint8_t> bits(elems * 8, 0), scale(total - elems, 0);
            for (unsigned row = 0; row < m; ++row)
                for (unsigned kk = 0; kk < k; ++kk) {
                    const unsigned kt = kk / 128, b = kk % 128 / 32, i = kk % 32, col16 = kk % 128 / 8;
                    const size_t tile_row = qact_tile_row(m, kt, row), lo = tile_row * qact_row_bytes(act);
                    if (act == 8) {
                        for (unsigned j = 0; j < 8; ++j)
                            ++bits.at((lo + qact_fp8_unit_pos(col16 >> 1) * 16 + (col16 & 1u) * 8 + kk % 8) * 8 + j);
                    } else if (act == 4) {
                        for (unsigned j = 0; j < 4; ++j)
                            ++bits.at((lo + 16 * b + i / 2) * 8 + 4 * (i & 1u) + j);
                    } else {
                        const size_t hi = qact_hi_offset(m, k) + tile_row * kQactHiRowBytes + 8 * qact_fp6_hi_slot(b);
                        for (unsigned j = 6 * i; j < 6 * i + 6; ++j)
                            ++bits.at((j < 128 ? lo + 16 * b : hi - 16) * 8 + j);
                    }
                    if (i == 0)
                        ++scale.at(qact_scale_dword(m, kt, row) * kQactScaleRowBytes + b);
                }
            EXPECT(std::count(bits.begin(), bits.end(), 1) == (long)bits.size() && std::count(scale.begin(), scale.end(), 1) == (long)scale.size());
        }
    // the largest image the entries accept stays below their 32-bit limit by the same count
    EXPECT(qact_bytes(1u << 20, 4096, 8) == (1ull << 32) + (1ull << 27) && qact_bytes(0, 4096, 8) == 0 && qact_hi_offset(1u << 20, 8192) == 1ull << 32);
}

int main() {
    check_numfmt();
    check_qact_layout();
    check_dense();
    check_moe();
    check_native();
    check_native_moe();
    check_nv_native();
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
