// tools/native_moe_invariant_hostcheck.cc -- a stand-alone program around the host side of the batch-invariant MoE launch on the native class
// (petit-kernel_amd/csrc/gemm_native_invariant_moe_host.h: the form rule, the workspace arithmetic, the argument checks, the CPU twin), for
// sanitizer runs on the CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipetit-kernel_amd/csrc \
//         tools/native_moe_invariant_hostcheck.cc -o native_moe_invariant_hostcheck && ./native_moe_invariant_hostcheck
//
// It fills buffers of exactly the bytes the layouts declare (so that an index outside them is a heap overflow the sanitizer sees) with random
// experts and a random quantised image of m grouped rows of every (type, activation format) pair, runs the MoE twin over well-formed and
// malformed offsets, with and without a C index that has out-of-range entries, and compares every row with the dense twin
// (gemm_native_invariant_host.h) on that row alone -- an image of one row, copied out here by the layout notes of gemm_native32.hpp, not by
// the header's own helper; rows of no expert and rows whose index is out of range must keep their poison.  Then the refusals, the form rule
// and the workspace arithmetic.  Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gemm_native_invariant_moe_host.h"

using namespace petit_amd;
using namespace petit_amd::invariant;
namespace ninv = petit_amd::native_invariant;

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// the image of grouped row `row` alone (m = 1): per k-tile the row's data bytes, MXFP6's second image, and its four scale bytes
static std::vector<uint8_t> row_image(const std::vector<uint8_t> &qa, unsigned m, unsigned k, int fmt, unsigned row) {
    const unsigned row_b = fmt == 8 ? 128u : 64u, per_row = k / 8 * (unsigned)fmt;
    std::vector<uint8_t> out((size_t)ninv::qact_bytes(1, k, fmt), 0u);
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

static void run_pair(int a_type, int fmt, unsigned E, unsigned m, unsigned n, unsigned k, unsigned seed) {
    const bool bf16 = a_type == kTypeBf16;
    std::mt19937 rng(seed);
    const size_t w_words = (size_t)n * k / 8, s_bytes = (size_t)n * k / kMxGroup;
    std::vector<uint32_t> pw(E * w_words);
    std::vector<uint8_t> ps(E * s_bytes);
    for (auto &x : pw)
        x = rng();
    for (auto &x : ps)
        x = (uint8_t)(124 + rng() % 7);
    std::vector<uint8_t> qa((size_t)ninv::qact_bytes(m, k, fmt));
    const size_t scale_at = (size_t)m * (k / 8 * (unsigned)fmt);
    for (size_t i = 0; i < qa.size(); ++i) // any element code (e4m3: not the two NaN codes); scale bytes around 2^0
        qa[i] = i < scale_at ? (uint8_t)((rng() & 0xffu) % 0x7fu | (rng() & 0x80u)) : (uint8_t)(122 + rng() % 9);
    std::vector<float> gs(E);
    std::vector<uint16_t> bias((size_t)E * n);
    for (auto &g : gs)
        g = 0.5f + (float)(rng() % 64) / 128.f;
    for (auto &b : bias)
        b = (uint16_t)f32_h16(bf16, (float)((int)(rng() % 33) - 16) * 0.25f);

    const unsigned c_rows = m + 2;
    std::vector<int32_t> c_idx(m);
    for (unsigned r = 0; r < m; ++r)
        c_idx[r] = (int32_t)((r * 7 + 3) % c_rows);
    if (m > 3)
        c_idx[1] = (int32_t)c_rows, c_idx[3] = -2; // outside [0, c_rows): stores nothing
    std::vector<std::vector<int32_t>> routings;
    auto frac = [&](std::initializer_list<double> f) {
        std::vector<int32_t> off(E + 1, (int32_t)m);
        unsigned i = 0;
        for (double x : f)
            if (i <= E)
                off[i++] = (int32_t)(x * m);
        routings.push_back(off);
    };
    frac({0, 0.3, 0.3, 0.7, 1});       // well formed, an empty expert
    frac({0, 0, 0.5, 0.5, 0.5});       // an empty first expert; the last ones take the rest
    frac({0.1, 0.3, 0.5, 0.5, 0.9});   // rows before the first expert (and after the last when E == 4)
    frac({0, 0.6, 0.2, 0.8, 1});       // descending
    frac({-0.2, 0.4, -0.1, 3.0, 0.5}); // negative, beyond m
    for (const auto &off : routings)
        for (int with_idx = 0; with_idx < 2; ++with_idx)
            for (int with_bias = 0; with_bias < 2; ++with_bias) {
                const unsigned rows_out = with_idx ? c_rows : m;
                std::vector<uint16_t> c((size_t)rows_out * n, 0x7fc1u), want((size_t)rows_out * n, 0x7fc1u), c1(n);
                EXPECT(ninv::moe_gemm_host(c.data(), qa.data(), pw.data(), ps.data(), gs.data(), with_bias ? bias.data() : nullptr, off.data(), E, m, n,
                                           k, with_idx ? c_idx.data() : nullptr, rows_out, a_type, fmt) == kRcOk);
                // the clamp rule, stated again: each offset clamped into [its predecessor, m], a running maximum
                auto clamp = [&](int32_t v, unsigned lo) {
                    const unsigned u = v < 0 ? 0u : (unsigned)v;
                    return u < lo ? lo : (u > m ? m : u);
                };
                unsigned lo = clamp(off[0], 0);
                for (unsigned e = 0; e < E; ++e) {
                    const unsigned hi = clamp(off[e + 1], lo);
                    for (unsigned r = lo; r < hi; ++r) {
                        const std::vector<uint8_t> img = row_image(qa, m, k, fmt, r);
                        EXPECT(ninv::gemm_host(c1.data(), img.data(), pw.data() + e * w_words, ps.data() + e * s_bytes, &gs[e],
                                               with_bias ? bias.data() + (size_t)e * n : nullptr, 1, n, k, a_type, fmt) == kRcOk);
                        const unsigned dst = with_idx ? (unsigned)c_idx[r] : r;
                        if (dst < rows_out)
                            for (unsigned col = 0; col < n; ++col)
                                want[(size_t)dst * n + col] = c1[col];
                    }
                    lo = hi;
                }
                EXPECT(c == want); // rows of an expert: the dense twin's bits; every other row: the poison
            }
}

int main() {
    for (int a_type : {kTypeBf16, kTypeFp16})
        for (int fmt : {8, 6, 4}) {
            run_pair(a_type, fmt, 4, 10, 32, 256, 1);
            run_pair(a_type, fmt, 3, 7, 64, 768, 2);   // three slices
            run_pair(a_type, fmt, 5, 6, 32, 4352, 3);  // L = 512, a last slice half as long
            run_pair(a_type, fmt, 70, 9, 32, 256, 4);  // more experts than one 64-expert chunk, most of them empty
        }
    // the form rule: split iff ceil(m / min(E, m)) <= kMoeSplitMaxRowsPer and m <= kMoeSplitMaxM
    for (unsigned E : {1u, 3u, 8u, 65u, 130u, 1024u})
        for (unsigned m = 1; m < 300; ++m) {
            const unsigned active = E < m ? E : m;
            EXPECT(ninv::moe_split(m, E) == ((m + active - 1) / active <= ninv::kMoeSplitMaxRowsPer && m <= ninv::kMoeSplitMaxM));
        }
    EXPECT(ninv::moe_split(0, 8));
    // workspace arithmetic
    const unsigned shapes[][2] = {{64, 1024}, {64, 4352}, {128, 256}, {96, 512}, {6144, 3072}, {3072, 3072}};
    for (const auto &s : shapes) {
        unsigned S = 0, L = 0;
        geometry(s[0], s[1], kTypeBf16, kTypeMx, &S, &L);
        for (unsigned E : {3u, 128u})
            for (unsigned m : {1u, 8u, 9u, 64u, 4096u, 70000u})
                for (int fmt : {8, 6, 4}) {
                    const bool split = ninv::moe_split(m, E);
                    const uint64_t slab = split ? ((uint64_t)S * m * s[0] * 4 + 255) / 256 * 256 : 0;
                    const uint64_t q = ((uint64_t)m * (s[1] / 8 * (unsigned)fmt) + (uint64_t)m * (s[1] / 32) + 255) / 256 * 256;
                    EXPECT(ninv::moe_workspace_bytes(E, m, s[0], s[1], kTypeFp16, fmt, 1) == slab);
                    EXPECT(ninv::moe_workspace_bytes(E, m, s[0], s[1], kTypeBf16, fmt, 0) == q + slab);
                }
    }
    EXPECT(ninv::moe_workspace_bytes(3, 4, 48, 256, kTypeBf16, 8, 0) == 0 && ninv::moe_workspace_bytes(3, 0, 32, 256, kTypeBf16, 8, 0) == 0);
    EXPECT(ninv::moe_workspace_bytes(0, 4, 32, 256, kTypeBf16, 8, 0) == 0 && ninv::moe_workspace_bytes(1025, 4, 32, 256, kTypeBf16, 8, 0) == 0);
    // refusals
    alignas(256) static char buf[512];
    const int32_t *idx = (const int32_t *)buf;
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcOk);
    EXPECT(ninv::moe_shape_rc(3, 70000, 32, 256, nullptr, 70000, nullptr, 70000, kTypeFp16, 6, 0, 0) == kRcOk); // no 65535-row limit
    EXPECT(ninv::moe_shape_rc(3, 4, 48, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 128, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(ninv::moe_shape_rc(3, kMaxRows, 32, 256, idx, 4, idx, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(ninv::moe_shape_rc(3, 4, 96, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 1) == kRcProblemShape);
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, 3, 8, 0, 0) == kRcBadArgument);
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 5, 0, 0) == kRcBadArgument);
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 3) == kRcBadArgument);
    EXPECT(ninv::moe_shape_rc(0, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(ninv::moe_shape_rc(1025, 4, 32, 256, nullptr, 4, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, nullptr, 3, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcProblemShape);  // a NULL A index, 3 rows
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, idx, 3, nullptr, 4, kTypeBf16, 8, 0, 0) == kRcOk);
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, nullptr, 4, nullptr, 3, kTypeBf16, 8, 0, 0) == kRcProblemShape);  // a NULL C index, 3 rows
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, nullptr, 0, nullptr, 4, kTypeBf16, 8, 1, 0) == kRcOk);            // quantised: a_rows is not read
    EXPECT(ninv::moe_shape_rc(3, 4, 32, 256, idx, 4, nullptr, 4, kTypeBf16, 8, 1, 0) == kRcBadArgument);       // quantised with an A index
    EXPECT(ninv::moe_shape_rc(3, 1u << 19, 32, 8192, nullptr, 0, idx, 4, kTypeBf16, 8, 1, 0) == kRcProblemShape);  // 2^32 quantised bytes
    EXPECT(ninv::moe_shape_rc(1024, kMaxRows - 1, 1u << 25, 256, nullptr, 0, idx, 4, kTypeBf16, 4, 1, 0) == kRcProblemShape); // 2^31 workgroups
    EXPECT(ninv::moe_grid(8, 64, 3, 4, true, 0) == (1 + 3) * 4 * 1 && ninv::moe_grid(200, 192, 3, 2, false, 1) == (4 + 3) * 1);
    void *ok = buf;
    EXPECT(ninv::moe_gemm_host(nullptr, ok, ok, ok, (const float *)ok, nullptr, idx, 3, 1, 32, 256, nullptr, 1, kTypeBf16, 8) == kRcProblemShape);
    EXPECT(ninv::moe_gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, 32, 256, nullptr, 0, kTypeBf16, 8) == kRcOk);
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
