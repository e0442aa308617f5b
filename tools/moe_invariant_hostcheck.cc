// tools/moe_invariant_hostcheck.cc -- a stand-alone program around the host side of the batch-invariant MoE launch
// (petit-kernel_amd/csrc/gemm_invariant_host.h: the form switch, grid and workspace arithmetic, argument checks, the CPU twin), for sanitizer
// runs on the CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipetit-kernel_amd/csrc \
//         tools/moe_invariant_hostcheck.cc -o moe_invariant_hostcheck && ./moe_invariant_hostcheck
//
// Every buffer has exactly the bytes the call declares (an index outside them is a heap overflow the sanitizer sees).  The twin runs under
// well-formed and malformed offsets, with gathers and scatters that go out of range, on poisoned outputs, and is compared row by row with the
// dense twin on the row's owner (the clamp rule, restated here); then the form switch, the workspace query and every refusal.
#include <algorithm>
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

static void run_pair(int a_type, int b_type, unsigned E, unsigned m, unsigned n, unsigned k, const std::vector<int32_t> &off, unsigned seed) {
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
        v = (uint16_t)f32_h16(bf16, (float)((int)(rng() % 9) - 4) * 0.25f);
    for (auto &v : bias)
        v = (uint16_t)f32_h16(bf16, (float)((int)(rng() % 17) - 8));
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
static void run_e8m0_byte0() {
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

int main() {
    const int pairs[3][2] = {{kTypeBf16, kTypeNv}, {kTypeBf16, kTypeMx}, {kTypeFp16, kTypeNv}};
    run_e8m0_byte0();
    for (const auto &p : pairs) {
        run_pair(p[0], p[1], 3, 9, 32, 256, {0, 4, 4, 9}, 1);          // well formed, an empty expert
        run_pair(p[0], p[1], 4, 11, 32, 768, {2, 7, 3, -5, 40}, 2);    // rows before offsets[0] unowned; descending, negative, beyond m
        run_pair(p[0], p[1], 2, 5, 32, 256, {-3, 2, 2}, 3);            // rows past the last offset unowned
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
            const uint64_t want = moe_split(m, E) ? ((uint64_t)S * m * 208 * 4 + 255) / 256 * 256 : 0;
            EXPECT(moe_workspace_bytes(E, m, 208, 768, kTypeBf16, kTypeNv) == want);
            EXPECT(moe_grid(m, 208, E, S, moe_split(m, E), 0) < (1ull << 31));
        }
    EXPECT(moe_workspace_bytes(0, 4, 32, 256, kTypeBf16, kTypeNv) == 0 && moe_workspace_bytes(1025, 4, 32, 256, kTypeBf16, kTypeNv) == 0);
    EXPECT(moe_workspace_bytes(4, 4, 32, 256, kTypeFp16, kTypeMx) == 0 && moe_workspace_bytes(4, 0, 32, 256, kTypeBf16, kTypeNv) == 0);
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
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
