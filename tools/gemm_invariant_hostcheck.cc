// tools/gemm_invariant_hostcheck.cc -- a stand-alone program around the host side of the batch-invariant GEMM
// (petit-kernel_amd/csrc/gemm_invariant_host.h: geometry, workspace arithmetic, argument checks, the CPU twin), for sanitizer runs on the CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipetit-kernel_amd/csrc \
//         tools/gemm_invariant_hostcheck.cc -o gemm_invariant_hostcheck && ./gemm_invariant_hostcheck
//
// It packs small exact problems of every accepted (type, format) pair into buffers of exactly the bytes the layout declares (so that an
// index outside them is a heap overflow the sanitizer sees), runs the twin with and without global scale and bias, for a batch and for each
// row alone, compares with a double-precision reference, and walks every refusal.  Exit status 0 and "ok" when everything holds.
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

static void run_pair(int a_type, int b_type, unsigned m, unsigned n, unsigned k, unsigned seed) {
    const bool mx = is_mx(b_type), bf16 = a_type == kTypeBf16;
    const unsigned group = mx ? kMxGroup : kNvGroup;
    std::mt19937 rng(seed);
    std::vector<uint32_t> pw((size_t)n * k / 8, 0u);
    std::vector<uint8_t> ps((size_t)n * k / group, 0u);
    std::vector<double> w((size_t)n * k);
    static const uint8_t nv_bytes[3] = {0x38, 0x40, 0x48}; // e4m3 1, 2, 4
    for (unsigned row = 0; row < n; ++row)
        for (unsigned g = 0; g < k / group; ++g) {
            const unsigned pick = rng() % 3;
            const size_t at = mx ? packed_mxscale_byte_index(k, row, g) : packed_nvscale_byte_index(k, row, g);
            ps.at(at) = mx ? (uint8_t)(127 + pick) : nv_bytes[pick];
            for (unsigned i = 0; i < group; ++i) {
                const unsigned kk = g * group + i, code = rng() & 15u;
                pw.at(packed_weight_word_index(k, row, kk / 8)) |= code << (4 * (kk % 8));
                w[(size_t)row * k + kk] = (double)e2m1_f32(code) * (double)(1u << pick);
            }
        }
    std::vector<uint16_t> a((size_t)m * k), bias(n), c((size_t)m * n, 0x7fc1u), c1(n);
    std::vector<double> a64((size_t)m * k), b64(n);
    for (size_t i = 0; i < a.size(); ++i) {
        const int v = (rng() & 1u) ? (int)(rng() % 7) - 3 : 0;
        a[i] = (uint16_t)f32_h16(bf16, (float)v), a64[i] = v;
    }
    for (unsigned i = 0; i < n; ++i) {
        const int v = (int)(rng() % 17) - 8;
        bias[i] = (uint16_t)f32_h16(bf16, (float)v), b64[i] = v;
    }
    for (int with_gs = 0; with_gs < 2; ++with_gs)
        for (int with_bias = 0; with_bias < 2; ++with_bias) {
            const float gs = 0.25f;
            EXPECT(gemm_host(c.data(), a.data(), pw.data(), ps.data(), with_gs ? &gs : nullptr, with_bias ? bias.data() : nullptr, m, n, k, a_type,
                             b_type) == kRcOk);
            for (unsigned row = 0; row < m; ++row) {
                EXPECT(gemm_host(c1.data(), a.data() + (size_t)row * k, pw.data(), ps.data(), with_gs ? &gs : nullptr,
                                 with_bias ? bias.data() : nullptr, 1, n, k, a_type, b_type) == kRcOk);
                for (unsigned col = 0; col < n; ++col) {
                    double y = 0;
                    for (unsigned kk = 0; kk < k; ++kk)
                        y += a64[(size_t)row * k + kk] * w[(size_t)col * k + kk];
                    y = y * (with_gs ? 0.25 : 1.0) + (with_bias ? b64[col] : 0.0);
                    EXPECT(c[(size_t)row * n + col] == (uint16_t)f32_h16(bf16, (float)y)); // exact inputs: one rounding is left
                    EXPECT(c1[col] == c[(size_t)row * n + col]);                           // the row alone: the same bits
                }
            }
        }
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

int main() {
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
            EXPECT(slabs(m, s[0], s[1], kTypeBf16, kTypeNv) == (m <= kSplitMaxM ? S : 1u));
            const uint64_t want = m <= kSplitMaxM ? ((uint64_t)S * m * s[0] * 4 + 255) / 256 * 256 : 0;
            EXPECT(workspace_bytes(m, s[0], s[1], kTypeBf16, kTypeNv) == want);
        }
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
    EXPECT(workspace_bytes(4, 32, 256, kTypeFp16, kTypeMx) == 0 && workspace_bytes(4, 24, 256, kTypeBf16, kTypeNv) == 0);
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
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
