// tools/native_invariant_hostcheck.cc -- a stand-alone program around the host side of the batch-invariant GEMM on the native class
// (petit-kernel_amd/csrc/gemm_native_invariant_host.h: workspace arithmetic, argument checks, the decode of "petit-qact/1" bytes, the CPU
// twin), for sanitizer runs on the CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipetit-kernel_amd/csrc \
//         tools/native_invariant_hostcheck.cc -o native_invariant_hostcheck && ./native_invariant_hostcheck
//
// It writes small exact problems of every (type, activation format) pair into buffers of exactly the bytes the layouts declare (so that an
// index outside them is a heap overflow the sanitizer sees) -- the quantised image element by element, with an encoder of its own that
// mirrors the layout notes of gemm_native32.hpp --, reads every element back through the header's decode, runs the twin with and without
// global scale and bias, for a batch and for each row alone, compares with a double-precision reference, and walks the refusals and the
// workspace arithmetic.  Exit status 0 and "ok" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "gemm_native_invariant_host.h"

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

// writes element (row, kk) of the image: the inverse of ninv::qact_element, stated from the layout notes
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

static void run_pair(int a_type, int fmt, unsigned m, unsigned n, unsigned k, unsigned seed) {
    const bool bf16 = a_type == kTypeBf16;
    std::mt19937 rng(seed);
    std::vector<uint32_t> pw((size_t)n * k / 8, 0u);
    std::vector<uint8_t> ps((size_t)n * k / kMxGroup, 0u);
    std::vector<double> w((size_t)n * k);
    for (unsigned row = 0; row < n; ++row)
        for (unsigned g = 0; g < k / kMxGroup; ++g) {
            const unsigned pick = rng() % 3;
            ps.at(packed_mxscale_byte_index(k, row, g)) = (uint8_t)(126 + pick);
            for (unsigned i = 0; i < kMxGroup; ++i) {
                const unsigned kk = g * kMxGroup + i, code = rng() & 15u;
                pw.at(packed_weight_word_index(k, row, kk / 8)) |= code << (4 * (kk % 8));
                w[(size_t)row * k + kk] = (double)e2m1_f32(code) * std::ldexp(1.0, (int)pick - 1);
            }
        }
    static const int vals[11] = {0, 1, -1, 2, -2, 3, -3, 4, -4, 6, -6};
    std::vector<uint8_t> qa((size_t)ninv::qact_bytes(m, k, fmt), 0u);
    std::vector<double> a64((size_t)m * k);
    for (unsigned row = 0; row < m; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            const unsigned sbyte = 125 + rng() % 5;
            qa.at((size_t)m * (k / 8 * (unsigned)fmt) + ((size_t)(blk / 4) * m + row) * 4 + blk % 4) = (uint8_t)sbyte;
            EXPECT(ninv::qact_scale_byte(qa.data(), m, k, fmt, row, blk) == sbyte);
            for (unsigned i = 0; i < 32; ++i) {
                const unsigned kk = 32 * blk + i;
                const int v = (rng() & 1u) ? vals[rng() % 11] : 0;
                put_element(qa, m, k, fmt, row, kk, code_of(fmt, v));
                a64[(size_t)row * k + kk] = v * std::ldexp(1.0, (int)sbyte - 127);
            }
        }
    for (unsigned row = 0; row < m; ++row) // every element reads back through the header's decode
        for (unsigned kk = 0; kk < k; ++kk)
            EXPECT((double)ninv::qact_element(qa.data(), m, k, fmt, row, kk) * ninv::e8m0_f64(ninv::qact_scale_byte(qa.data(), m, k, fmt, row, kk / 32)) ==
                   a64[(size_t)row * k + kk]);
    std::vector<uint16_t> bias(n), c((size_t)m * n, 0x7fc1u), c1(n);
    std::vector<double> b64(n);
    for (unsigned i = 0; i < n; ++i) {
        const int v = (int)(rng() % 17) - 8;
        bias[i] = (uint16_t)f32_h16(bf16, (float)v), b64[i] = v;
    }
    // a row alone is an image of its own (m = 1): the same elements at other addresses
    std::vector<std::vector<uint8_t>> alone(m, std::vector<uint8_t>((size_t)ninv::qact_bytes(1, k, fmt), 0u));
    for (unsigned row = 0; row < m; ++row)
        for (unsigned blk = 0; blk < k / 32; ++blk) {
            alone[row].at((size_t)(k / 8 * (unsigned)fmt) + (size_t)(blk / 4) * 4 + blk % 4) = (uint8_t)ninv::qact_scale_byte(qa.data(), m, k, fmt, row, blk);
            for (unsigned i = 0; i < 32; ++i) {
                const unsigned kk = 32 * blk + i;
                const double scale = ninv::e8m0_f64(ninv::qact_scale_byte(qa.data(), m, k, fmt, row, blk));
                put_element(alone[row], 1, k, fmt, 0, kk, code_of(fmt, (int)std::lround(a64[(size_t)row * k + kk] / scale)));
            }
        }
    for (int with_gs = 0; with_gs < 2; ++with_gs)
        for (int with_bias = 0; with_bias < 2; ++with_bias) {
            const float gs = 0.25f;
            EXPECT(ninv::gemm_host(c.data(), qa.data(), pw.data(), ps.data(), with_gs ? &gs : nullptr, with_bias ? bias.data() : nullptr, m, n, k,
                                   a_type, fmt) == kRcOk);
            for (unsigned row = 0; row < m; ++row) {
                EXPECT(ninv::gemm_host(c1.data(), alone[row].data(), pw.data(), ps.data(), with_gs ? &gs : nullptr,
                                       with_bias ? bias.data() : nullptr, 1, n, k, a_type, fmt) == kRcOk);
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

int main() {
    for (int a_type : {kTypeBf16, kTypeFp16})
        for (int fmt : {8, 6, 4}) {
            run_pair(a_type, fmt, 3, 32, 256, 1);
            run_pair(a_type, fmt, 2, 64, 768, 2);  // three slices
            run_pair(a_type, fmt, 1, 32, 4352, 3); // L = 512, a last slice half as long
        }
    // element tables
    EXPECT(ninv::e2m3_elem(0) == 0.f && ninv::e2m3_elem(1) == 0.125f && ninv::e2m3_elem(7) == 0.875f && ninv::e2m3_elem(8) == 1.f);
    EXPECT(ninv::e2m3_elem(15) == 1.875f && ninv::e2m3_elem(16) == 2.f && ninv::e2m3_elem(31) == 7.5f && ninv::e2m3_elem(63) == -7.5f);
    EXPECT(ninv::e4m3_elem(0x38) == 1.f && ninv::e4m3_elem(0x7e) == 448.f && ninv::e4m3_elem(0x01) == 0x1p-9f && std::isnan(ninv::e4m3_elem(0x7f)));
    EXPECT(ninv::e8m0_f64(0) == 0x1p-127 && ninv::e8m0_f64(127) == 1.0 && ninv::e8m0_f64(254) == 0x1p127);
    // workspace arithmetic
    const unsigned shapes[][2] = {{64, 1024}, {4096, 2304}, {128, 256}, {8192, 8192}, {57344, 8192}, {8192, 28672}};
    for (const auto &s : shapes) {
        unsigned S = 0, L = 0;
        geometry(s[0], s[1], kTypeBf16, kTypeMx, &S, &L);
        for (unsigned m : {1u, 17u, ninv::kSplitMaxM, ninv::kSplitMaxM + 1, 4096u, 65535u})
            for (int fmt : {8, 6, 4}) {
                const bool split = m <= ninv::kSplitMaxM;
                EXPECT(ninv::slabs(m, s[0], s[1], kTypeFp16) == (split ? S : 1u));
                const uint64_t slab = split ? ((uint64_t)S * m * s[0] * 4 + 255) / 256 * 256 : 0;
                const uint64_t q = ((uint64_t)m * (s[1] / 8 * (unsigned)fmt) + (uint64_t)m * (s[1] / 32) + 255) / 256 * 256;
                EXPECT(ninv::workspace_bytes(m, s[0], s[1], kTypeBf16, fmt, 1) == slab);
                EXPECT(ninv::workspace_bytes(m, s[0], s[1], kTypeBf16, fmt, 0) == q + slab);
            }
    }
    // refusals
    EXPECT(ninv::shape_rc(4, 32, 256, kTypeBf16, 8, 0, 0) == kRcOk && ninv::shape_rc(0, 64, 256, kTypeFp16, 4, 1, 2) == kRcOk);
    EXPECT(ninv::shape_rc(4, 48, 256, kTypeBf16, 8, 0, 0) == kRcProblemShape && ninv::shape_rc(4, 32, 128, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(ninv::shape_rc(4, 0, 256, kTypeBf16, 8, 0, 0) == kRcProblemShape && ninv::shape_rc(4, 32, 0, kTypeBf16, 8, 0, 0) == kRcProblemShape);
    EXPECT(ninv::shape_rc(kMaxRows, 32, 256, kTypeBf16, 8, 1, 0) == kRcProblemShape && ninv::shape_rc(4, 96, 256, kTypeBf16, 8, 0, 1) == kRcProblemShape);
    EXPECT(ninv::shape_rc(4, 32, 256, 3, 8, 0, 0) == kRcBadArgument && ninv::shape_rc(4, 32, 256, kTypeBf16, 5, 0, 0) == kRcBadArgument);
    EXPECT(ninv::shape_rc(4, 32, 256, kTypeBf16, 8, 0, 3) == kRcBadArgument && ninv::shape_rc(4, 32, 256, kTypeBf16, 8, 0, -1) == kRcBadArgument);
    EXPECT(ninv::shape_rc(65536, 32, 256, kTypeBf16, 8, 0, 0) == kRcKernelShape && ninv::shape_rc(65536, 32, 256, kTypeBf16, 8, 1, 0) == kRcOk);
    EXPECT(ninv::workspace_bytes(4, 48, 256, kTypeBf16, 8, 0) == 0 && ninv::workspace_bytes(0, 32, 256, kTypeBf16, 8, 0) == 0);
    alignas(256) static char buf[512];
    void *ok = buf;
    EXPECT(ninv::gemm_host(nullptr, ok, ok, ok, nullptr, nullptr, 1, 32, 256, kTypeBf16, 8) == kRcProblemShape);
    EXPECT(ninv::gemm_host(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 32, 256, kTypeBf16, 8) == kRcOk);
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
