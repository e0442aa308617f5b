// tools/native_image_readback_hostcheck.cc -- a stand-alone program around the host twins of petit-kernel_amd/csrc/native_image_readback.hip
// (petit_native_images_dequant_host, petit_mxfp6_export_images_host), for sanitizer runs on the CPU; no GPU is touched:
//
//     cd petit-kernel_amd/csrc && hipcc -std=c++20 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=all ../../tools/native_image_readback_hostcheck.cc native_image_readback.hip mxfp6_weights.hip hal.hip \
//         -o readback_hostcheck && ./readback_hostcheck
//
// Every buffer has exactly the bytes the contract declares (an index outside them is a heap overflow the sanitizer sees).  Over E in (1, 3),
// n in (32, 80), k in (256, 512, 1024): a random OCP MXFP6 tensor (every code, scale bytes 0 .. 255) is imaged by the ingest's twin; the export
// must return its bytes; the dequantiser must return, for f32, the value computed here in double precision, and for the 16-bit types and the
// global scales one rounding of it (bf16: restated here; fp16: through the compiler's _Float16).  Exit status 0 and "ok" when everything holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace petit_amd {
int mxfp6_native_images_host(void *images, const void *elems, const void *scales, unsigned num_experts, unsigned n, unsigned k);
int native_images_dequant_host(void *out, int out_type, const void *images, const float *global_scales, unsigned num_experts, unsigned n, unsigned k);
int mxfp6_export_images_host(void *elems, void *scales, const void *images, unsigned num_experts, unsigned n, unsigned k);
} // namespace petit_amd

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static uint32_t bits_of(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
static uint16_t bf16_rne(float x) {
    const uint32_t u = bits_of(x);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static uint16_t fp16_rne(float x) {
    const _Float16 h = (_Float16)x;
    uint16_t u;
    std::memcpy(&u, &h, 2);
    return u;
}

int main() {
    constexpr int kFp32 = 100, kBf16 = 5, kFp16 = 4;
    const float gs[3] = {0.75f, 3.0f, 1.0f / 3.0f};
    std::mt19937 rng(7);
    for (unsigned E : {1u, 3u})
        for (unsigned n : {32u, 80u})
            for (unsigned k : {256u, 512u, 1024u}) {
                const size_t rows = (size_t)E * n, image_bytes = (size_t)((n + 31) / 32) * (k / 128) * (3072 + 128);
                std::vector<unsigned char> elems(rows * (k / 4 * 3)), scales(rows * (k / 32)), images(E * image_bytes, 0xAA);
                for (auto &b : elems)
                    b = (unsigned char)rng();
                for (auto &b : scales)
                    b = (unsigned char)rng();
                EXPECT(petit_amd::mxfp6_native_images_host(images.data(), elems.data(), scales.data(), E, n, k) == 0);
                std::vector<unsigned char> elems2(elems.size(), 0x55), scales2(scales.size(), 0x55);
                EXPECT(petit_amd::mxfp6_export_images_host(elems2.data(), scales2.data(), images.data(), E, n, k) == 0);
                EXPECT(elems2 == elems && scales2 == scales);
                std::vector<float> f32(rows * k), f32s(rows * k);
                std::vector<uint16_t> b16(rows * k), h16(rows * k), b16s(rows * k), h16s(rows * k);
                EXPECT(petit_amd::native_images_dequant_host(f32.data(), kFp32, images.data(), nullptr, E, n, k) == 0);
                EXPECT(petit_amd::native_images_dequant_host(b16.data(), kBf16, images.data(), nullptr, E, n, k) == 0);
                EXPECT(petit_amd::native_images_dequant_host(h16.data(), kFp16, images.data(), nullptr, E, n, k) == 0);
                EXPECT(petit_amd::native_images_dequant_host(f32s.data(), kFp32, images.data(), gs, E, n, k) == 0);
                EXPECT(petit_amd::native_images_dequant_host(b16s.data(), kBf16, images.data(), gs, E, n, k) == 0);
                EXPECT(petit_amd::native_images_dequant_host(h16s.data(), kFp16, images.data(), gs, E, n, k) == 0);
                size_t bad = 0;
                for (size_t row = 0; row < rows; ++row)
                    for (unsigned i = 0; i < k; ++i) {
                        const unsigned char *const blk = elems.data() + (row * (k / 32) + i / 32) * 24;
                        const unsigned bit = 6 * (i % 32), sb = scales[row * (k / 32) + i / 32];
                        const unsigned code = ((blk[bit / 8] | (bit / 8 + 1 < 24 ? blk[bit / 8 + 1] << 8 : 0)) >> (bit % 8)) & 63u;
                        const unsigned e = (code >> 3) & 3u, m = code & 7u;
                        const double mag = std::ldexp(e ? (8.0 + m) * (1 << (e - 1)) : (double)m, (int)sb - 130);
                        const float v = sb == 255 ? std::nanf("") : (float)((code & 32u) ? -mag : mag), p = v * gs[row / n];
                        const size_t at = row * k + i;
                        if (sb == 255) { // E8M0's NaN: the quiet NaN, whatever the global scale
                            bad += bits_of(f32[at]) != 0x7fc00000u || b16[at] != 0x7fc0u || h16[at] != 0x7e00u || bits_of(f32s[at]) != 0x7fc00000u;
                            continue;
                        }
                        bad += bits_of(f32[at]) != bits_of(v) || b16[at] != bf16_rne(v) || h16[at] != fp16_rne(v);
                        bad += bits_of(f32s[at]) != bits_of(p) || b16s[at] != bf16_rne(p) || h16s[at] != fp16_rne(p);
                    }
                EXPECT(bad == 0);
            }
    EXPECT(petit_amd::native_images_dequant_host(&failures, 7, &failures, nullptr, 1, 32, 256) == 4);   // out_type, before the shape
    EXPECT(petit_amd::native_images_dequant_host(&failures, kBf16, &failures, nullptr, 1, 32, 384) == 1);
    EXPECT(petit_amd::mxfp6_export_images_host(&failures, &failures, &failures, 0, 32, 256) == 1);
    EXPECT(petit_amd::mxfp6_export_images_host(nullptr, &failures, &failures, 1, 32, 256) == 4);
    EXPECT(petit_amd::mxfp6_export_images_host(nullptr, nullptr, nullptr, 1, 0, 256) == 0);
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures != 0;
}
