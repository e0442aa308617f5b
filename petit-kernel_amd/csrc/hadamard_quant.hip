// hadamard_quant.hip -- the block-Hadamard rotation "petit-had/1" (include/petit_amd.h "Block-Hadamard rotation") in front of the native class's
// activation quantisers, and as a 16-bit stream for weights at load time.  The definition's butterfly is hadamard.h; on the device it runs in
// the quantisers' own thread map (qact_hadamard.inc), so a rotating quantiser is the unrotated one with that fragment in front of
// qact_column.inc: the same loads, the same stores, no LDS.  The fused norm's rotating forms are instantiations of rmsnorm_quant.hip.
// No counterpart in the reference, which has no activation quantiser.
//
// Compiled with floating-point contraction OFF, as rmsnorm_quant.hip: the sums and differences of the definition are one operation each.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/petit_amd.h"
#include "device_common.hpp"
#include "gemm_native32.hpp" // QuantGather and the quantisers' row / source helpers
#include "hadamard.h"
#include "numfmt.h"
#include "petit_internal.h"

#pragma clang fp contract(off)

namespace petit_amd {

// quantize_act32_kernel (gemm_native32.hpp) with the rotation in front of the column: its grid, its loads, its gathering form
template <bool BF16, int ACT, int HAD, class... Gather>
__global__ __launch_bounds__(256) void quantize_act32_rot_kernel(const void *a, unsigned char *ws, unsigned m, unsigned k, const Gather... gather) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned char *qa = ws;
    unsigned char *qs = ws + qact_elem_bytes(m, k, ACT);
    constexpr int kIlp = 4;
    const unsigned row = q_row(gather...), cols = k / 8, bx = q_bx(gather...);
    const unsigned src = q_src(row, gather...);
    const bool valid = q_valid(src, gather...);
    const u32x4 *const a_row = reinterpret_cast<const u32x4 *>(a) + (size_t)src * cols;
    u32x4 raws[kIlp];
#pragma unroll
    for (int j = 0; j < kIlp; ++j) {
        const unsigned c = (bx * kIlp + j) * 256 + threadIdx.x;
        raws[j] = (c < cols && valid) ? a_row[c] : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < kIlp; ++j) {
        const unsigned c8 = (bx * kIlp + j) * 256 + threadIdx.x; // 8-element column
        if (c8 >= cols) // (K / 8 is a multiple of 16: the 16 lanes of a k-tile leave together)
            break;
        float v[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned w = raws[j][d];
            v[2 * d] = h16_f32<BF16>(w & 0xffffu), v[2 * d + 1] = h16_f32<BF16>(w >> 16);
        }
#include "qact_hadamard.inc"
#include "qact_column.inc"
    }
#endif
}

// The rotation to 16 bit: a stream of 8-element columns over the whole [rows][k] matrix (k / 8 is a multiple of 32, so a block's lanes share
// a row and a wave), four columns per thread, every load requested before the first is used.  A lane writes only the column it has read, and
// a wave has read a block completely before it writes it: out may be in.
template <bool BF16, int HAD>
__global__ __launch_bounds__(256) void hadamard_rows_kernel(void *out, const void *in, size_t cols_total, float scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int kIlp = 4;
    const u32x4 *const src = reinterpret_cast<const u32x4 *>(in);
    u32x4 *const dst = reinterpret_cast<u32x4 *>(out);
    u32x4 raws[kIlp];
#pragma unroll
    for (int j = 0; j < kIlp; ++j) {
        const size_t c = ((size_t)blockIdx.x * kIlp + j) * 256 + threadIdx.x;
        raws[j] = c < cols_total ? src[c] : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < kIlp; ++j) {
        const size_t c = ((size_t)blockIdx.x * kIlp + j) * 256 + threadIdx.x;
        if (c >= cols_total) // (a multiple of 32: the 16 lanes of a block leave together)
            break;
        const unsigned c8 = threadIdx.x; // (the lane's place in its block: the column's low bits)
        float v[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned w = raws[j][d];
            v[2 * d] = h16_f32<BF16>(w & 0xffffu), v[2 * d + 1] = h16_f32<BF16>(w >> 16);
        }
#include "qact_hadamard.inc"
        u32x4 o;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            o[d] = (f32_h16<BF16>(v[2 * d] * scale) & 0xffffu) | (f32_h16<BF16>(v[2 * d + 1] * scale) << 16);
        dst[c] = o;
    }
#endif
}

namespace {

template <bool BF16, int ACT, int HAD>
int launch_quantize_rot(const void *a, const int *a_idx, unsigned a_rows, bool gather, void *qa, unsigned m, unsigned k, hipStream_t stream) {
    const unsigned xb = (k / 8 + 1023) / 1024;
    unsigned char *const ws = (unsigned char *)qa;
    if (gather) { // (petit_quantize_activations_rows' grid: xb workgroups per layout row, all along x)
        if ((uint64_t)xb * m >= (1ull << 31))
            return kErrProblemShape;
        hipLaunchKernelGGL((quantize_act32_rot_kernel<BF16, ACT, HAD, QuantGather>), dim3(xb * m), dim3(256), 0, stream, a, ws, m, k,
                           QuantGather{a_idx, a_rows, xb});
    } else {
        if (m > 65535)
            return kErrKernelShape; // (petit_quantize_activations': one grid row per activation row)
        hipLaunchKernelGGL((quantize_act32_rot_kernel<BF16, ACT, HAD>), dim3(xb, m), dim3(256), 0, stream, a, ws, m, k);
    }
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}
template <bool BF16, int ACT> int launch_quantize_rot(unsigned block, const void *a, const int *a_idx, unsigned a_rows, bool gather, void *qa,
                                                      unsigned m, unsigned k, hipStream_t stream) {
    return block == 32 ? launch_quantize_rot<BF16, ACT, 32>(a, a_idx, a_rows, gather, qa, m, k, stream)
                       : launch_quantize_rot<BF16, ACT, 128>(a, a_idx, a_rows, gather, qa, m, k, stream);
}
// format 8 / 4, block 32 / 128, a_type bf16 / fp16: checked by the callers
int launch_quantize_rot(int a_type, int format, unsigned block, const void *a, const int *a_idx, unsigned a_rows, bool gather, void *qa, unsigned m,
                        unsigned k, hipStream_t stream) {
    if (a_type == kDataTypeBf16)
        return format == 8 ? launch_quantize_rot<true, 8>(block, a, a_idx, a_rows, gather, qa, m, k, stream)
                           : launch_quantize_rot<true, 4>(block, a, a_idx, a_rows, gather, qa, m, k, stream);
    return format == 8 ? launch_quantize_rot<false, 8>(block, a, a_idx, a_rows, gather, qa, m, k, stream)
                       : launch_quantize_rot<false, 4>(block, a, a_idx, a_rows, gather, qa, m, k, stream);
}

// what petit_hadamard_rows and its twin refuse; kOk with *run = false: nothing to do
int hadamard_rows_check(const void *out, const void *in, unsigned rows, unsigned k, int a_type, unsigned block, int log2_scale, bool *run) {
    *run = false;
    if (block != 32 && block != 128)
        return kErrBadArgument;
    if (log2_scale > 126 || log2_scale < -126)
        return kErrBadArgument;
    if (rows == 0 || k == 0)
        return kOk;
    if (!out || !in || (((uintptr_t)out | (uintptr_t)in) & 15))
        return kErrBadArgument;
    if (k % 256 != 0)
        return kErrProblemShape;
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrKernelShape;
    *run = true;
    return kOk;
}
float pow2_f32(int e) { return bits_f32((unsigned)(127 + e) << 23); } // |e| <= 126: a normal number

template <bool BF16> void hadamard_rows_host_t(uint16_t *out, const uint16_t *in, unsigned rows, unsigned k, unsigned block, float scale) {
    std::vector<float> z(k);
    for (unsigned r = 0; r < rows; ++r) {
        const uint16_t *const x = in + (size_t)r * k;
        uint16_t *const o = out + (size_t)r * k;
        for (unsigned i = 0; i < k; ++i)
            z[i] = h16_f32<BF16>(x[i]);
        hadamard_row_host(z.data(), k, block);
        for (unsigned i = 0; i < k; ++i)
            o[i] = (uint16_t)f32_h16<BF16>(z[i] * scale);
    }
}

} // namespace
} // namespace petit_amd

using namespace petit_amd;

extern "C" {

int petit_hadamard_rows(void *out, const void *in, unsigned rows, unsigned k, int a_type, unsigned block, int log2_scale, void *stream) {
    bool run;
    if (const int rc = hadamard_rows_check(out, in, rows, k, a_type, block, log2_scale, &run); rc != kOk || !run)
        return rc;
    const size_t cols_total = (size_t)rows * (k / 8);
    const size_t blocks = (cols_total + 1023) / 1024;
    if (blocks >= (1ull << 31))
        return kErrProblemShape;
    const bool bf16 = a_type == kDataTypeBf16;
    const auto kern = block == 32 ? (bf16 ? hadamard_rows_kernel<true, 32> : hadamard_rows_kernel<false, 32>)
                                  : (bf16 ? hadamard_rows_kernel<true, 128> : hadamard_rows_kernel<false, 128>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, out, in, cols_total, pow2_f32(log2_scale));
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int petit_hadamard_rows_host(void *out, const void *in, unsigned rows, unsigned k, int a_type, unsigned block, int log2_scale) {
    bool run;
    if (const int rc = hadamard_rows_check(out, in, rows, k, a_type, block, log2_scale, &run); rc != kOk || !run)
        return rc;
    if (a_type == kDataTypeBf16)
        hadamard_rows_host_t<true>((uint16_t *)out, (const uint16_t *)in, rows, k, block, pow2_f32(log2_scale));
    else
        hadamard_rows_host_t<false>((uint16_t *)out, (const uint16_t *)in, rows, k, block, pow2_f32(log2_scale));
    return kOk;
}

int petit_quantize_activations_rot(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format, unsigned block, void *stream) {
    if (!hadamard_block_ok(block))
        return kErrBadArgument;
    if (block == 0)
        return petit_quantize_activations(qa, a, m, k, a_type, format, stream);
    if (m == 0 || k == 0)
        return kOk;
    if (!qa || !a || ((uintptr_t)qa & 15) || ((uintptr_t)a & 15))
        return kErrBadArgument;
    if (k % 256 != 0)
        return kErrProblemShape;
    if ((a_type != kDataTypeBf16 && a_type != kDataTypeFp16) || (format != 8 && format != 4))
        return kErrKernelShape; // (MXFP6 included: its converts read 16-bit patterns)
    return launch_quantize_rot(a_type, format, block, a, nullptr, 0, false, qa, m, k, (hipStream_t)stream);
}

int petit_quantize_activations_rot_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format, unsigned block) {
    return quantize_activations_rot_host(qa, a, m, k, a_type, format, block);
}

int petit_quantize_activations_rows_rot(void *qa, const void *a, const int32_t *a_row_index, unsigned a_rows, unsigned m, unsigned k, int a_type,
                                        int format, unsigned block, void *stream) {
    if (!hadamard_block_ok(block))
        return kErrBadArgument;
    if (block == 0)
        return petit_quantize_activations_rows(qa, a, a_row_index, a_rows, m, k, a_type, format, stream);
    if (m == 0 || k == 0)
        return kOk;
    if (!qa || !a || ((uintptr_t)qa & 15) || ((uintptr_t)a & 15))
        return kErrBadArgument;
    if (k % 256 != 0 || (!a_row_index && a_rows < m) || petit_quantized_activation_bytes(m, k, format) >= (1ull << 32))
        return kErrProblemShape;
    if ((a_type != kDataTypeBf16 && a_type != kDataTypeFp16) || (format != 8 && format != 4))
        return kErrKernelShape;
    return launch_quantize_rot(a_type, format, block, a, a_row_index, a_rows, true, qa, m, k, (hipStream_t)stream);
}

int petit_rmsnorm_quantize_rot(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                               float weight_offset, unsigned m, unsigned k, int a_type, int format, unsigned block, void *stream) {
    return rmsnorm_quantize_rot(qa, y16, residual_out, x, residual, weight, eps, weight_offset, m, k, a_type, format, block, (hipStream_t)stream);
}
int petit_rmsnorm_quantize_rot_host(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                                    float weight_offset, unsigned m, unsigned k, int a_type, int format, unsigned block) {
    return rmsnorm_quantize_rot_host(qa, y16, residual_out, x, residual, weight, eps, weight_offset, m, k, a_type, format, block);
}

} // extern "C"
