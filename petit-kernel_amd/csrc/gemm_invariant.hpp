// gemm_invariant.hpp -- the batch-invariant dense GEMM (include/petit_amd.h "Batch-invariant GEMM"): every output element is a pure function of
// its activation row, the weights, the scales and the bias -- never of M, of the row's position, or of the launch form.
//
// K is cut into S slices of L (geometry, gemm_invariant_host.h: a function of (n, k, a_type, b_type) alone).  The partial sum p_s of a
// slice is ONE chain of v_mfma_f32_16x16x32_{bf16,f16} from a zero accumulator: k-tiles of 128 ascending, the four words of a packed tile in
// their own order (layout.h), the weight operand dequantised exactly to the activation type with its group scale applied BEFORE the MFMA.  The
// result is ((p_0 + p_1) + ... + p_{S-1}) * gs + bias in fp32, rounded once.  Two forms produce those bits:
//   split (m <= the form switch): grid = n-tiles / 4 x S x m-tiles.  A wave owns one 16 x 16 tile of one slice and stores it to slab s of
//     [S][m][n] fp32 with plain vector stores -- no tickets, no fences, no atomics; invariant_fold_kernel adds the slabs in ascending order and
//     applies scale, bias and activation.  The weights go straight to VGPRs (non-temporal buffer_load_dwordx4 into a register ring kDepth
//     tiles deep); the main loop has no barrier and no LDS.
//   whole (above): grid = n-tiles / 8 x m-blocks of 64 rows.  The workgroup stages its 64 x 128 activation tile of every k-tile in LDS once
//     (double-buffered, one barrier per k-tile, as gemm_tiled.hpp does); a wave owns 4 m-tiles x 2 n-tiles (gated: the gate / up pair), walks
//     ALL the slices, accumulates each from zero and joins it to the running total with one plain fp32 add per accumulator -- the slab sum's
//     additions -- and applies the epilogue itself.  No wave-level K split: the fold is never reordered.
// An MFMA computes every output element from its own row and column alone, and rows past M read zeros through the buffer descriptor, so what
// sits next to a row in its tile cannot reach it.
//
// Each form's body is stated once, in gemm_invariant_split.inc and gemm_invariant_whole.inc.  The dense kernels below and the routed-expert
// kernels (gemm_invariant_moe.hpp) are a prologue each -- the activation descriptor and the per-lane byte offsets into it, the weight and scale
// bases, the tile's first row m0 and its rows_valid, the row of C an output row goes to -- and the include.
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "gemm_invariant_host.h"

namespace petit_amd {

struct InvariantArgs {
    void *c;         // [m][n] (gated: [m][n/2]) 16-bit
    const void *a;   // [m][k] 16-bit
    const void *w;   // packed weights
    const void *s;   // packed scales
    const float *gs; // device pointer to one float, or null: no multiply
    const void *bias; // [n] in c's type, or null: no add
    float *slabs;    // split form: [slices][m][n] fp32
    unsigned m, n, k;
    unsigned slice_k, slices; // L, S
    unsigned act;             // PETIT_ACTIVATION_*
};

// The plain epilogue of the definition: 4 consecutive n of one row; a multiply, then an add, each rounded (no fma), ONE rounding to 16 bit.
template <class AT> __device__ __forceinline__ uint2 invariant_finish4(const f32x4 v, const float *gs, const void *bias, const unsigned n) {
#pragma clang fp contract(off)
    float y[4] = {v[0], v[1], v[2], v[3]};
    if (gs) {
        const float g = *gs;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            y[i] = y[i] * g;
    }
    if (bias) {
        const uint2 raw = *reinterpret_cast<const uint2 *>((const char *)bias + (size_t)n * 2);
        const unsigned w0 = raw.x, w1 = raw.y; // named scalars: see the bit_cast note in device_common.hpp
        float b[4];
        if constexpr (AT::kType == kDataTypeBf16) {
            const unsigned b0 = w0 << 16, b1 = w0 & 0xffff0000u, b2 = w1 << 16, b3 = w1 & 0xffff0000u;
            b[0] = __builtin_bit_cast(float, b0), b[1] = __builtin_bit_cast(float, b1);
            b[2] = __builtin_bit_cast(float, b2), b[3] = __builtin_bit_cast(float, b3);
        } else {
            const f16x2 h0 = __builtin_bit_cast(f16x2, w0), h1 = __builtin_bit_cast(f16x2, w1);
            const _Float16 e0 = h0[0], e1 = h0[1], e2 = h1[0], e3 = h1[1];
            b[0] = (float)e0, b[1] = (float)e1, b[2] = (float)e2, b[3] = (float)e3;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            y[i] = y[i] + b[i];
    }
    uint2 o;
    o.x = pack2(AT{}, y[0], y[1]);
    o.y = pack2(AT{}, y[2], y[3]);
    return o;
}

// The split form.  AT: Bf16 / Fp16.  FMT: kFmtNv / kFmtMx.  kDepth: k-tiles in flight per wave.
template <class AT, int FMT, int kDepth>
__global__ __launch_bounds__(256) void gemm_invariant_split_kernel(const InvariantArgs p) {
#pragma clang fp contract(off)
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned tile = blockIdx.x * 4u + wave; // a wave's slot is its n-tile
    const bool live = tile < p.n / kTileN;
    const unsigned m0 = blockIdx.z * 16u, s = blockIdx.y;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 16u ? rows_left : 16u; // (the grid keeps m0 < m)
    // the activations [rows_valid][k] from row m0 on: rows past M are out of range -> zeros
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc((const char *)p.a + (size_t)m0 * p.k * 2, rows_valid * p.k * 2);
    const unsigned a_voff = (lane & 15u) * p.k * 2 + (lane >> 4) * (kLaneK * 2);
    const char *const w_base = (const char *)p.w, *const s_base = (const char *)p.s;
#include "gemm_invariant_split.inc"
}

// The whole form.  A workgroup owns 64 rows x 8 n-tiles (4 waves x 2): wave w takes the tile pair of slot 4 blockIdx.x + w -- tiles 2 t and 2 t + 1,
// or (gated) gate tile t and up tile t + ntiles / 2 -- against all four m-tiles.  Per k-tile the 256 threads fetch the 64 x 128 activation tile
// once (4 buffer_load_dwordx4 each, one k-tile ahead, rows past M read zeros through the descriptor) and drop it into the other half of a
// double-buffered LDS image (rows padded by 16 B: the fragment reads of 16 rows are conflict-free); one barrier per k-tile.  The weights stream
// into a register ring kWholeRing k-tiles deep.  Every accumulator keeps ONE chain per slice; at a slice boundary it joins the running total.
constexpr int kWholeRing = 3, kWholeRowBytes = kTileK * 2 + 16, kWholeBufBytes = 64 * kWholeRowBytes;
template <class AT, int FMT> __global__ __launch_bounds__(256) void gemm_invariant_whole_kernel(const InvariantArgs p) {
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned slot = blockIdx.x * 4u + wave;
    const unsigned m0 = blockIdx.y * 64u;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 64u ? rows_left : 64u; // (the grid keeps m0 < m)
    // the activations [rows_valid][k] from row m0 on: rows past M are out of range -> zeros
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc((const char *)p.a + (size_t)m0 * p.k * 2, rows_valid * p.k * 2);
    auto a_row_off = [&](unsigned row) { return row * p.k * 2; };
    const char *const w_base = (const char *)p.w, *const s_base = (const char *)p.s;
    const float *const gs = p.gs;
    const void *const bias = p.bias;
    auto c_row = [](unsigned row) { return row; };
#include "gemm_invariant_whole.inc"
}

// The split form's second launch: one thread per 4 consecutive output columns of one row adds the slabs in ascending order -- the definition's
// additions -- and applies scale, bias and activation with the single rounding.
template <class AT> __global__ __launch_bounds__(256) void invariant_fold_kernel(const InvariantArgs p) {
#pragma clang fp contract(off)
    const unsigned n_out = p.act ? p.n / 2 : p.n, per_row = n_out / 4;
    const size_t count = (size_t)p.m * per_row, slab = (size_t)p.m * p.n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const unsigned row = (unsigned)(i / per_row), n = (unsigned)(i % per_row) * 4u;
        auto fold = [&](unsigned col) {
            const float *src = p.slabs + (size_t)row * p.n + col;
            f32x4 v = *reinterpret_cast<const f32x4 *>(src);
            for (unsigned s = 1; s < p.slices; ++s)
                v = v + *reinterpret_cast<const f32x4 *>(src + s * slab);
            return v;
        };
        uint2 o;
        if (p.act) {
            const float g = p.gs ? *p.gs : 1.0f;
            o = finish4_silu_mul<AT>(fold(n), fold(n + n_out), g, p.bias, n, n_out, p.act);
        } else {
            o = invariant_finish4<AT>(fold(n), p.gs, p.bias, n);
        }
        *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * n_out + n) * 2) = o;
    }
}

constexpr int kInvariantSplitDepth = 4;

// the grid of one launch of the plan (gemm_invariant_host.h), which is where every grid of the family is computed
inline dim3 invariant_grid(const invariant::Launch &l) { return dim3((unsigned)l.grid_x, l.grid_y, l.grid_z); }

// one (format, type) pair's launches; instantiated by gemm_invariant_*.hip
template <class AT, int FMT> void invariant_launch(const InvariantArgs &p, const invariant::Plan &plan, hipStream_t stream) {
    if (plan.split) {
        hipLaunchKernelGGL((gemm_invariant_split_kernel<AT, FMT, kInvariantSplitDepth>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        hipLaunchKernelGGL((invariant_fold_kernel<AT>), invariant_grid(plan.fold), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL((gemm_invariant_whole_kernel<AT, FMT>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
    }
}

} // namespace petit_amd
