// rmsnorm_quant.hip -- (residual add +) RMSNorm that writes the native class's quantised activations: one launch computes h = x (+ residual),
// y = RMSNorm(h) * (weight + offset) and the "petit-qact/1" bytes of y in MXFP8 / MXFP6 / MXFP4, with a bit-identical host twin.
// The contract (every rounding, the ONE summation order) is stated in include/petit_amd.h "RMSNorm into quantised activations"; this file is its
// evaluation.  No counterpart in the reference, which has no norm and no activation quantiser.
//
// A memory-bound row kernel: one 256-thread workgroup per row, thread t owns the 8-element columns t + 256 j, j < ILP, as one 16-byte load each
// (the thread map of quantize_act32_kernel, gemm_native32.hpp), so the row is read from memory ONCE, stays in registers through the reduction, and
// MXFP8 / MXFP4 quantise in the map the loads already have (a quad of lanes = one 32-k block).  MXFP6 needs 32 consecutive values per lane for the
// hardware's 32-element convert: the 16-bit y row goes through LDS once (<= 32 KiB) and is quantised as quantize_act32_fp6_kernel does.
// The quantise-and-store code is those two kernels' own: qact_column.inc and qact_block6.inc.
//
// moe_combine_rmsnorm_kernel (include/petit_amd.h "Top-k combine into the norm") is the same row with petit_moe_combine as its front end: h comes
// from the token's top-k slot rows instead of x.  Both kernels end in ONE device function, norm_quant_tail; its format 0 writes 16-bit outputs only.
//
// Host and device evaluate the same scalar helpers below; this file is compiled with floating-point contraction OFF (the pragma), so a product
// and a sum fuse only where the code says fma, on either side.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_common.hpp"
#include "hadamard.h"
#include "numfmt.h"
#include "petit_internal.h"

#pragma clang fp contract(off)

namespace petit_amd {

namespace {

// one rounding each, never fused with a neighbour (contraction is off in this file)
PETIT_HD float mul_rn(float a, float b) { return a * b; }
PETIT_HD float add_rn(float a, float b) { return a + b; }
PETIT_HD float fma_rn(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// the two elements of a dword (h16_f32 / f32_h16 of numfmt.h: bf16 by the integer rule on both sides; fp16 by the hardware convert on the device
// and the same rule spelled out on the host)
template <bool BF16> PETIT_HD void unpack2(unsigned w, float &lo, float &hi) {
    if constexpr (BF16) {
        lo = bits_f32(w << 16), hi = bits_f32(w & 0xffff0000u);
    } else {
        lo = h16_f32<false>(w & 0xffffu), hi = h16_f32<false>(w >> 16);
    }
}
template <bool BF16> PETIT_HD unsigned pack2(float lo, float hi) { return (f32_h16<BF16>(lo) & 0xffffu) | (f32_h16<BF16>(hi) << 16); }

// the sum of squares of one 8-element column: an ascending chain
PETIT_HD float column_sumsq(const float (&v)[8]) {
    float p = mul_rn(v[0], v[0]);
#pragma unroll
    for (int i = 1; i < 8; ++i)
        p = fma_rn(v[i], v[i], p);
    return p;
}
// steps 3 and 4 of the contract
PETIT_HD float inv_rms(float sumsq, float rk, float eps) {
#if defined(__HIP_DEVICE_COMPILE__)
    return 1.0f / __builtin_sqrtf(add_rn(mul_rn(sumsq, rk), eps)); // (correctly rounded: no fast-math in this library's build)
#else
    return 1.0f / std::sqrt(add_rn(mul_rn(sumsq, rk), eps));
#endif
}
PETIT_HD float normed(float h, float inv, float w, float woff) { return mul_rn(mul_rn(h, inv), add_rn(w, woff)); }

} // namespace

struct RmsQuantArgs {
    unsigned char *qa;
    void *y16, *res_out;      // nullable
    const void *x, *res, *w;  // res nullable
    float eps, woff, rk;      // rk = 1 / k, rounded once on the host
    unsigned m, k;
};

#if defined(__HIP_DEVICE_COMPILE__)
// h = round16(h + r), element by element (step 1 of the contract)
template <bool BF16, int ILP> __device__ __forceinline__ void add_residual(u32x4 (&h)[ILP], const u32x4 (&r)[ILP]) {
#pragma unroll
    for (int j = 0; j < ILP; ++j)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned xw = h[j][d], rw = r[j][d];
            float x0, x1, r0, r1;
            unpack2<BF16>(xw, x0, x1);
            unpack2<BF16>(rw, r0, r1);
            h[j][d] = pack2<BF16>(add_rn(x0, r0), add_rn(x1, r1));
        }
}

// Steps 2 - 5 of the contract on a row of h held as thread t's columns t + 256 j, and every store of y16 / qa: the tail of rmsnorm_quant_kernel and
// of moe_combine_rmsnorm_kernel, which differ only in how they come by h.  wave_sum: 4 floats of LDS; y_row: the MXFP6 row (256 ILP vectors).
// ACT == 0 writes no quantised bytes and needs no whole k-tiles: any K / 8.  HAD = 32 / 128 (ACT 8 / 4 only): the quantiser runs on the rotated
// f32(y16) ("petit-had/1", qact_hadamard.inc); y16 itself leaves unrotated.
template <bool BF16, int ACT, int ILP, int HAD = 0>
__device__ __forceinline__ void norm_quant_tail(const RmsQuantArgs &p, const u32x4 (&h)[ILP], const u32x4 (&wv)[ILP], float *wave_sum, u32x4 *y_row) {
    const unsigned t = threadIdx.x, row = blockIdx.x, cols = p.k / 8, m = p.m;
    const size_t row_v = (size_t)row * cols;
    // the sum of squares in the contract's order: column chains, the thread's columns ascending, butterflies 1 .. 32, the four waves ascending
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        float v[8];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned hw = h[j][d];
            unpack2<BF16>(hw, v[2 * d], v[2 * d + 1]);
        }
        s = add_rn(s, column_sumsq(v));
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1)
        s = add_rn(s, __shfl_xor(s, off));
    if (t % 64 == 0)
        wave_sum[t / 64] = s;
    __syncthreads();
    const float sumsq = add_rn(add_rn(add_rn(wave_sum[0], wave_sum[1]), wave_sum[2]), wave_sum[3]);
    const float inv = inv_rms(sumsq, p.rk, p.eps), woff = p.woff;

    unsigned char *const qa = p.qa;
    unsigned char *const qs = p.qa + qact_elem_bytes(m, p.k, ACT); // (ACT == 0: neither is used)
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        const unsigned c8 = t + 256u * j; // 8-element column
        if (c8 < cols) {
            u32x4 yv;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned hw = h[j][d], ww = wv[j][d];
                float h0, h1, w0, w1;
                unpack2<BF16>(hw, h0, h1);
                unpack2<BF16>(ww, w0, w1);
                yv[d] = pack2<BF16>(normed(h0, inv, w0, woff), normed(h1, inv, w1, woff));
            }
            if (p.y16)
                (reinterpret_cast<u32x4 *>(p.y16) + row_v)[c8] = yv;
            if constexpr (ACT == 6) {
                y_row[c8] = yv;
            } else if constexpr (ACT != 0) {
                // quantize_act32_kernel's column, on the 16-bit y
                float v[8];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned yw = yv[d];
                    unpack2<BF16>(yw, v[2 * d], v[2 * d + 1]);
                }
#include "qact_hadamard.inc"
#include "qact_column.inc"
            }
        }
    }
    if constexpr (ACT == 6) {
        // quantize_act32_fp6_kernel's block, read from the LDS row -- one thread = one 32-k block, the four blocks of a k-tile on four
        // consecutive lanes
        __syncthreads();
        const unsigned blocks = p.k / 32;
        unsigned char *const qa_hi = p.qa + qact_hi_offset(m, p.k);
#pragma unroll
        for (int i = 0; i < (ILP + 3) / 4; ++i) {
            const unsigned blk = t + 256u * i;
            if (blk < blocks) {
                u32x4 raw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    raw[q] = y_row[blk * 4 + q];
#include "qact_block6.inc"
            }
        }
    }
}
#endif

// grid = (M): one workgroup per row.  ILP = columns per thread: K <= 2048 ILP.  Lanes whose column lies past K / 8 hold zeros and add +0 to the sum;
// K / 8 is a multiple of 32, so the 16 lanes of a k-tile (and the 4 of a block) are masked together and every shuffle of the tail stays among live
// lanes.
template <bool BF16, int ACT, int ILP, int HAD = 0> __global__ __launch_bounds__(256) void rmsnorm_quant_kernel(const RmsQuantArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ float wave_sum[4];
    __shared__ u32x4 y_row[ACT == 6 ? 256 * ILP : 1]; // MXFP6 only: the 16-bit y row
    const unsigned t = threadIdx.x, row = blockIdx.x, cols = p.k / 8;
    const size_t row_v = (size_t)row * cols;
    const u32x4 *const x_row = reinterpret_cast<const u32x4 *>(p.x) + row_v;
    const u32x4 *const w_row = reinterpret_cast<const u32x4 *>(p.w);
    // every load of the row is requested before the first is used
    u32x4 h[ILP], wv[ILP];
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        const unsigned c = t + 256u * j;
        h[j] = c < cols ? x_row[c] : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < ILP; ++j) {
        const unsigned c = t + 256u * j;
        wv[j] = c < cols ? w_row[c] : u32x4{0u, 0u, 0u, 0u};
    }
    if (p.res) { // (wave-uniform: one branch around all the residual loads, not one per load)
        const u32x4 *const r_row = reinterpret_cast<const u32x4 *>(p.res) + row_v;
        u32x4 r[ILP];
#pragma unroll
        for (int j = 0; j < ILP; ++j) {
            const unsigned c = t + 256u * j;
            r[j] = c < cols ? r_row[c] : u32x4{0u, 0u, 0u, 0u};
        }
        add_residual<BF16, ILP>(h, r);
        if (p.res_out) { // a thread writes only the columns it has read: res_out may be residual or x
            u32x4 *const o_row = reinterpret_cast<u32x4 *>(p.res_out) + row_v;
#pragma unroll
            for (int j = 0; j < ILP; ++j) {
                const unsigned c = t + 256u * j;
                if (c < cols)
                    o_row[c] = h[j];
            }
        }
    }
    norm_quant_tail<BF16, ACT, ILP, HAD>(p, h, wv, wave_sum, y_row);
#endif
}

// --- the MoE top-k combine as the front end of the same row (include/petit_amd.h "Top-k combine into the norm") --------------------------------------

struct CombineNormArgs {
    RmsQuantArgs n;            // x unused: the row comes from the combine; m = num_tokens
    const void *slot;          // [num_tokens * topk][k]
    const float *topk_weights; // [num_tokens][topk]
    const void *ids;           // [num_tokens][topk], int32 or int64
    unsigned i64, topk, num_experts;
};

namespace {

// petit_moe_combine's rule: an id outside [0, num_experts) is not routed
PETIT_HD bool slot_routed(const void *ids, bool i64, size_t p, unsigned num_experts) {
    const long long v = i64 ? ((const long long *)ids)[p] : (long long)((const int *)ids)[p];
    return v >= 0 && v < (long long)num_experts;
}
// the combine's one rounding of two accumulators into a dword.  bf16: the convert moe_combine_kernel uses (the integer rule of f32_h16 on every
// number; a NaN comes out quiet with its upper payload bits, which the host spells out); fp16: f32_h16's
template <bool BF16> PETIT_HD unsigned combine_round2(float lo, float hi) {
    if constexpr (BF16) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
#else
        return (f32_h16_quiet_nan<true>(lo) & 0xffffu) | ((f32_h16_quiet_nan<true>(hi) & 0xffffu) << 16);
#endif
    }
    return pack2<false>(lo, hi);
}

} // namespace

// grid = (num_tokens): one workgroup per token, the thread map of rmsnorm_quant_kernel.  Each column has 8 f32 accumulators.  The token's ids and
// weights are read ONCE, 64 slots at a time, one per lane; a ballot turns the routed ones into a wave-uniform mask, and the slots are taken off that
// mask in ascending order, up to kSlotDepth at a time.  A group of N slots is one straight-line piece of code (combine_slots<N>): the N x ILP 16-byte
// loads, all unconditional, then the N x ILP accumulations in slot order -- so the loads of a group are in flight together and the sums are
// petit_moe_combine's.  An unrouted slot never enters the mask: its row is not read.  The residual and weight loads are requested before the first
// slot's.  A lane without a column reads column 0 of the slot rows and of the weight row in its place (no divergent branch around a load; neither
// is written by this launch) and is set to h = +0 once, after the residual add.
template <int ILP> constexpr int kSlotDepth = ILP >= 4 ? 2 : 8 / ILP;

#if defined(__HIP_DEVICE_COMPILE__)
// N routed slots of the token, lanes idx[0 .. N-1] of the chunk starting at `first`: every load, then every accumulation
template <bool BF16, int ILP, int N>
__device__ __forceinline__ void combine_slots(float (&acc)[ILP][8], const u32x4 *first, unsigned cols, const unsigned (&col)[ILP], float w_lane,
                                              const unsigned *idx) {
    u32x4 v[N][ILP];
    float w[N];
#pragma unroll
    for (int d = 0; d < N; ++d) {
        w[d] = bits_f32((unsigned)__builtin_amdgcn_readlane((int)f32_bits(w_lane), (int)idx[d]));
        const u32x4 *const s_row = first + (size_t)idx[d] * cols;
#pragma unroll
        for (int j = 0; j < ILP; ++j)
            v[d][j] = s_row[col[j]];
    }
    __builtin_amdgcn_sched_barrier(0); // the scheduler moves nothing across: no accumulation of slot 0 ahead of the loads of slot N - 1
#pragma unroll
    for (int d = 0; d < N; ++d)
#pragma unroll
        for (int j = 0; j < ILP; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned xw = v[d][j][q];
                float x0, x1;
                unpack2<BF16>(xw, x0, x1);
                acc[j][2 * q] = add_rn(acc[j][2 * q], mul_rn(x0, w[d])); // product and sum each rounded: petit_moe_combine's
                acc[j][2 * q + 1] = add_rn(acc[j][2 * q + 1], mul_rn(x1, w[d]));
            }
}
// the group of n slots, 1 <= n <= N (wave-uniform): one branch to its straight-line form
template <bool BF16, int ILP, int N>
__device__ __forceinline__ void combine_group(int n, float (&acc)[ILP][8], const u32x4 *first, unsigned cols, const unsigned (&col)[ILP],
                                              float w_lane, const unsigned *idx) {
    if (n == N)
        combine_slots<BF16, ILP, N>(acc, first, cols, col, w_lane, idx);
    else if constexpr (N > 1)
        combine_group<BF16, ILP, N - 1>(n, acc, first, cols, col, w_lane, idx);
}
#endif

template <bool BF16, int ACT, int ILP> __global__ __launch_bounds__(256) void moe_combine_rmsnorm_kernel(const CombineNormArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int kDepth = kSlotDepth<ILP>;
    __shared__ float wave_sum[4];
    __shared__ u32x4 y_row[ACT == 6 ? 256 * ILP : 1]; // MXFP6 only: the 16-bit y row
    const RmsQuantArgs &p = a.n;
    const unsigned t = threadIdx.x, row = blockIdx.x, cols = p.k / 8, topk = a.topk;
    const size_t row_v = (size_t)row * cols, p0 = (size_t)row * topk;
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    const u32x4 *const w_row = reinterpret_cast<const u32x4 *>(p.w);
    const bool has_res = p.res != nullptr; // (wave-uniform)
    unsigned col[ILP];
#pragma unroll
    for (int j = 0; j < ILP; ++j)
        col[j] = t + 256u * j < cols ? t + 256u * j : 0u;
    u32x4 wv[ILP], r[ILP];
#pragma unroll
    for (int j = 0; j < ILP; ++j)
        wv[j] = w_row[col[j]];
    if (has_res) { // a lane without a column reads the weight row here, not the residual row: residual_out may be residual, which another thread writes
        const u32x4 *const r_row = reinterpret_cast<const u32x4 *>(p.res) + row_v;
#pragma unroll
        for (int j = 0; j < ILP; ++j)
            r[j] = *(t + 256u * j < cols ? r_row + col[j] : w_row);
    }
    float acc[ILP][8];
#pragma unroll
    for (int j = 0; j < ILP; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            acc[j][i] = 0.f;
    const u32x4 *const slot = reinterpret_cast<const u32x4 *>(a.slot);
    for (unsigned base = 0; base < topk; base += 64) { // (one pass for topk <= 64)
        const unsigned s = base + (t & 63u);
        const bool routed = s < topk && slot_routed(a.ids, a.i64 != 0, p0 + s, a.num_experts);
        const float w_lane = routed ? a.topk_weights[p0 + s] : 0.f;
        unsigned long long mask = __ballot(routed);
        const u32x4 *const first = slot + (p0 + base) * cols;
        while (mask) {
            unsigned idx[kDepth];
            int n = 0;
#pragma unroll
            for (int d = 0; d < kDepth; ++d) {
                idx[d] = 0;
                if (mask) {
                    idx[d] = (unsigned)__builtin_ctzll(mask);
                    mask &= mask - 1;
                    ++n;
                }
            }
            combine_group<BF16, ILP, kDepth>(n, acc, first, cols, col, w_lane, idx);
        }
    }
    u32x4 h[ILP];
#pragma unroll
    for (int j = 0; j < ILP; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            h[j][q] = combine_round2<BF16>(acc[j][2 * q], acc[j][2 * q + 1]);
    if (has_res)
        add_residual<BF16, ILP>(h, r);
#pragma unroll
    for (int j = 0; j < ILP; ++j)
        if (!(t + 256u * j < cols))
            h[j] = zero;
    if (p.res_out) { // h with or without a residual; a thread writes only columns of the residual row that it alone has read: res_out may be residual
        u32x4 *const o_row = reinterpret_cast<u32x4 *>(p.res_out) + row_v;
#pragma unroll
        for (int j = 0; j < ILP; ++j) {
            const unsigned c = t + 256u * j;
            if (c < cols)
                o_row[c] = h[j];
        }
    }
    norm_quant_tail<BF16, ACT, ILP>(p, h, wv, wave_sum, y_row);
#endif
}

namespace {

// what both forms refuse, in one place (include/petit_amd.h lists it); kOk with *run = false: nothing to do
// k_step: what k must be a multiple of -- 256 where quantised bytes are written (whole k-tiles), 8 for the query that only sums a row
int rmsq_check(const void *qa, const void *y16, const void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
               unsigned k, int a_type, int format, bool *run, unsigned k_step = 256) {
    *run = false;
    if (m == 0 || k == 0)
        return kOk;
    if (format != 8 && format != 6 && format != 4)
        return kErrBadArgument;
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrKernelShape;
    if (k % k_step != 0 || m > kMaxM)
        return kErrProblemShape;
    if (k > 16384)
        return kErrKernelShape; // (the row is held in registers)
    if (!std::isfinite(eps) || !(eps > 0.f) || !std::isfinite(woff))
        return kErrBadArgument;
    if (!qa || !x || !w || (res_out && !res))
        return kErrBadArgument;
    if (((uintptr_t)qa | (uintptr_t)y16 | (uintptr_t)res_out | (uintptr_t)x | (uintptr_t)res | (uintptr_t)w) & 15)
        return kErrBadArgument;
    *run = true;
    return kOk;
}

template <bool BF16, int ACT, int HAD = 0> auto rmsq_kernel_for(unsigned k) {
    return k <= 2048   ? rmsnorm_quant_kernel<BF16, ACT, 1, HAD>
           : k <= 4096 ? rmsnorm_quant_kernel<BF16, ACT, 2, HAD>
           : k <= 8192 ? rmsnorm_quant_kernel<BF16, ACT, 4, HAD>
                       : rmsnorm_quant_kernel<BF16, ACT, 8, HAD>;
}
// the rotating forms: MXFP8 / MXFP4 only
template <bool BF16, int HAD> auto rmsq_rot_kernel_for(int format, unsigned k) {
    return format == 8 ? rmsq_kernel_for<BF16, 8, HAD>(k) : rmsq_kernel_for<BF16, 4, HAD>(k);
}
template <bool BF16> auto rmsq_kernel_for(int format, unsigned k) {
    return format == 8 ? rmsq_kernel_for<BF16, 8>(k) : format == 6 ? rmsq_kernel_for<BF16, 6>(k) : rmsq_kernel_for<BF16, 4>(k);
}

// (the host twin's element converts -- round to nearest even, the sign kept on a zero too, as the hardware converts do -- are e4m3_rne,
// e2m1_rne and e2m3_rne of numfmt.h, the last two on a quotient v / scale that is exact in f64)

// one row of the quantiser on f32 values z (the 16-bit y widened, or its rotation), written where the kernels write it
template <int ACT> void quantize_row_f32_host(unsigned char *ws, const float *z, unsigned m, unsigned k, unsigned row) {
    unsigned char *const qs = ws + qact_elem_bytes(m, k, ACT);
    unsigned char *const qa_hi = ws + qact_hi_offset(m, k); // (MXFP6)
    for (unsigned blk = 0; blk < k / 32; ++blk) {
        const float *const v = z + 32 * blk;
        float amax = 0.f;
        for (int i = 0; i < 32; ++i)
            amax = std::fmax(amax, std::fabs(v[i])); // (a NaN does not count, as fmaxf on the device)
        const unsigned sbyte = act_scale_byte<ACT>(amax);
        const unsigned kt = blk / 4, b = blk % 4;
        const size_t tile_row = qact_tile_row(m, kt, row);
        qs[qact_scale_dword(m, kt, row) * kQactScaleRowBytes + b] = (unsigned char)sbyte;
        if constexpr (ACT == 8) {
            const float sc = bits_f32((254u - sbyte) << 23);
            for (unsigned c = 0; c < 4; ++c) { // the block's four 8-element columns
                const unsigned col16 = 4 * b + c, u16 = col16 >> 1, half = col16 & 1u;
                unsigned char *const o = ws + tile_row * qact_row_bytes(8) + qact_fp8_unit_pos(u16) * 16 + half * 8;
                for (int i = 0; i < 8; ++i)
                    o[i] = (unsigned char)e4m3_rne(v[8 * c + i] * sc);
            }
        } else if constexpr (ACT == 4) {
            unsigned char *const o = ws + tile_row * qact_row_bytes(4) + 16 * b;
            for (int i = 0; i < 16; ++i)
                o[i] = (unsigned char)(e2m1_rne(std::ldexp((double)v[2 * i], 127 - (int)sbyte)) |
                                       (e2m1_rne(std::ldexp((double)v[2 * i + 1], 127 - (int)sbyte)) << 4));
        } else {
            unsigned char bytes[24] = {};
            for (int i = 0; i < 32; ++i) { // element i at bits [6 i, 6 i + 6)
                const unsigned code = e2m3_rne(std::ldexp((double)v[i], 127 - (int)sbyte));
                const unsigned bit = 6 * i;
                bytes[bit / 8] |= (unsigned char)(code << (bit % 8));
                if (bit % 8 > 2)
                    bytes[bit / 8 + 1] |= (unsigned char)(code >> (8 - bit % 8));
            }
            memcpy(ws + tile_row * qact_row_bytes(6) + 16 * b, bytes, 16);
            memcpy(qa_hi + tile_row * kQactHiRowBytes + 8 * qact_fp6_hi_slot(b), bytes + 16, 8);
        }
    }
}
// one row of the quantiser on the 16-bit y; had = 32 / 128: on the rotation of f32(y) ("petit-had/1": no 16-bit rounding in between)
template <bool BF16, int ACT> void quantize_row_host(unsigned char *ws, const uint16_t *y, unsigned m, unsigned k, unsigned row, unsigned had = 0) {
    std::vector<float> z(k);
    for (unsigned i = 0; i < k; ++i)
        z[i] = h16_f32<BF16>(y[i]);
    if (had)
        hadamard_row_host(z.data(), k, had);
    quantize_row_f32_host<ACT>(ws, z.data(), m, k, row);
}

// steps 2 and 3 on one row of h -- the kernel's reduction, walked literally: 256 thread sums, six butterflies inside each wave of 64, the four
// waves in ascending order
template <bool BF16> float row_inv_host(const uint16_t *h, unsigned k, float rk, float eps) {
    const unsigned cols = k / 8;
    float s[256];
    for (unsigned t = 0; t < 256; ++t) {
        s[t] = 0.f;
        for (unsigned c = t; c < cols; c += 256) {
            float v[8];
            for (int i = 0; i < 8; ++i)
                v[i] = h16_f32<BF16>(h[8 * c + i]);
            s[t] = add_rn(s[t], column_sumsq(v));
        }
    }
    for (unsigned off = 1; off < 64; off <<= 1) {
        float n[256];
        for (unsigned t = 0; t < 256; ++t)
            n[t] = add_rn(s[t], s[t ^ off]);
        memcpy(s, n, sizeof(s));
    }
    return inv_rms(add_rn(add_rn(add_rn(s[0], s[64]), s[128]), s[192]), rk, eps);
}
template <bool BF16> void add_row_host(uint16_t *h, const uint16_t *x, const uint16_t *r, unsigned k) {
    for (unsigned i = 0; i < k; ++i)
        h[i] = r ? (uint16_t)f32_h16<BF16>(add_rn(h16_f32<BF16>(x[i]), h16_f32<BF16>(r[i]))) : x[i];
}

template <bool BF16, int ACT> void rmsq_host(const RmsQuantArgs &p, unsigned had = 0) {
    const unsigned k = p.k;
    std::vector<uint16_t> h(k), y(k);
    const uint16_t *const w = (const uint16_t *)p.w;
    for (unsigned row = 0; row < p.m; ++row) {
        const uint16_t *const x = (const uint16_t *)p.x + (size_t)row * k;
        const uint16_t *const r = p.res ? (const uint16_t *)p.res + (size_t)row * k : nullptr;
        add_row_host<BF16>(h.data(), x, r, k);
        if (p.res_out)
            memcpy((uint16_t *)p.res_out + (size_t)row * k, h.data(), 2 * (size_t)k);
        const float inv = row_inv_host<BF16>(h.data(), k, p.rk, p.eps);
        for (unsigned i = 0; i < k; ++i)
            y[i] = (uint16_t)f32_h16<BF16>(normed(h16_f32<BF16>(h[i]), inv, h16_f32<BF16>(w[i]), p.woff));
        if (p.y16)
            memcpy((uint16_t *)p.y16 + (size_t)row * k, y.data(), 2 * (size_t)k);
        quantize_row_host<BF16, ACT>(p.qa, y.data(), p.m, k, row, had);
    }
}

RmsQuantArgs rmsq_args(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
                       unsigned k) {
    return RmsQuantArgs{(unsigned char *)qa, y16, res_out, x, res, w, eps, woff, 1.0f / (float)k, m, k};
}

} // namespace

int rmsnorm_quantize(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m, unsigned k,
                     int a_type, int format, hipStream_t stream) {
    bool run;
    if (const int rc = rmsq_check(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, &run); rc != kOk || !run)
        return rc;
    const auto kern = a_type == kDataTypeBf16 ? rmsq_kernel_for<true>(format, k) : rmsq_kernel_for<false>(format, k);
    hipLaunchKernelGGL(kern, dim3(m), dim3(256), 0, stream, rmsq_args(qa, y16, res_out, x, res, w, eps, woff, m, k));
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int rmsnorm_quantize_host(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
                          unsigned k, int a_type, int format) {
    bool run;
    if (const int rc = rmsq_check(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, &run); rc != kOk || !run)
        return rc;
    const RmsQuantArgs p = rmsq_args(qa, y16, res_out, x, res, w, eps, woff, m, k);
    const bool bf16 = a_type == kDataTypeBf16;
    if (format == 8)
        bf16 ? rmsq_host<true, 8>(p) : rmsq_host<false, 8>(p);
    else if (format == 6)
        bf16 ? rmsq_host<true, 6>(p) : rmsq_host<false, 6>(p);
    else
        bf16 ? rmsq_host<true, 4>(p) : rmsq_host<false, 4>(p);
    return kOk;
}

// The rotating forms (include/petit_amd.h "Block-Hadamard rotation"): block 0 is the entry above; what it refuses is refused here, then MXFP6.
// *run = false with kOk: nothing to do, or (block == 0) the caller delegates
namespace {
int rmsq_rot_check(const void *qa, const void *y16, const void *res_out, const void *x, const void *res, const void *w, float eps, float woff,
                   unsigned m, unsigned k, int a_type, int format, unsigned block, bool *run) {
    *run = false;
    if (!hadamard_block_ok(block))
        return kErrBadArgument;
    if (block == 0)
        return kOk;
    if (const int rc = rmsq_check(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, run); rc != kOk || !*run)
        return rc;
    if (format == 6) {
        *run = false;
        return kErrKernelShape; // (its converts read 16-bit patterns: no f32 form)
    }
    return kOk;
}
} // namespace

int rmsnorm_quantize_rot(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
                         unsigned k, int a_type, int format, unsigned block, hipStream_t stream) {
    bool run;
    if (const int rc = rmsq_rot_check(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, block, &run); rc != kOk)
        return rc;
    if (block == 0)
        return rmsnorm_quantize(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, stream);
    if (!run)
        return kOk;
    const bool bf16 = a_type == kDataTypeBf16;
    const auto kern = block == 32 ? (bf16 ? rmsq_rot_kernel_for<true, 32>(format, k) : rmsq_rot_kernel_for<false, 32>(format, k))
                                  : (bf16 ? rmsq_rot_kernel_for<true, 128>(format, k) : rmsq_rot_kernel_for<false, 128>(format, k));
    hipLaunchKernelGGL(kern, dim3(m), dim3(256), 0, stream, rmsq_args(qa, y16, res_out, x, res, w, eps, woff, m, k));
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int rmsnorm_quantize_rot_host(void *qa, void *y16, void *res_out, const void *x, const void *res, const void *w, float eps, float woff, unsigned m,
                              unsigned k, int a_type, int format, unsigned block) {
    bool run;
    if (const int rc = rmsq_rot_check(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format, block, &run); rc != kOk)
        return rc;
    if (block == 0)
        return rmsnorm_quantize_host(qa, y16, res_out, x, res, w, eps, woff, m, k, a_type, format);
    if (!run)
        return kOk;
    const RmsQuantArgs p = rmsq_args(qa, y16, res_out, x, res, w, eps, woff, m, k);
    const bool bf16 = a_type == kDataTypeBf16;
    if (format == 8)
        bf16 ? rmsq_host<true, 8>(p, block) : rmsq_host<false, 8>(p, block);
    else
        bf16 ? rmsq_host<true, 4>(p, block) : rmsq_host<false, 4>(p, block);
    return kOk;
}

// the f32 `inv` of every row as the host twin (and so the kernel) forms it: what a test of steps 2 and 3 needs, since y carries it only through
// a 16-bit rounding
int rmsnorm_inv_host(float *inv, const void *x, const void *res, float eps, unsigned m, unsigned k, int a_type) {
    bool run;
    alignas(16) static const uint64_t aligned[2] = {0, 0}; // (stands in for the pointers this query does not take)
    // any k % 8 == 0: the stated order needs no whole k-tiles, and the 16-bit-only form of petit_moe_combine_rmsnorm norms such rows
    if (const int rc = rmsq_check(aligned, nullptr, nullptr, x, res, aligned, eps, 0.f, m, k, a_type, 8, &run, 8); rc != kOk || !run)
        return rc;
    if (!inv)
        return kErrBadArgument;
    std::vector<uint16_t> h(k);
    for (unsigned row = 0; row < m; ++row) {
        const uint16_t *const xr = (const uint16_t *)x + (size_t)row * k;
        const uint16_t *const rr = res ? (const uint16_t *)res + (size_t)row * k : nullptr;
        if (a_type == kDataTypeBf16) {
            add_row_host<true>(h.data(), xr, rr, k);
            inv[row] = row_inv_host<true>(h.data(), k, 1.0f / (float)k, eps);
        } else {
            add_row_host<false>(h.data(), xr, rr, k);
            inv[row] = row_inv_host<false>(h.data(), k, 1.0f / (float)k, eps);
        }
    }
    return kOk;
}

// petit_quantize_activations on HOST pointers: quantize_row_host on every row of a 16-bit [m][k] matrix (what the twins above write after the norm).
// It refuses what petit_quantize_activations refuses, and an unknown format.
int quantize_activations_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format) {
    if (m == 0 || k == 0)
        return kOk;
    if (!qa || !a || (((uintptr_t)qa | (uintptr_t)a) & 15) || (format != 8 && format != 6 && format != 4))
        return kErrBadArgument;
    if (k % 256 != 0)
        return kErrProblemShape;
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrKernelShape;
    const bool bf16 = a_type == kDataTypeBf16;
    for (unsigned row = 0; row < m; ++row) {
        const uint16_t *const y = (const uint16_t *)a + (size_t)row * k;
        unsigned char *const ws = (unsigned char *)qa;
        if (format == 8)
            bf16 ? quantize_row_host<true, 8>(ws, y, m, k, row) : quantize_row_host<false, 8>(ws, y, m, k, row);
        else if (format == 6)
            bf16 ? quantize_row_host<true, 6>(ws, y, m, k, row) : quantize_row_host<false, 6>(ws, y, m, k, row);
        else
            bf16 ? quantize_row_host<true, 4>(ws, y, m, k, row) : quantize_row_host<false, 4>(ws, y, m, k, row);
    }
    return kOk;
}

// petit_quantize_activations_rot on HOST pointers: the same rows, each rotated in f32 before the quantiser
int quantize_activations_rot_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format, unsigned block) {
    if (!hadamard_block_ok(block))
        return kErrBadArgument;
    if (block == 0)
        return quantize_activations_host(qa, a, m, k, a_type, format);
    if (m == 0 || k == 0)
        return kOk;
    if (!qa || !a || (((uintptr_t)qa | (uintptr_t)a) & 15) || (format != 8 && format != 6 && format != 4))
        return kErrBadArgument;
    if (k % 256 != 0)
        return kErrProblemShape;
    if ((a_type != kDataTypeBf16 && a_type != kDataTypeFp16) || format == 6)
        return kErrKernelShape;
    const bool bf16 = a_type == kDataTypeBf16;
    for (unsigned row = 0; row < m; ++row) {
        const uint16_t *const y = (const uint16_t *)a + (size_t)row * k;
        unsigned char *const ws = (unsigned char *)qa;
        if (format == 8)
            bf16 ? quantize_row_host<true, 8>(ws, y, m, k, row, block) : quantize_row_host<false, 8>(ws, y, m, k, row, block);
        else
            bf16 ? quantize_row_host<true, 4>(ws, y, m, k, row, block) : quantize_row_host<false, 4>(ws, y, m, k, row, block);
    }
    return kOk;
}

// --- petit_moe_combine_rmsnorm ----------------------------------------------------------------------------------------------------------------

namespace {

// what both forms refuse, in one place (include/petit_amd.h lists it); kOk with *run = false: nothing to do
int mcn_check(const void *qa, const void *y16, const void *res_out, const void *slot, const float *tw, const void *ids, const void *res,
              const void *w, float eps, float woff, unsigned num_tokens, unsigned topk, unsigned k, unsigned num_experts, int a_type, int format,
              bool *run) {
    *run = false;
    if (num_tokens == 0 || k == 0)
        return kOk;
    if (format != 0 && format != 8 && format != 6 && format != 4)
        return kErrBadArgument;
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrKernelShape;
    if (k % 8 != 0 || (format != 0 && k % 256 != 0))
        return kErrProblemShape;
    if (topk == 0 || num_experts == 0 || num_experts > kMoeMaxExperts || (uint64_t)num_tokens * topk >= (1ull << 31) || num_tokens > kMaxM)
        return kErrProblemShape;
    if (k > 16384)
        return kErrKernelShape; // (the row is held in registers)
    if (!std::isfinite(eps) || !(eps > 0.f) || !std::isfinite(woff))
        return kErrBadArgument;
    if (!slot || !tw || !ids || !w)
        return kErrBadArgument;
    if (format == 0 ? (qa != nullptr || !y16) : !qa)
        return kErrBadArgument;
    if (((uintptr_t)qa | (uintptr_t)y16 | (uintptr_t)res_out | (uintptr_t)slot | (uintptr_t)res | (uintptr_t)w) & 15)
        return kErrBadArgument;
    *run = true;
    return kOk;
}

template <bool BF16, int ACT> auto mcn_kernel_for(unsigned k) {
    return k <= 2048   ? moe_combine_rmsnorm_kernel<BF16, ACT, 1>
           : k <= 4096 ? moe_combine_rmsnorm_kernel<BF16, ACT, 2>
           : k <= 8192 ? moe_combine_rmsnorm_kernel<BF16, ACT, 4>
                       : moe_combine_rmsnorm_kernel<BF16, ACT, 8>;
}
template <bool BF16> auto mcn_kernel_for(int format, unsigned k) {
    return format == 8   ? mcn_kernel_for<BF16, 8>(k)
           : format == 6 ? mcn_kernel_for<BF16, 6>(k)
           : format == 4 ? mcn_kernel_for<BF16, 4>(k)
                         : mcn_kernel_for<BF16, 0>(k);
}

template <bool BF16, int ACT> void mcn_host(const CombineNormArgs &a) {
    const RmsQuantArgs &p = a.n;
    const unsigned k = p.k;
    std::vector<float> acc(k);
    std::vector<uint16_t> c(k), h(k), y(k);
    const uint16_t *const w = (const uint16_t *)p.w;
    for (unsigned row = 0; row < p.m; ++row) {
        std::fill(acc.begin(), acc.end(), 0.f);
        for (unsigned s = 0; s < a.topk; ++s) {
            const size_t e = (size_t)row * a.topk + s;
            if (!slot_routed(a.ids, a.i64 != 0, e, a.num_experts))
                continue; // (the row is not read)
            const float tw = a.topk_weights[e];
            const uint16_t *const x = (const uint16_t *)a.slot + e * k;
            for (unsigned i = 0; i < k; ++i)
                acc[i] = add_rn(acc[i], mul_rn(h16_f32<BF16>(x[i]), tw));
        }
        for (unsigned i = 0; i < k; i += 2) {
            const unsigned d = combine_round2<BF16>(acc[i], acc[i + 1]);
            c[i] = (uint16_t)d, c[i + 1] = (uint16_t)(d >> 16);
        }
        const uint16_t *const r = p.res ? (const uint16_t *)p.res + (size_t)row * k : nullptr;
        add_row_host<BF16>(h.data(), c.data(), r, k);
        if (p.res_out)
            memcpy((uint16_t *)p.res_out + (size_t)row * k, h.data(), 2 * (size_t)k);
        const float inv = row_inv_host<BF16>(h.data(), k, p.rk, p.eps);
        for (unsigned i = 0; i < k; ++i)
            y[i] = (uint16_t)f32_h16<BF16>(normed(h16_f32<BF16>(h[i]), inv, h16_f32<BF16>(w[i]), p.woff));
        if (p.y16)
            memcpy((uint16_t *)p.y16 + (size_t)row * k, y.data(), 2 * (size_t)k);
        if constexpr (ACT != 0)
            quantize_row_host<BF16, ACT>(p.qa, y.data(), p.m, k, row);
    }
}

CombineNormArgs mcn_args(void *qa, void *y16, void *res_out, const void *slot, const float *tw, const void *ids, int i64, const void *res,
                         const void *w, float eps, float woff, unsigned num_tokens, unsigned topk, unsigned k, unsigned num_experts) {
    return CombineNormArgs{rmsq_args(qa, y16, res_out, nullptr, res, w, eps, woff, num_tokens, k), slot, tw, ids, i64 ? 1u : 0u, topk, num_experts};
}

} // namespace

int moe_combine_rmsnorm(void *qa, void *y16, void *res_out, const void *slot, const float *tw, const void *ids, int i64, const void *res,
                        const void *w, float eps, float woff, unsigned num_tokens, unsigned topk, unsigned k, unsigned num_experts, int a_type,
                        int format, hipStream_t stream) {
    bool run;
    if (const int rc = mcn_check(qa, y16, res_out, slot, tw, ids, res, w, eps, woff, num_tokens, topk, k, num_experts, a_type, format, &run);
        rc != kOk || !run)
        return rc;
    const auto kern = a_type == kDataTypeBf16 ? mcn_kernel_for<true>(format, k) : mcn_kernel_for<false>(format, k);
    hipLaunchKernelGGL(kern, dim3(num_tokens), dim3(256), 0, stream,
                       mcn_args(qa, y16, res_out, slot, tw, ids, i64, res, w, eps, woff, num_tokens, topk, k, num_experts));
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int moe_combine_rmsnorm_host(void *qa, void *y16, void *res_out, const void *slot, const float *tw, const void *ids, int i64, const void *res,
                             const void *w, float eps, float woff, unsigned num_tokens, unsigned topk, unsigned k, unsigned num_experts,
                             int a_type, int format) {
    bool run;
    if (const int rc = mcn_check(qa, y16, res_out, slot, tw, ids, res, w, eps, woff, num_tokens, topk, k, num_experts, a_type, format, &run);
        rc != kOk || !run)
        return rc;
    const CombineNormArgs a = mcn_args(qa, y16, res_out, slot, tw, ids, i64, res, w, eps, woff, num_tokens, topk, k, num_experts);
    const bool bf16 = a_type == kDataTypeBf16;
    if (format == 8)
        bf16 ? mcn_host<true, 8>(a) : mcn_host<false, 8>(a);
    else if (format == 6)
        bf16 ? mcn_host<true, 6>(a) : mcn_host<false, 6>(a);
    else if (format == 4)
        bf16 ? mcn_host<true, 4>(a) : mcn_host<false, 4>(a);
    else
        bf16 ? mcn_host<true, 0>(a) : mcn_host<false, 0>(a);
    return kOk;
}

} // namespace petit_amd
