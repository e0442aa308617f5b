// gemm_native_invariant.hpp -- the batch-invariant GEMM on the native class (include/petit_amd.h "Batch-invariant GEMM on the native class"):
// raw MXFP4 weights against MXFP8 / MXFP6 / MXFP4 activations ("petit-qact/1" bytes) on v_mfma_scale_f32_32x32x64_f8f6f4, every output element a
// pure function of its quantised activation row, the weights, the scales and the bias -- never of M, of the row's position, or of the launch form.
//
// K is cut into S slices of L (geometry, gemm_invariant_host.h: a function of (n, k) alone).  The partial sum p_s of a slice is ONE
// chain of the 32x32x64 instruction from a zero accumulator: k-tiles of 128 ascending, two instructions per k-tile -- P1 (k 0..63 of the tile),
// then P2 (k 64..127).  The weight operand is the pair of neighbouring n-tiles merged in registers (merge_tiles, gemm_wide.hpp: the lane's four
// registers ARE the FP4 operand) with the merged span-record byte as its E8M0 scale; the activation operand is the row's quantised bytes of that
// k-tile (layouts: gemm_native32.hpp) and the E8M0 byte of the lane's block.  The result is ((p_0 + p_1) + ... + p_{S-1}) * gs + bias in fp32.
// Two forms produce those bits:
//   split (m <= the form switch): grid = pairs of n-tiles / 4 x S x m-tiles of 32.  A wave owns one 32 x 32 tile of ONE slice and stores it to
//     slab s of [S][m][n] fp32 with plain vector stores; invariant_fold_kernel (gemm_invariant.hpp) adds the slabs in ascending order and applies
//     scale, bias and activation.  Weights (non-temporal) and the row's quantised bytes go straight to VGPRs through bounded descriptors, in a
//     register ring kDepth k-tiles deep; no LDS, no barrier, no atomics, tickets or fences.
//   whole (above): grid = slots / 4 x m-blocks of 64 rows.  The workgroup stages its 64-row activation tile of every k-tile in LDS once
//     (double-buffered, one barrier per k-tile, the swizzle of gemm_native32.hpp); a wave owns 2 m-blocks of 32 x 2 pairs of n-tiles (gated: the
//     gate pair t and the up pair t + ntiles / 4), walks ALL the slices, accumulates each from zero and joins it to the running total with one
//     plain fp32 add per accumulator -- the slab sum's additions -- and applies the epilogue itself.  No wave-level K split, no slab workspace.
// The instruction computes every output element from its own row and column alone, and rows past M read zeros through the descriptor (the
// descriptor of a k-tile ends with the workgroup's last valid row), so what sits next to a row in its tile cannot reach it.
//
// WF names the weight operand, as in gemm_native32.hpp: 4 = raw MXFP4 (everything above); 6 = the "petit-cdna4-nv6/1" image of NVFP4 weights
// (layout.h): block `pair` of 32 weight rows is stored as the instruction's own FP6 e2m3 operand -- lane 32 h + r holds row r, three 16-byte
// units per lane and k-tile (registers 0-3 of P1, registers 0-3 of P2, and {P1 r4, P1 r5, P2 r4, P2 r5}), the E8M0 byte of instruction q at
// [q][t] of the lane's span record -- so a wave loads its operand as it stands (no merge_tiles) and everything after the MFMA is shared: row c
// of the 32 at lane c, the lane's block 2 q + h, the same output columns.  The entries take n % 32 == 0, so the image has no padded block.
//
// Each form's body is stated once, in gemm_native_invariant_split.inc and gemm_native_invariant_whole.inc.  The dense kernels below and the
// routed-expert kernels (gemm_native_invariant_moe.hpp) are a prologue each -- the weight and scale bases, the tile's first row m0 and its
// rows_valid, the row of C an output row goes to -- and the include.
#pragma once

#include <hip/hip_runtime.h>

#include "gemm_invariant.hpp"
#include "gemm_native32.hpp"

namespace petit_amd {

struct NativeInvariantArgs {
    void *c;                 // [m][n] (gated: [m][n/2]) 16-bit
    const unsigned char *qa; // "petit-qact/1" bytes of (m, k, ACT)
    const void *w;           // packed weights
    const void *s;           // packed MX scales
    const float *gs;         // device pointer to one float, or null: no multiply
    const void *bias;        // [n] in c's type, or null: no add
    float *slabs;            // split form: [slices][m][n] fp32
    unsigned m, n, k;
    unsigned slice_k, slices; // L, S
    unsigned act;             // PETIT_ACTIVATION_*
};

// bytes of one row and k-tile in the (first) data image: 128 (MXFP8) / 64 (MXFP4; MXFP6: registers 0-3 of every block)
template <int ACT> constexpr unsigned native_inv_row_bytes() { return qact_row_bytes(ACT); }
// 16-byte units of one k-tile a lane holds: P1 + P2 (MXFP6: the two register 0-3 units and the unit with registers 4-5 of both)
template <int ACT> constexpr int native_inv_frag_units() { return ACT == 8 ? 4 : ACT == 6 ? 3 : 2; }

// the activation operand of instruction q (0: P1, 1: P2) from the lane's units of one k-tile
template <int ACT> __device__ __forceinline__ i32x8 native_inv_aop(const u32x4 (&a)[native_inv_frag_units<ACT>()], const int q) {
    if constexpr (ACT == 8) {
        const u32x4 lo = a[2 * q], hi = a[2 * q + 1];
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    } else if constexpr (ACT == 6) {
        const u32x4 lo = a[q], tail = a[2];
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)tail[2 * q], (int)tail[2 * q + 1], 0, 0};
    } else {
        const u32x4 lo = a[q];
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], 0, 0, 0, 0};
    }
}

// 16-byte units of one k-tile a lane holds of its 32 weight rows: the pair's two n-tiles (raw MXFP4) / the image block's three planes
template <int WF> constexpr int native_inv_w_units() { return WF == 6 ? 3 : 2; }

// one k-tile of one accumulator's chain: P1, then P2.  wop / wsc: the weight operands and E8M0 bytes of the two instructions.
template <int ACT, int WF = 4>
__device__ __forceinline__ f32x16 native_inv_ktile(f32x16 acc, const i32x8 (&wop)[2], const unsigned (&wsc)[2],
                                                   const u32x4 (&a)[native_inv_frag_units<ACT>()], const unsigned a_sc1, const unsigned a_sc2) {
    constexpr int kBlgp = ACT == 8 ? 0 : ACT == 6 ? 2 : 4; // the activation operand's format: e4m3 / e2m3 / e2m1
    constexpr int kCbsz = WF == 6 ? 2 : 4;                 // the weight operand's: e2m3 (the image) / e2m1 (raw MXFP4)
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wop[0], native_inv_aop<ACT>(a, 0), acc, kCbsz, kBlgp, 0, (int)wsc[0], 0, (int)a_sc1);
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wop[1], native_inv_aop<ACT>(a, 1), acc, kCbsz, kBlgp, 0, (int)wsc[1], 0, (int)a_sc2);
    return acc;
}

// the pair's weight operands and scales from the raw loads of its two n-tiles
__device__ __forceinline__ void native_inv_merge(const u32x4 w0, const u32x4 w1, const unsigned s0, const unsigned s1, i32x8 (&wop)[2],
                                                 unsigned (&wsc)[2]) {
    unsigned pw[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        merge_tiles(w0[j], w1[j], pw[0][j], pw[1][j]);
    merge_tiles(s0, s1, wsc[0], wsc[1]);
#pragma unroll
    for (int q = 0; q < 2; ++q)
        wop[q] = i32x8{(int)pw[q][0], (int)pw[q][1], (int)pw[q][2], (int)pw[q][3], 0, 0, 0, 0};
}

// WF = 6: the block's operands from its three planes -- P1 is plane 0 followed by plane 2's words 0 and 1, P2 plane 1 followed by words 2 and 3
// (the assembly native_inv_aop<6> does for MXFP6 activations) -- and the two bytes [q][t] of the lane's span record
__device__ __forceinline__ void native_inv_image_ops(const u32x4 (&w)[3], const unsigned (&sc)[2], i32x8 (&wop)[2], unsigned (&wsc)[2]) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        wop[q] = i32x8{(int)w[q][0], (int)w[q][1], (int)w[q][2], (int)w[q][3], (int)w[2][2 * q], (int)w[2][2 * q + 1], 0, 0};
        wsc[q] = sc[q];
    }
}

// The split form.  ACT: 8 / 6 / 4.  kDepth: k-tiles in flight per wave.  (AT does not enter the arithmetic: the slabs are fp32.)
template <class AT, int ACT, int kDepth> __global__ __launch_bounds__(256) void native_invariant_split_kernel(const NativeInvariantArgs p) {
    const unsigned lane = threadIdx.x & 63u, m_l = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned ntiles = p.n / kTileN, pairs = ntiles / 2, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    const unsigned pair = blockIdx.x * 4u + wave; // a wave's slot is its pair of n-tiles
    if (pair >= pairs)
        return; // (wave-uniform; the loop has no barrier)
    const unsigned m0 = blockIdx.z * 32u, s = blockIdx.y;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 32u ? rows_left : 32u; // (the grid keeps m0 < m)
    const char *const w_base = (const char *)p.w, *const s_base = (const char *)p.s;
    constexpr int WF = 4;
#include "gemm_native_invariant_split.inc"
}

// The split form on the image (WF = 6): p.w is the image's elements, p.s its scale region; a wave's `pair` is its block of 32 weight rows.
template <class AT, int ACT, int kDepth> __global__ __launch_bounds__(256) void native_invariant_nv_split_kernel(const NativeInvariantArgs p) {
    const unsigned lane = threadIdx.x & 63u, m_l = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned pairs = p.n / 32u, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    const unsigned pair = blockIdx.x * 4u + wave;
    if (pair >= pairs)
        return; // (wave-uniform; the loop has no barrier)
    const unsigned m0 = blockIdx.z * 32u, s = blockIdx.y;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 32u ? rows_left : 32u; // (the grid keeps m0 < m)
    const char *const w_base = (const char *)p.w, *const s_base = (const char *)p.s;
    constexpr int WF = 6;
#include "gemm_native_invariant_split.inc"
}

// The whole form.  A workgroup owns 64 rows x 4 slots (one per wave); a slot is two pairs of n-tiles: pairs 2 t and 2 t + 1, or (gated) gate pair t
// and up pair t + ntiles / 4.  Per k-tile the 256 threads fetch the 64-row activation tile once (one k-tile ahead; the tile is ONE contiguous run
// of the k-tile-major layout, rows past the tile's last valid row read zeros through the descriptor) and drop it into the other half of a
// double-buffered LDS image with the unit swizzle of gemm_native32.hpp (the 16 lanes of a ds_read_b128 group hit 16 different slots); one barrier
// per k-tile.  The weights stream into a register ring kNativeWholeRing k-tiles deep.  Every accumulator keeps ONE chain per slice; at a slice
// boundary it joins the running total.
constexpr int kNativeWholeRing = 2;
template <int ACT> struct NativeWholeLds {
    static constexpr unsigned kRowB = native_inv_row_bytes<ACT>(), U = kRowB / 16;
    static constexpr unsigned kData = 64 * kRowB, kHi = ACT == 6 ? 64 * kQactHiRowBytes : 0, kScale = 64 * kQactScaleRowBytes;
    static constexpr unsigned kBuf = kData + kHi + kScale;
};
template <class AT, int ACT> __global__ __launch_bounds__(256) void native_invariant_whole_kernel(const NativeInvariantArgs p) {
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned slot = blockIdx.x * 4u + wave;
    const unsigned m0 = blockIdx.y * 64u;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 64u ? rows_left : 64u; // (the grid keeps m0 < m)
    const char *const w_base = (const char *)p.w, *const s_base = (const char *)p.s;
    const float *const gs = p.gs;
    const void *const bias = p.bias;
    auto c_row = [](unsigned row) { return row; };
    constexpr int WF = 4;
#include "gemm_native_invariant_whole.inc"
}

// The whole form on the image (WF = 6): a slot is two blocks of 32 weight rows -- 2 t and 2 t + 1, or (gated) gate block t and up block t + n / 64.
template <class AT, int ACT> __global__ __launch_bounds__(256) void native_invariant_nv_whole_kernel(const NativeInvariantArgs p) {
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned slot = blockIdx.x * 4u + wave;
    const unsigned m0 = blockIdx.y * 64u;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 64u ? rows_left : 64u; // (the grid keeps m0 < m)
    const char *const w_base = (const char *)p.w, *const s_base = (const char *)p.s;
    const float *const gs = p.gs;
    const void *const bias = p.bias;
    auto c_row = [](unsigned row) { return row; };
    constexpr int WF = 6;
#include "gemm_native_invariant_whole.inc"
}

constexpr int kNativeInvariantSplitDepth = 3;

// one activation type's launches of one weight operand; instantiated by gemm_native_invariant_{bf16,f16}.hip (WF = 4) and
// gemm_native_invariant_nv_{bf16,f16}.hip (WF = 6)
template <class AT, int ACT, int WF> void native_invariant_launch_fmt(const NativeInvariantArgs &p, const invariant::Plan &plan, hipStream_t stream) {
    if (plan.split) {
        if constexpr (WF == 6)
            hipLaunchKernelGGL((native_invariant_nv_split_kernel<AT, ACT, kNativeInvariantSplitDepth>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((native_invariant_split_kernel<AT, ACT, kNativeInvariantSplitDepth>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        InvariantArgs f{}; // the fold of the exact class
        f.c = p.c, f.gs = p.gs, f.bias = p.bias, f.slabs = p.slabs, f.m = p.m, f.n = p.n, f.k = p.k, f.slice_k = p.slice_k, f.slices = p.slices,
        f.act = p.act;
        hipLaunchKernelGGL((invariant_fold_kernel<AT>), invariant_grid(plan.fold), dim3(256), 0, stream, f);
    } else {
        if constexpr (WF == 6)
            hipLaunchKernelGGL((native_invariant_nv_whole_kernel<AT, ACT>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((native_invariant_whole_kernel<AT, ACT>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
    }
}
template <class AT, int WF = 4>
void native_invariant_launch(const NativeInvariantArgs &p, int act_format, const invariant::Plan &plan, hipStream_t stream) {
    if (act_format == 8)
        native_invariant_launch_fmt<AT, 8, WF>(p, plan, stream);
    else if (act_format == 6)
        native_invariant_launch_fmt<AT, 6, WF>(p, plan, stream);
    else
        native_invariant_launch_fmt<AT, 4, WF>(p, plan, stream);
}

} // namespace petit_amd
