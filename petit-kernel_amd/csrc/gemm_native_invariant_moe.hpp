// gemm_native_invariant_moe.hpp -- the batch-invariant routed-expert (MoE) GEMM on the native class (include/petit_amd.h "Batch-invariant MoE
// launch on the native class"): grouped row r of expert e gets, bit for bit, row 0 of the dense native-invariant call
// (gemm_native_invariant.hpp) on that row's quantised bytes and expert e's tensors.
//
// The chain is shared with the dense kernels: both forms include the dense kernels' bodies (gemm_native_invariant_split.inc,
// gemm_native_invariant_whole.inc) on expert e's tensors, gs[e] and bias + e * n.  What is this header's is the addressing, which is
// gemm_invariant_moe.hpp's: a launch sized for every possible routing, ONE linear workgroup index in grid x, slot -> (expert, m-tile) by
// moe_locate on the device (the clamp rule), scattered C rows.
//
// The quantised activations are the image of the m GROUPED rows, k-tile-major (row r of k-tile kt at (kt * m + r) * row_bytes), so a tile's rows
// are one contiguous run as in the dense kernels: its descriptor starts at the tile's first grouped row and ends with the tile's last valid row
// of this expert -- rows of the next expert, or past m, read zeros.
//   split: slots = ceil(m / 32) + min(E, m).  A wave owns (slot, slice, pair of n-tiles) and stores its fp32 tile to slab s of [S][m][n],
//     indexed by GROUPED row, rows below rows_valid only.  The second launch is invariant_moe_fold_kernel (gemm_invariant_moe.hpp) as it
//     stands: it walks its own 16-row slot map over the same offsets, so slabs indexed by grouped row are all it needs, and nothing in the
//     workspace needs clearing.
//   whole: slots = ceil(m / 64) + min(E, m).  A workgroup owns (slot, 4 slots of two pairs of n-tiles); the epilogue in the launch, C scattered.
#pragma once

#include "gemm_invariant_moe.hpp"
#include "gemm_native_invariant.hpp"

namespace petit_amd {

struct NativeInvariantMoeArgs {
    void *c;                 // [c_rows][n] (gated: [c_rows][n/2]) 16-bit
    const unsigned char *qa; // "petit-qact/1" bytes of (m, k, ACT): the m grouped rows
    const void *w;           // the experts' packed weights, back to back
    const void *s;           // the experts' packed MX scales, back to back
    const float *gs;         // [E]
    const void *bias;        // [E][n] in c's type, or null
    float *slabs;            // split form: [slices][m][n] fp32
    const int *offsets;      // [E + 1], device
    const int *c_idx;        // [m] or null: the identity
    unsigned m, n, k;
    unsigned slice_k, slices; // L, S
    unsigned act;             // PETIT_ACTIVATION_*
    unsigned experts, c_rows;
    unsigned nblocks;         // workgroups along n per (slot[, slice])
};

// C row of grouped row `row`, or ~0u: the store is skipped
__device__ __forceinline__ unsigned native_moe_c_row(const NativeInvariantMoeArgs &p, unsigned row) {
    const unsigned c = p.c_idx ? (unsigned)p.c_idx[row] : row;
    return c < p.c_rows ? c : ~0u;
}

// The split form: a wave on (expert, m-tile of 32, slice, pair of n-tiles).
template <class AT, int ACT, int kDepth> __global__ __launch_bounds__(256) void native_invariant_moe_split_kernel(const NativeInvariantMoeArgs p) {
    const unsigned lane = threadIdx.x & 63u, m_l = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned ntiles = p.n / kTileN, pairs = ntiles / 2, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    // the linear index: n-block fastest, then the slice, then the slot
    const unsigned nb = blockIdx.x % p.nblocks, rest = blockIdx.x / p.nblocks;
    const unsigned s = rest % p.slices, slot = rest / p.slices;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 32u, slot, t))
        return; // a slot past the last tile: before any operand load
    const unsigned pair = nb * 4u + wave; // a wave's pair of n-tiles
    if (pair >= pairs)
        return; // (wave-uniform; the loop has no barrier) a ragged last workgroup
    // (m0 + rows_valid <= m: the clamp rule keeps every expert's rows inside [0, m))
    const unsigned m0 = t.row0 + (slot - t.first) * 32u, rows_valid = min(t.row0 + t.rows - m0, 32u);
    const char *const w_base = (const char *)p.w + t.expert * moe_w_bytes<kFmtMx>(p.n, p.k);
    const char *const s_base = (const char *)p.s + t.expert * moe_s_bytes<kFmtMx>(p.n, p.k);
    constexpr int WF = 4;
#include "gemm_native_invariant_split.inc"
}

// The split form on the experts' images (WF = 6): expert e's image starts e * nv6_image_bytes(n, k) into p.w and its scale region follows its own
// elements -- the layout gemm_moe_native.hpp reads; p.s is not read.
template <class AT, int ACT, int kDepth> __global__ __launch_bounds__(256) void native_invariant_moe_nv_split_kernel(const NativeInvariantMoeArgs p) {
    const unsigned lane = threadIdx.x & 63u, m_l = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned pairs = p.n / 32u, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    const unsigned nb = blockIdx.x % p.nblocks, rest = blockIdx.x / p.nblocks;
    const unsigned s = rest % p.slices, slot = rest / p.slices;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 32u, slot, t))
        return; // a slot past the last tile: before any operand load
    const unsigned pair = nb * 4u + wave; // a wave's block of 32 weight rows
    if (pair >= pairs)
        return; // (wave-uniform; the loop has no barrier) a ragged last workgroup
    const unsigned m0 = t.row0 + (slot - t.first) * 32u, rows_valid = min(t.row0 + t.rows - m0, 32u);
    const char *const w_base = (const char *)p.w + t.expert * nv6_image_bytes(p.n, p.k);
    const char *const s_base = w_base + nv6_elem_bytes(p.n, p.k);
    constexpr int WF = 6;
#include "gemm_native_invariant_split.inc"
}

// The whole form: a workgroup on (expert, m-tile of 64, 4 slots of two pairs of n-tiles).
template <class AT, int ACT> __global__ __launch_bounds__(256) void native_invariant_moe_whole_kernel(const NativeInvariantMoeArgs p) {
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned nb = blockIdx.x % p.nblocks, mslot = blockIdx.x / p.nblocks;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 64u, mslot, t))
        return; // (workgroup-uniform: before any barrier and any operand load)
    const unsigned slot = nb * 4u + wave;
    const unsigned m0 = t.row0 + (mslot - t.first) * 64u, rows_valid = min(t.row0 + t.rows - m0, 64u);
    const char *const w_base = (const char *)p.w + t.expert * moe_w_bytes<kFmtMx>(p.n, p.k);
    const char *const s_base = (const char *)p.s + t.expert * moe_s_bytes<kFmtMx>(p.n, p.k);
    const float *const gs = p.gs + t.expert;
    const void *const bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
    auto c_row = [&](unsigned row) { return native_moe_c_row(p, row); };
    constexpr int WF = 4;
#include "gemm_native_invariant_whole.inc"
}

// The whole form on the experts' images (WF = 6).
template <class AT, int ACT> __global__ __launch_bounds__(256) void native_invariant_moe_nv_whole_kernel(const NativeInvariantMoeArgs p) {
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned nb = blockIdx.x % p.nblocks, mslot = blockIdx.x / p.nblocks;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 64u, mslot, t))
        return; // (workgroup-uniform: before any barrier and any operand load)
    const unsigned slot = nb * 4u + wave;
    const unsigned m0 = t.row0 + (mslot - t.first) * 64u, rows_valid = min(t.row0 + t.rows - m0, 64u);
    const char *const w_base = (const char *)p.w + t.expert * nv6_image_bytes(p.n, p.k);
    const char *const s_base = w_base + nv6_elem_bytes(p.n, p.k);
    const float *const gs = p.gs + t.expert;
    const void *const bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
    auto c_row = [&](unsigned row) { return native_moe_c_row(p, row); };
    constexpr int WF = 6;
#include "gemm_native_invariant_whole.inc"
}

// one activation type's launches of one weight operand; instantiated by gemm_native_invariant_moe_{bf16,f16}.hip (WF = 4) and
// gemm_native_invariant_moe_nv_{bf16,f16}.hip (WF = 6).  The grids are the plan's (gemm_invariant_host.h), which refused the call had one of
// them reached 2^31.
template <class AT, int ACT, int WF> void native_invariant_moe_launch_fmt(NativeInvariantMoeArgs p, const invariant::Plan &plan, hipStream_t stream) {
    p.nblocks = plan.gemm.nblocks;
    if (plan.split) {
        if constexpr (WF == 6)
            hipLaunchKernelGGL((native_invariant_moe_nv_split_kernel<AT, ACT, kNativeInvariantSplitDepth>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((native_invariant_moe_split_kernel<AT, ACT, kNativeInvariantSplitDepth>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        // the fold of the exact MoE launch, over its own 16-row slot map of the same offsets
        InvariantMoeArgs f{};
        f.c = p.c, f.gs = p.gs, f.bias = p.bias, f.slabs = p.slabs, f.offsets = p.offsets, f.c_idx = p.c_idx;
        f.m = p.m, f.n = p.n, f.k = p.k, f.slice_k = p.slice_k, f.slices = p.slices, f.act = p.act, f.experts = p.experts, f.c_rows = p.c_rows;
        f.nblocks = plan.fold.nblocks;
        hipLaunchKernelGGL((invariant_moe_fold_kernel<AT>), invariant_grid(plan.fold), dim3(256), 0, stream, f);
    } else {
        if constexpr (WF == 6)
            hipLaunchKernelGGL((native_invariant_moe_nv_whole_kernel<AT, ACT>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((native_invariant_moe_whole_kernel<AT, ACT>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
    }
}
template <class AT, int WF = 4>
void native_invariant_moe_launch(const NativeInvariantMoeArgs &p, int act_format, const invariant::Plan &plan, hipStream_t stream) {
    if (act_format == 8)
        native_invariant_moe_launch_fmt<AT, 8, WF>(p, plan, stream);
    else if (act_format == 6)
        native_invariant_moe_launch_fmt<AT, 6, WF>(p, plan, stream);
    else
        native_invariant_moe_launch_fmt<AT, 4, WF>(p, plan, stream);
}

} // namespace petit_amd
