// gemm_invariant_moe.hpp -- the batch-invariant routed-expert (MoE) GEMM (include/petit_amd.h "Batch-invariant MoE launch"): grouped row r of
// expert e gets, bit for bit, row 0 of the dense batch-invariant call (gemm_invariant.hpp) on A row a_idx[r] and expert e's tensors.
//
// The chain is shared with the dense kernels: both forms include the dense kernels' bodies (gemm_invariant_split.inc,
// gemm_invariant_whole.inc) on expert e's tensors, gs[e] and bias[e].  What is this header's is the addressing, which is gemm_moe.hpp's: a launch
// sized for every possible routing, slot -> (expert, m-tile) by moe_locate on the device (the clamp rule), gathered A rows and scattered C
// rows (RowIndex's rules).
//
// Every form uses ONE linear workgroup index in grid x (y / z stop at 65535; m goes to 2^20): index = slot x (slices x n-blocks) + ...
//   split: slots = ceil(m / 16) + min(E, m).  A wave owns one 16 x 16 tile of one slice of one expert's m-tile and stores it to slab s of
//     [S][m][n] fp32, indexed by GROUPED row.  invariant_moe_fold_kernel walks the same slot map, so it knows each row's expert without a
//     per-row table and never visits a row of no expert: nothing in the workspace needs clearing.
//   whole: slots = ceil(m / 64) + min(E, m).  The workgroup stages the gathered 64 x 128 activation tile through LDS, walks all slices with
//     one join per slice, applies the epilogue and scatters C.  No workspace.
// Activations go through one descriptor over the caller's a_rows x k matrix (the host refuses a_rows * k * 2 > 2^31); a lane whose row lies
// past the expert's end, or whose index is outside the matrix, carries voffset 2^31 (kIdxOob) and reads zeros.
#pragma once

#include "gemm_invariant.hpp"
#include "gemm_moe.hpp"

namespace petit_amd {

struct InvariantMoeArgs {
    void *c;           // [c_rows][n] (gated: [c_rows][n/2]) 16-bit
    const void *a;     // [a_rows][k] 16-bit
    const void *w;     // the experts' packed weights, back to back
    const void *s;     // the experts' packed scales, back to back
    const float *gs;   // [E]
    const void *bias;  // [E][n] in c's type, or null
    float *slabs;      // split form: [slices][m][n] fp32
    const int *offsets; // [E + 1], device
    const int *a_idx, *c_idx; // [m] or null: the identity
    unsigned m, n, k;
    unsigned slice_k, slices; // L, S
    unsigned act;             // PETIT_ACTIVATION_*
    unsigned experts, a_rows, c_rows;
    unsigned nblocks;         // n-blocks of the GEMM launch (the fold: column chunks per slot)
};

// byte offset of grouped row `row`'s A row, or kIdxOob: rows past the tile's valid rows read no index
__device__ __forceinline__ unsigned invariant_moe_a_off(const InvariantMoeArgs &p, unsigned row, bool valid) {
    if (!valid)
        return kIdxOob;
    const unsigned a = p.a_idx ? (unsigned)p.a_idx[row] : row;
    return a < p.a_rows ? a * p.k * 2 : kIdxOob;
}
// C row of grouped row `row`, or ~0u: the store is skipped
__device__ __forceinline__ unsigned invariant_moe_c_row(const InvariantMoeArgs &p, unsigned row) {
    const unsigned c = p.c_idx ? (unsigned)p.c_idx[row] : row;
    return c < p.c_rows ? c : ~0u;
}

// The split form: a wave on (expert, m-tile of 16, slice, n-tile).
template <class AT, int FMT, int kDepth> __global__ __launch_bounds__(256) void gemm_invariant_moe_split_kernel(const InvariantMoeArgs p) {
#pragma clang fp contract(off)
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the linear index: n-block fastest, then the slice, then the slot
    const unsigned nb = blockIdx.x % p.nblocks, rest = blockIdx.x / p.nblocks;
    const unsigned s = rest % p.slices, slot = rest / p.slices;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 16u, slot, t))
        return; // a slot past the last tile: before any operand load
    const unsigned tile = nb * 4u + wave;
    const bool live = tile < p.n / kTileN;
    // (m0 + rows_valid <= m: the clamp rule keeps every expert's rows inside [0, m))
    const unsigned m0 = t.row0 + (slot - t.first) * 16u, rows_valid = min(t.row0 + t.rows - m0, 16u);
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.a, p.a_rows * p.k * 2);
    const char *const w_base = (const char *)p.w + t.expert * moe_w_bytes<FMT>(p.n, p.k);
    const char *const s_base = (const char *)p.s + t.expert * moe_s_bytes<FMT>(p.n, p.k);
    const unsigned a_voff = invariant_moe_a_off(p, m0 + (lane & 15u), (lane & 15u) < rows_valid) + (lane >> 4) * (kLaneK * 2);
#include "gemm_invariant_split.inc"
}

// The split form's second launch, over the same slot map: a workgroup takes a column chunk of one (expert, m-tile of 16); a thread adds the
// slabs of 4 consecutive output columns of one row in ascending order and applies gs[e], bias[e] and the activation with the single rounding.
template <class AT> __global__ __launch_bounds__(256) void invariant_moe_fold_kernel(const InvariantMoeArgs p) {
#pragma clang fp contract(off)
    const unsigned chunk = blockIdx.x % p.nblocks, slot = blockIdx.x / p.nblocks;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 16u, slot, t))
        return;
    const unsigned m0 = t.row0 + (slot - t.first) * 16u, rows_valid = min(t.row0 + t.rows - m0, 16u);
    const unsigned n_out = p.act ? p.n / 2 : p.n, per_row = n_out / 4;
    const size_t slab = (size_t)p.m * p.n;
    const float *gs = p.gs + t.expert;
    const void *bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
    for (unsigned u = chunk * 256u + threadIdx.x; u < rows_valid * per_row; u += p.nblocks * 256u) {
        const unsigned row = m0 + u / per_row, n = (u % per_row) * 4u;
        const unsigned cm = invariant_moe_c_row(p, row);
        if (cm == ~0u)
            continue;
        auto fold = [&](unsigned col) {
            const float *src = p.slabs + (size_t)row * p.n + col;
            f32x4 v = *reinterpret_cast<const f32x4 *>(src);
            for (unsigned s = 1; s < p.slices; ++s)
                v = v + *reinterpret_cast<const f32x4 *>(src + s * slab);
            return v;
        };
        uint2 o;
        if (p.act)
            o = finish4_silu_mul<AT>(fold(n), fold(n + n_out), *gs, bias, n, n_out, p.act);
        else
            o = invariant_finish4<AT>(fold(n), gs, bias, n);
        *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)cm * n_out + n) * 2) = o;
    }
}

// The whole form: a workgroup on (expert, m-tile of 64, n-block of 8 tiles), the activation tile gathered.
template <class AT, int FMT> __global__ __launch_bounds__(256) void gemm_invariant_moe_whole_kernel(const InvariantMoeArgs p) {
#pragma clang fp contract(off)
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned nb = blockIdx.x % p.nblocks, mslot = blockIdx.x / p.nblocks;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 64u, mslot, t))
        return; // (workgroup-uniform: before any barrier and any operand load)
    const unsigned slot = nb * 4u + wave;
    const unsigned m0 = t.row0 + (mslot - t.first) * 64u, rows_valid = min(t.row0 + t.rows - m0, 64u);
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.a, p.a_rows * p.k * 2);
    auto a_row_off = [&](unsigned row) { return invariant_moe_a_off(p, m0 + row, row < rows_valid); }; // (each row's index is read once)
    const char *const w_base = (const char *)p.w + t.expert * moe_w_bytes<FMT>(p.n, p.k);
    const char *const s_base = (const char *)p.s + t.expert * moe_s_bytes<FMT>(p.n, p.k);
    const float *const gs = p.gs + t.expert;
    const void *const bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
    auto c_row = [&](unsigned row) { return invariant_moe_c_row(p, row); };
#include "gemm_invariant_whole.inc"
}

// one (format, type) pair's launches; instantiated by gemm_invariant_moe_*.hip.  The grids are the plan's (gemm_invariant_host.h), which refused
// the call had one of them reached 2^31.
template <class AT, int FMT> void invariant_moe_launch(InvariantMoeArgs p, const invariant::Plan &plan, hipStream_t stream) {
    p.nblocks = plan.gemm.nblocks;
    if (plan.split) {
        hipLaunchKernelGGL((gemm_invariant_moe_split_kernel<AT, FMT, kInvariantSplitDepth>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
        p.nblocks = plan.fold.nblocks;
        hipLaunchKernelGGL((invariant_moe_fold_kernel<AT>), invariant_grid(plan.fold), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL((gemm_invariant_moe_whole_kernel<AT, FMT>), invariant_grid(plan.gemm), dim3(256), 0, stream, p);
    }
}

} // namespace petit_amd
