// gemm_moe.hpp -- routed-expert (MoE) forms of the streaming, decode and tiled kernels: all experts of a layer in ONE launch
// (petit_gemm_fp4_fp16_moe, include/petit_amd.h).
//
// The activation rows arrive grouped by expert: rows offsets[e] .. offsets[e+1]-1 belong to expert e, whose packed weights,
// scales, global scale and bias sit at index e of arrays stacked back to back.  The host never reads the offsets (the call
// is graph-capturable), so the grid is sized for every possible routing: x = the dense kernel's n-blocks, y = m-slots with
//     slots = ceil(m / BM) + min(E, m)   >=   sum over experts of ceil(c_e / BM)       (BM = rows per workgroup)
// and every workgroup maps its slot to (expert, m-block inside the expert) on the device (moe_locate below): the per-expert
// tile counts ceil(c_e / BM), a wave-wide prefix sum over 64 experts at a time, a ballot for the expert whose tile range holds
// the slot.  Slots past the last tile exit before any load, so an expert without rows costs nothing and its weights are
// never read.  The workgroup then runs the dense kernel's body on its expert's operands (64-bit bases); within an expert
// the numerics are those of a dense call on that expert's rows with the same kernel, bit for bit (the m-blocks start at the
// expert's first row, as a dense call's start at row 0).
//
// Robustness: every offset is clamped into [offsets[e-1], m] (offsets[-1] := 0) before use -- a running maximum, then
// min(., m) -- so malformed offsets can only leave rows unwritten, never read or write out of bounds.  The same rule decides which experts
// the NVFP4 image builder skips (moe_expert_rows, petit_internal.h, used by nvnative.hip): moe_locate below and that function are its two
// statements, and must change together.
//
// Indexed forms (petit_gemm_fp4_fp16_moe_ex; the *_idx_kernel templates below, instantiated by the gemm_moe_idx_<family> TUs): grouped
// row r reads A row a_idx[r] and writes C row c_idx[r] (device_common.hpp RowIndex), so the layer needs no gathered copy of the
// activations and no un-permute of the output.  Only addresses change: each workgroup reads its rows' indices once before the K loop
// (A: into the VGPR / SGPR offsets of its loads, against one descriptor over the caller's a_rows x k matrix, so an index outside
// [0, a_rows) reads zeros) and once more in the epilogue (C: an explicit check, an index outside [0, c_rows) stores nothing).  Within an
// expert the numbers are the plain form's, bit for bit.
#pragma once

#include "gemm_decode.hpp"
#include "gemm_stream.hpp"
#include "gemm_tiled.hpp"

namespace petit_amd {

// the slot of a workgroup, resolved: rows [row0, row0 + rows) of A / C are expert `expert`'s; its m-tiles are slots
// [first, first + tiles) of the launch
struct MoeTile {
    unsigned expert, row0, rows, first, tiles;
};

// Wave-uniform: every wave of the workgroup computes the same answer from the same loads (no LDS, no barrier).
__device__ __forceinline__ bool moe_locate(const int *offsets, unsigned num_experts, unsigned m, unsigned bm, unsigned slot, MoeTile &t) {
    const unsigned lane = threadIdx.x & 63u;
    // every load first (one memory latency, not one per 64 experts: a slot past the last tile pays this and exits)
    constexpr unsigned kChunks = kMoeMaxExperts / 64;
    int raw[kChunks];
#pragma unroll
    for (unsigned c = 0; c < kChunks; ++c)
        raw[c] = c * 64 + lane < num_experts ? offsets[c * 64 + lane + 1] : 0;
    unsigned carry_off = min((unsigned)max(offsets[0], 0), m); // clamped offsets[0]
    unsigned carry_tiles = 0;
#pragma unroll
    for (unsigned c = 0; c < kChunks; ++c) {
        const unsigned base = c * 64;
        if (base >= num_experts)
            break;
        const unsigned e = base + lane;
        const bool live = e < num_experts;
        // hi = clamped offsets[e + 1]: running maximum over the chunk and everything before it, then min(., m)
        unsigned hi = live ? min((unsigned)max(raw[c], 0), m) : 0u;
#pragma unroll
        for (unsigned d = 1; d < 64; d *= 2) {
            const unsigned u = __shfl_up(hi, d);
            if (lane >= d)
                hi = max(hi, u);
        }
        hi = max(hi, carry_off);
        unsigned lo = __shfl_up(hi, 1);
        if (lane == 0)
            lo = carry_off;
        const unsigned rows = hi - lo;
        const unsigned tiles = live ? (rows + bm - 1) / bm : 0u;
        unsigned incl = tiles;
#pragma unroll
        for (unsigned d = 1; d < 64; d *= 2) {
            const unsigned u = __shfl_up(incl, d);
            if (lane >= d)
                incl += u;
        }
        incl += carry_tiles;
        const unsigned excl = incl - tiles;
        const unsigned long long hit = __ballot(live && slot >= excl && slot < incl);
        if (hit) {
            const int l = __builtin_ctzll(hit);
            t.expert = __builtin_amdgcn_readfirstlane(base + (unsigned)l);
            t.row0 = __builtin_amdgcn_readfirstlane(__shfl(lo, l));
            t.rows = __builtin_amdgcn_readfirstlane(__shfl(rows, l));
            t.first = __builtin_amdgcn_readfirstlane(__shfl(excl, l));
            t.tiles = __builtin_amdgcn_readfirstlane(__shfl(tiles, l));
            return true;
        }
        carry_off = __builtin_amdgcn_readfirstlane(__shfl(hi, 63));
        carry_tiles = __builtin_amdgcn_readfirstlane(__shfl(incl, 63));
    }
    return false; // a slot past the last tile
}

// bytes of one expert's packed weights / scales
template <int FMT> __device__ __forceinline__ size_t moe_w_bytes(unsigned n, unsigned k) { return (size_t)n * k / 2; }
template <int FMT> __device__ __forceinline__ size_t moe_s_bytes(unsigned n, unsigned k) { return (size_t)n * k / (FMT == kFmtNv ? 16 : 32); }

// Staged streaming kernels (AM rows per workgroup, MT == 1) and the decode kernels (R rows): the m-block's rows are handed
// to the body as a block of its own (block_y = 0), exactly what a dense call on <= BM rows runs.
template <class Cfg>
__global__ __launch_bounds__(Cfg::kThreads) void gemm_stream_moe_kernel(const void *arg_w, const void *arg_s, const void *arg_a, unsigned arg_k,
                                                                        unsigned arg_n, unsigned arg_m, unsigned arg_spw, unsigned arg_act,
                                                                        void *arg_c, const float *arg_gs, const void *arg_bias,
                                                                        const int *arg_offsets, unsigned arg_experts) {
    constexpr unsigned BM = Cfg::AM;
    static_assert(Cfg::AM > 0 && Cfg::MT == 1, "MoE form: the staged streaming kernels");
    MoeTile t;
    if (!moe_locate(arg_offsets, arg_experts, arg_m, BM, blockIdx.y, t))
        return;
    const unsigned r0 = t.row0 + (blockIdx.y - t.first) * BM;
    const unsigned n_out = arg_act ? arg_n / 2 : arg_n;
    gemm_stream_body<Cfg>((const char *)arg_w + t.expert * moe_w_bytes<Cfg::FMT>(arg_n, arg_k),
                          (const char *)arg_s + t.expert * moe_s_bytes<Cfg::FMT>(arg_n, arg_k), (const char *)arg_a + (size_t)r0 * arg_k * 2,
                          arg_k, arg_n, min(t.row0 + t.rows - r0, BM), arg_spw, arg_act, (char *)arg_c + (size_t)r0 * n_out * 2,
                          arg_gs + t.expert, arg_bias ? (const char *)arg_bias + (size_t)t.expert * arg_n * 2 : nullptr, nullptr, blockIdx.x, 0u);
}

template <class Cfg>
__global__ __launch_bounds__(Cfg::kThreads, Cfg::kWavesPerSimd) void gemm_decode_moe_kernel(const void *arg_w, const void *arg_s, const void *arg_a,
                                                                                            unsigned arg_k, unsigned arg_n, unsigned arg_m,
                                                                                            unsigned arg_spw, unsigned arg_act, void *arg_c,
                                                                                            const float *arg_gs, const void *arg_bias,
                                                                                            const int *arg_offsets, unsigned arg_experts) {
    constexpr unsigned BM = Cfg::R;
    MoeTile t;
    if (!moe_locate(arg_offsets, arg_experts, arg_m, BM, blockIdx.y, t))
        return;
    const unsigned r0 = t.row0 + (blockIdx.y - t.first) * BM;
    const unsigned n_out = arg_act ? arg_n / 2 : arg_n;
    gemm_decode_body<Cfg>((const char *)arg_w + t.expert * moe_w_bytes<kFmtNv>(arg_n, arg_k),
                          (const char *)arg_s + t.expert * moe_s_bytes<kFmtNv>(arg_n, arg_k), (const char *)arg_a + (size_t)r0 * arg_k * 2,
                          arg_k, arg_n, min(t.row0 + t.rows - r0, BM), arg_spw, arg_act, (char *)arg_c + (size_t)r0 * n_out * 2,
                          arg_gs + t.expert, arg_bias ? (const char *)arg_bias + (size_t)t.expert * arg_n * 2 : nullptr, blockIdx.x);
}

// Tiled kernel: plain raster order over the linear workgroup index L = y * gridDim.x + x.  Expert e owns L in
// [first_e * nb, (first_e + tiles_e) * nb) (nb = gridDim.x n-blocks), walked with its m-blocks fastest so that the W panel of
// an n-block is reused from L2 by all of the expert's m-blocks.  p: the call's arguments with the stacked bases; p.m = total rows.
template <class Cfg>
__global__ __launch_bounds__(Cfg::kThreads, Cfg::kMinWavesPerSimd) void gemm_tiled_moe_kernel(const GemmArgs p, const int *arg_offsets,
                                                                                                unsigned arg_experts) {
    const unsigned nb = gridDim.x;
    const unsigned lin = blockIdx.y * nb + blockIdx.x;
    MoeTile t;
    if (!moe_locate(arg_offsets, arg_experts, p.m, Cfg::BM, lin / nb, t))
        return;
    const unsigned local = lin - t.first * nb;
    GemmArgs q = p;
    const unsigned n_out = p.act ? p.n / 2 : p.n;
    q.w = (const char *)p.w + t.expert * moe_w_bytes<Cfg::FMT>(p.n, p.k);
    q.s = (const char *)p.s + t.expert * moe_s_bytes<Cfg::FMT>(p.n, p.k);
    q.a = (const char *)p.a + (size_t)t.row0 * p.k * 2;
    q.c = (char *)p.c + (size_t)t.row0 * n_out * 2;
    q.gs = p.gs + t.expert;
    q.bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
    q.m = t.rows;
    gemm_tiled_body<Cfg>(q, local / t.tiles, local % t.tiles);
}

// --- indexed forms: the same kernels on gathered A rows and scattered C rows (A and C are the caller's whole matrices) ----------------
template <class Cfg>
__global__ __launch_bounds__(Cfg::kThreads) void gemm_stream_moe_idx_kernel(const void *arg_w, const void *arg_s, const void *arg_a, unsigned arg_k,
                                                                            unsigned arg_n, unsigned arg_m, unsigned arg_spw, unsigned arg_act,
                                                                            void *arg_c, const float *arg_gs, const void *arg_bias,
                                                                            const int *arg_offsets, unsigned arg_experts, RowIndex ix) {
    constexpr unsigned BM = Cfg::AM;
    static_assert(Cfg::AM > 0 && Cfg::MT == 1, "MoE form: the staged streaming kernels");
    MoeTile t;
    if (!moe_locate(arg_offsets, arg_experts, arg_m, BM, blockIdx.y, t))
        return;
    const unsigned r0 = t.row0 + (blockIdx.y - t.first) * BM;
    ix.row0 = r0;
    gemm_stream_body<Cfg, false, true>((const char *)arg_w + t.expert * moe_w_bytes<Cfg::FMT>(arg_n, arg_k),
                                       (const char *)arg_s + t.expert * moe_s_bytes<Cfg::FMT>(arg_n, arg_k), arg_a, arg_k, arg_n,
                                       min(t.row0 + t.rows - r0, BM), arg_spw, arg_act, arg_c, arg_gs + t.expert,
                                       arg_bias ? (const char *)arg_bias + (size_t)t.expert * arg_n * 2 : nullptr, nullptr, blockIdx.x, 0u, nullptr, ix);
}

template <class Cfg>
__global__ __launch_bounds__(Cfg::kThreads, Cfg::kWavesPerSimd) void gemm_decode_moe_idx_kernel(const void *arg_w, const void *arg_s,
                                                                                                const void *arg_a, unsigned arg_k, unsigned arg_n,
                                                                                                unsigned arg_m, unsigned arg_spw, unsigned arg_act,
                                                                                                void *arg_c, const float *arg_gs,
                                                                                                const void *arg_bias, const int *arg_offsets,
                                                                                                unsigned arg_experts, RowIndex ix) {
    constexpr unsigned BM = Cfg::R;
    MoeTile t;
    if (!moe_locate(arg_offsets, arg_experts, arg_m, BM, blockIdx.y, t))
        return;
    const unsigned r0 = t.row0 + (blockIdx.y - t.first) * BM;
    ix.row0 = r0;
    gemm_decode_body<Cfg, true>((const char *)arg_w + t.expert * moe_w_bytes<kFmtNv>(arg_n, arg_k),
                                (const char *)arg_s + t.expert * moe_s_bytes<kFmtNv>(arg_n, arg_k), arg_a, arg_k, arg_n, min(t.row0 + t.rows - r0, BM),
                                arg_spw, arg_act, arg_c, arg_gs + t.expert,
                                arg_bias ? (const char *)arg_bias + (size_t)t.expert * arg_n * 2 : nullptr, blockIdx.x, ix);
}

template <class Cfg>
__global__ __launch_bounds__(Cfg::kThreads, Cfg::kMinWavesPerSimd) void gemm_tiled_moe_idx_kernel(const GemmArgs p, const int *arg_offsets,
                                                                                                    unsigned arg_experts, RowIndex ix) {
    const unsigned nb = gridDim.x;
    const unsigned lin = blockIdx.y * nb + blockIdx.x;
    MoeTile t;
    if (!moe_locate(arg_offsets, arg_experts, p.m, Cfg::BM, lin / nb, t))
        return;
    const unsigned local = lin - t.first * nb;
    GemmArgs q = p;
    q.w = (const char *)p.w + t.expert * moe_w_bytes<Cfg::FMT>(p.n, p.k);
    q.s = (const char *)p.s + t.expert * moe_s_bytes<Cfg::FMT>(p.n, p.k);
    q.gs = p.gs + t.expert;
    q.bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
    q.m = t.rows;
    ix.row0 = t.row0;
    gemm_tiled_body<Cfg, true>(q, local / t.tiles, local % t.tiles, ix);
}

} // namespace petit_amd
