// gemm_invariant_moe.hpp -- the batch-invariant routed-expert (MoE) GEMM (include/petit_amd.h "Batch-invariant MoE launch"): grouped row r of
// expert e gets, bit for bit, row 0 of the dense batch-invariant call (gemm_invariant.hpp) on A row a_idx[r] and expert e's tensors.
//
// The arithmetic is gemm_invariant.hpp's, statement for statement: S slices of L (invariant_geometry: a function of (n, k, types) alone), one
// v_mfma_f32_16x16x32 chain per slice from zero, k-tiles ascending, the weight dequantised with its group scale before the MFMA, the slices
// added in ascending order, then * gs[e] + bias[e] and one rounding.  The addressing is gemm_moe.hpp's: a launch sized for every possible
// routing, slot -> (expert, m-tile) by moe_locate on the device (the clamp rule), gathered A rows and scattered C rows (RowIndex's rules).
// The kernels are separate from the dense ones, which this header does not touch: they compile to the code they had.
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

// The split form: gemm_invariant_split_kernel's wave on (expert, m-tile of 16, slice, n-tile).
template <class AT, int FMT, int kDepth> __global__ __launch_bounds__(256) void gemm_invariant_moe_split_kernel(const InvariantMoeArgs p) {
#pragma clang fp contract(off)
    using Frag = typename AT::frag;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned ntiles = p.n / kTileN, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    constexpr unsigned kRec = FMT == kFmtNv ? 2u : 1u; // scale bytes per lane and k-tile

    // the linear index: n-block fastest, then the slice, then the slot
    const unsigned nb = blockIdx.x % p.nblocks, rest = blockIdx.x / p.nblocks;
    const unsigned s_lo = rest % p.slices, slot = rest / p.slices;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 16u, slot, t))
        return; // a slot past the last tile: before any operand load
    const unsigned tile = nb * 4u + wave;
    const bool live = tile < ntiles; // (wave-uniform) a ragged last n-block: empty descriptors, nothing stored
    const unsigned m0 = t.row0 + (slot - t.first) * 16u, rows_valid = min(t.row0 + t.rows - m0, 16u);

    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.a, p.a_rows * p.k * 2);
    const char *w_base = (const char *)p.w + t.expert * moe_w_bytes<FMT>(p.n, p.k);
    const char *s_base = (const char *)p.s + t.expert * moe_s_bytes<FMT>(p.n, p.k);
    const unsigned wt = live ? tile : 0u;
    const __amdgpu_buffer_rsrc_t w_rsrc = make_rsrc(w_base + (size_t)wt * ktiles * kTileBytes, live ? ktiles * kTileBytes : 0u);
    const __amdgpu_buffer_rsrc_t s_rsrc = make_rsrc(s_base + (size_t)wt * ktiles * (64 * kRec), live ? ktiles * (64 * kRec) : 0u);
    // row (lane & 15) of the m-tile, 32 consecutive k
    const unsigned a_voff = invariant_moe_a_off(p, m0 + (lane & 15u), (lane & 15u) < rows_valid) + (lane >> 4) * (kLaneK * 2);

    struct Stage {
        u32x4 w;
        unsigned sc;
        u32x4 a[4];
    };
    auto load_stage = [&](Stage &st, unsigned kt) {
        const unsigned sp = kt / ks, tt = kt - sp * ks;
        const unsigned s_voff = ((sp * 64u + lane) * ks + tt) * kRec;
        st.w = buf_load16(w_rsrc, kt * kTileBytes + lane * 16u, 0, kAuxNt);
        if constexpr (FMT == kFmtNv)
            st.sc = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(s_rsrc, s_voff, 0, kAuxNt);
        else
            st.sc = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc, s_voff, 0, kAuxNt);
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4)
            st.a[j4] = buf_load16(a_rsrc, a_voff + kt * (kTileK * 2) + j4 * 16u, 0, kAuxDefault);
    };

    const unsigned kt0 = s_lo * (p.slice_k / kTileK);
    const unsigned kt_end = (s_lo + 1) * (p.slice_k / kTileK), kt1 = kt_end < ktiles ? kt_end : ktiles;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    // the ring: stage d holds k-tile kt + d; a load past the slice's end repeats its last tile and is never used
    Stage ring[kDepth];
#pragma unroll
    for (int d = 0; d < kDepth; ++d)
        load_stage(ring[d], kt0 + d < kt1 ? kt0 + d : kt1 - 1);
    for (unsigned kt = kt0; kt < kt1; ++kt) {
        const Stage cur = ring[0];
#pragma unroll
        for (int d = 0; d + 1 < kDepth; ++d)
            ring[d] = ring[d + 1];
        load_stage(ring[kDepth - 1], kt + kDepth < kt1 ? kt + kDepth : kt1 - 1);
        Frag wf[4];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            const unsigned word = cur.w[j4];
            if constexpr (FMT == kFmtNv)
                wf[j4] = unpack_nv(AT{}, word, j4 < 2 ? e4m3_byte<0>(cur.sc) : e4m3_byte<1>(cur.sc));
            else
                wf[j4] = unpack_mx(AT{}, word, e8m0_byte<0>(cur.sc));
        }
        // the chain: k-tiles ascending, the tile's words in order
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4)
            acc = mfma16(wf[j4], __builtin_bit_cast(Frag, cur.a[j4]), acc);
    }
    // the accumulator leaves the loop's basic block: see mfma_join_pin (device_common.hpp)
    mfma_join_pin(acc);
    mfma_join_settle();
    mfma_join_pin(acc);
    if (!live)
        return;
    // a lane holds 4 consecutive n (4 (lane >> 4) + i) of row (lane & 15) of the tile
    if ((lane & 15u) < rows_valid) {
        const unsigned row = m0 + (lane & 15u); // < m: the clamp rule keeps every expert's rows inside [0, m)
        float *out = p.slabs + ((size_t)s_lo * p.m + row) * p.n + tile * 16u + (lane >> 4) * 4u;
        *reinterpret_cast<f32x4 *>(out) = acc;
    }
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

// The whole form: gemm_invariant_whole_kernel's workgroup on (expert, m-tile of 64, n-block of 8 tiles), the activation tile gathered.
template <class AT, int FMT> __global__ __launch_bounds__(256) void gemm_invariant_moe_whole_kernel(const InvariantMoeArgs p) {
#pragma clang fp contract(off)
    using Frag = typename AT::frag;
    constexpr int MT = 4, NT = 2;
    __shared__ __attribute__((aligned(16))) char lds[2 * kWholeBufBytes];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned ntiles = p.n / kTileN, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    constexpr unsigned kRec = FMT == kFmtNv ? 2u : 1u;
    const bool gated = p.act != 0;
    const unsigned nb = blockIdx.x % p.nblocks, mslot = blockIdx.x / p.nblocks;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 64u, mslot, t))
        return; // (workgroup-uniform: before any barrier and any operand load)
    const unsigned slot = nb * 4u + wave;
    unsigned tile[NT];
    bool live[NT]; // (wave-uniform) tiles past N: empty descriptors, nothing stored.  Dead waves still walk the loop: they share the barriers.
    tile[0] = gated ? slot : 2u * slot, tile[1] = gated ? slot + ntiles / 2 : 2u * slot + 1;
    live[0] = gated ? slot < ntiles / 2 : tile[0] < ntiles, live[1] = gated ? live[0] : tile[1] < ntiles;
    const unsigned m0 = t.row0 + (mslot - t.first) * 64u, rows_valid = min(t.row0 + t.rows - m0, 64u);
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.a, p.a_rows * p.k * 2);
    const char *w_base = (const char *)p.w + t.expert * moe_w_bytes<FMT>(p.n, p.k);
    const char *s_base = (const char *)p.s + t.expert * moe_s_bytes<FMT>(p.n, p.k);
    __amdgpu_buffer_rsrc_t w_rsrc[NT], s_rsrc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const unsigned tt = live[j] ? tile[j] : 0u;
        w_rsrc[j] = make_rsrc(w_base + (size_t)tt * ktiles * kTileBytes, live[j] ? ktiles * kTileBytes : 0u);
        s_rsrc[j] = make_rsrc(s_base + (size_t)tt * ktiles * (64 * kRec), live[j] ? ktiles * (64 * kRec) : 0u);
    }
    // staging: 16-byte unit u = tid + 256 i of the tile is row u / 16, bytes 16 (u % 16) of the row's 256; the four rows' indices are read here, once
    unsigned st_voff[4], st_lds[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned u = tid + 256u * i, row = u >> 4, cu = u & 15u;
        st_voff[i] = invariant_moe_a_off(p, m0 + row, row < rows_valid) + cu * 16u, st_lds[i] = row * kWholeRowBytes + cu * 16u;
    }
    auto fetch_a = [&](u32x4 (&r)[4], unsigned kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            r[i] = buf_load16(a_rsrc, st_voff[i] + kt * (kTileK * 2), 0, kAuxDefault);
    };
    auto put_a = [&](const u32x4 (&r)[4], unsigned buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<u32x4 *>(lds + buf * kWholeBufBytes + st_lds[i]) = r[i];
    };
    struct WStage {
        u32x4 w[NT];
        unsigned sc[NT];
    };
    auto load_w = [&](WStage &st, unsigned kt) {
        const unsigned sp = kt / ks, tt = kt - sp * ks;
        const unsigned s_voff = ((sp * 64u + lane) * ks + tt) * kRec;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            st.w[j] = buf_load16(w_rsrc[j], kt * kTileBytes + lane * 16u, 0, kAuxDefault);
            if constexpr (FMT == kFmtNv)
                st.sc[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(s_rsrc[j], s_voff, 0, kAuxDefault);
            else
                st.sc[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[j], s_voff, 0, kAuxDefault);
        }
    };
    // this lane's fragment of m-tile mt, word j4: row 16 mt + (lane & 15), k = 32 (lane >> 4) + 8 j4 .. + 7
    const unsigned frag_off = (lane & 15u) * kWholeRowBytes + (lane >> 4) * (kLaneK * 2);

    f32x4 total[MT][NT], acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < NT; ++j)
            acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f}, total[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto join = [&](bool first) { // a slice is done: the accumulators leave the loop's MFMA block (mfma_join_pin, device_common.hpp)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                mfma_join_pin(acc[mt][j]);
        mfma_join_settle();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                mfma_join_pin(acc[mt][j]);
                total[mt][j] = first ? acc[mt][j] : total[mt][j] + acc[mt][j];
                acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
    };

    WStage ring[kWholeRing];
#pragma unroll
    for (int d = 0; d < kWholeRing; ++d)
        load_w(ring[d], (unsigned)d < ktiles ? d : ktiles - 1);
    {
        u32x4 r[4];
        fetch_a(r, 0);
        put_a(r, 0);
    }
    __syncthreads();
    const unsigned slice_tiles = p.slice_k / kTileK;
    unsigned boundary = slice_tiles; // the k-tile that opens the next slice
    for (unsigned kt = 0; kt < ktiles; ++kt) {
        if (kt == boundary) {
            join(boundary == slice_tiles);
            boundary += slice_tiles;
        }
        u32x4 nxt[4];
        fetch_a(nxt, kt + 1 < ktiles ? kt + 1 : kt);
        const WStage cur = ring[0];
#pragma unroll
        for (int d = 0; d + 1 < kWholeRing; ++d)
            ring[d] = ring[d + 1];
        load_w(ring[kWholeRing - 1], kt + kWholeRing < ktiles ? kt + kWholeRing : ktiles - 1);
        Frag wf[NT][4];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const unsigned sc = cur.sc[j];
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4) {
                const unsigned word = cur.w[j][j4];
                if constexpr (FMT == kFmtNv)
                    wf[j][j4] = unpack_nv(AT{}, word, j4 < 2 ? e4m3_byte<0>(sc) : e4m3_byte<1>(sc));
                else
                    wf[j][j4] = unpack_mx(AT{}, word, e8m0_byte<0>(sc));
            }
        }
        const char *img = lds + (kt & 1u) * kWholeBufBytes + frag_off;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            u32x4 af[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                af[mt] = *reinterpret_cast<const u32x4 *>(img + mt * 16 * kWholeRowBytes + j4 * 16);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[mt][j] = mfma16(wf[j][j4], __builtin_bit_cast(Frag, af[mt]), acc[mt][j]);
        }
        put_a(nxt, (kt + 1u) & 1u); // the other half: everybody left it at the barrier that ended the previous step
        __syncthreads();
    }
    join(boundary == slice_tiles);

    const unsigned nq = (lane >> 4) * 4u;
    const float *gs = p.gs + t.expert;
    const void *bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const unsigned local = mt * 16u + (lane & 15u);
        if (local >= rows_valid) // rows past the expert's end
            continue;
        const unsigned cm = invariant_moe_c_row(p, m0 + local);
        if (cm == ~0u)
            continue;
        if (gated) {
            if (live[0]) {
                const unsigned n_half = p.n / 2, n = slot * 16u + nq;
                *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)cm * n_half + n) * 2) =
                    finish4_silu_mul<AT>(total[mt][0], total[mt][1], *gs, bias, n, n_half, p.act);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (live[j]) {
                    const unsigned n = tile[j] * 16u + nq;
                    *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)cm * p.n + n) * 2) = invariant_finish4<AT>(total[mt][j], gs, bias, n);
                }
        }
    }
}

// one (format, type) pair's launches; instantiated by gemm_invariant_moe_*.hip.  The grids were bounded by the host (moe_grid, gemm_invariant_host.h).
template <class AT, int FMT> void invariant_moe_launch(InvariantMoeArgs p, bool split, hipStream_t stream) {
    const unsigned ntiles = p.n / kTileN, active = p.experts < p.m ? p.experts : p.m;
    if (split) {
        const unsigned slots = (p.m + 15) / 16 + active;
        p.nblocks = (ntiles + 3) / 4;
        hipLaunchKernelGGL((gemm_invariant_moe_split_kernel<AT, FMT, kInvariantSplitDepth>), dim3(slots * p.slices * p.nblocks), dim3(256), 0, stream, p);
        const unsigned n_out = p.act ? p.n / 2 : p.n;
        p.nblocks = (16u * (n_out / 4) + 1023) / 1024; // a thread folds at most 4 units of its m-tile
        hipLaunchKernelGGL((invariant_moe_fold_kernel<AT>), dim3(slots * p.nblocks), dim3(256), 0, stream, p);
    } else {
        const unsigned slots = (p.m + 63) / 64 + active;
        const unsigned pairs = p.act ? ntiles / 2 : (ntiles + 1) / 2;
        p.nblocks = (pairs + 3) / 4;
        hipLaunchKernelGGL((gemm_invariant_moe_whole_kernel<AT, FMT>), dim3(slots * p.nblocks), dim3(256), 0, stream, p);
    }
}

} // namespace petit_amd
