// gemm_native_invariant_moe.hpp -- the batch-invariant routed-expert (MoE) GEMM on the native class (include/petit_amd.h "Batch-invariant MoE
// launch on the native class"): grouped row r of expert e gets, bit for bit, row 0 of the dense native-invariant call
// (gemm_native_invariant.hpp) on that row's quantised bytes and expert e's tensors.
//
// The arithmetic is gemm_native_invariant.hpp's, statement for statement, through its own device functions (native_inv_ktile,
// native_inv_merge, native_inv_aop): S slices of L (invariant_geometry: a function of (n, k) alone), one v_mfma_scale_f32_32x32x64_f8f6f4 chain
// per slice from zero, k-tiles of 128 ascending, P1 then P2, the slices added ascending in fp32, then invariant_finish4 / finish4_silu_mul with
// gs[e] and bias + e * n.  The addressing is gemm_invariant_moe.hpp's: a launch sized for every possible routing, ONE linear workgroup index in
// grid x, slot -> (expert, m-tile) by moe_locate on the device (the clamp rule), scattered C rows.  The dense kernels and the exact MoE kernels
// are not touched: they compile to the code they had.
//
// The quantised activations are the image of the m GROUPED rows, k-tile-major (row r of k-tile kt at (kt * m + r) * row_bytes), so a tile's rows
// are one contiguous run as in the dense kernels: its descriptor starts at the tile's first grouped row and ends with the tile's last valid row
// of this expert -- rows of the next expert, or past m, read zeros.
//   split: slots = ceil(m / 32) + min(E, m).  A wave owns (slot, slice, pair of n-tiles), runs the dense split body (register ring, no LDS, no
//     barrier, non-temporal weight loads) and stores its fp32 tile to slab s of [S][m][n], indexed by GROUPED row, rows below rows_valid only.
//     The second launch is invariant_moe_fold_kernel (gemm_invariant_moe.hpp) as it stands: it walks its own 16-row slot map over the same
//     offsets, so slabs indexed by grouped row are all it needs, and nothing in the workspace needs clearing.
//   whole: slots = ceil(m / 64) + min(E, m).  The dense whole body on the slot's expert: LDS-staged activation tile, double-buffered, one
//     barrier per k-tile, the unit swizzle, two m-blocks x two pairs per wave, one join per slice; the epilogue in the launch, C scattered.
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

// The split form: native_invariant_split_kernel's wave on (expert, m-tile of 32, slice, pair of n-tiles).
template <class AT, int ACT, int kDepth> __global__ __launch_bounds__(256) void native_invariant_moe_split_kernel(const NativeInvariantMoeArgs p) {
    constexpr unsigned kRowB = native_inv_row_bytes<ACT>();
    constexpr int NA = native_inv_frag_units<ACT>();
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
    const unsigned m0 = t.row0 + (slot - t.first) * 32u, rows_valid = min(t.row0 + t.rows - m0, 32u);

    const char *const w_base = (const char *)p.w + t.expert * moe_w_bytes<kFmtMx>(p.n, p.k);
    const char *const s_base = (const char *)p.s + t.expert * moe_s_bytes<kFmtMx>(p.n, p.k);
    __amdgpu_buffer_rsrc_t w_rsrc[2], s_rsrc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned tile = 2u * pair + j;
        w_rsrc[j] = make_rsrc(w_base + (size_t)tile * ktiles * kTileBytes, ktiles * kTileBytes);
        s_rsrc[j] = make_rsrc(s_base + (size_t)tile * ktiles * 64, ktiles * 64);
    }
    const unsigned char *const qa_hi = p.qa + (size_t)p.m * (p.k / 2); // (MXFP6)
    const unsigned char *const qs = p.qa + (size_t)p.m * (p.k / 8 * ACT);
    const unsigned a_voff = m_l * kRowB + h * (ACT == 8 ? 32u : 16u);

    struct Stage {
        u32x4 w[2];
        unsigned sc[2];
        u32x4 a[NA];
        unsigned asc;
    };
    auto load_stage = [&](Stage &st, unsigned kt) {
        const unsigned sp = kt / ks, tt = kt - sp * ks;
        const unsigned s_voff = (sp * 64u + lane) * ks + tt;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            st.w[j] = buf_load16(w_rsrc[j], kt * kTileBytes + lane * 16u, 0, kAuxNt);
            st.sc[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[j], s_voff, 0, kAuxNt);
        }
        // the k-tile's grouped rows m0 .. m0 + rows_valid - 1 of every image: rows past the expert's end are out of range -> zeros
        const size_t tile_row = (size_t)kt * p.m + m0;
        const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.qa + tile_row * kRowB, rows_valid * kRowB);
        const __amdgpu_buffer_rsrc_t q_rsrc = make_rsrc(qs + tile_row * 4, rows_valid * 4u);
        if constexpr (ACT == 8) {
            st.a[0] = buf_load16(a_rsrc, a_voff, 0, kAuxDefault), st.a[1] = buf_load16(a_rsrc, a_voff + 16u, 0, kAuxDefault);
            st.a[2] = buf_load16(a_rsrc, a_voff + 64u, 0, kAuxDefault), st.a[3] = buf_load16(a_rsrc, a_voff + 80u, 0, kAuxDefault);
        } else {
            st.a[0] = buf_load16(a_rsrc, a_voff, 0, kAuxDefault), st.a[1] = buf_load16(a_rsrc, a_voff + 32u, 0, kAuxDefault);
            if constexpr (ACT == 6) {
                const __amdgpu_buffer_rsrc_t h_rsrc = make_rsrc(qa_hi + tile_row * 32, rows_valid * 32u);
                st.a[2] = buf_load16(h_rsrc, m_l * 32u + h * 16u, 0, kAuxDefault);
            }
        }
        st.asc = __builtin_amdgcn_raw_buffer_load_b32(q_rsrc, m_l * 4u, 0, kAuxDefault);
    };

    const unsigned kt0 = s * (p.slice_k / kTileK);
    const unsigned kt_end = (s + 1) * (p.slice_k / kTileK), kt1 = kt_end < ktiles ? kt_end : ktiles;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v)
        acc[v] = 0.f;
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
        i32x8 wop[2];
        unsigned wsc[2];
        native_inv_merge(cur.w[0], cur.w[1], cur.sc[0], cur.sc[1], wop, wsc);
        // this lane's block is 2 q + h of the k-tile's four
        acc = native_inv_ktile<ACT>(acc, wop, wsc, cur.a, (cur.asc >> (8u * h)) & 0xffu, (cur.asc >> (16u + 8u * h)) & 0xffu);
    }
    // the accumulator leaves the loop's basic block (mfma_join_pin, device_common.hpp), and every MFMA executes with all 64 lanes before the
    // lane-divergent stores (pin_acc, gemm_native.hpp)
    mfma_join_pin(acc);
    mfma_join_settle();
    mfma_join_pin(acc);

    // lane (m_l, h) holds row m_l of the tile; register 4 u + i is column 16 (u >> 1) + 8 (u & 1) + 4 h + i of the pair's 32
    if (m_l >= rows_valid)
        return;
    const unsigned row = m0 + m_l; // < m: the clamp rule keeps every expert's rows inside [0, m)
    float *const out = p.slabs + ((size_t)s * p.m + row) * p.n + pair * 32u + 4u * h;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        *reinterpret_cast<f32x4 *>(out + (u >> 1) * 16 + (u & 1) * 8) = f32x4{acc[4 * u], acc[4 * u + 1], acc[4 * u + 2], acc[4 * u + 3]};
}

// The whole form: native_invariant_whole_kernel's workgroup on (expert, m-tile of 64, 4 slots of two pairs of n-tiles).
template <class AT, int ACT> __global__ __launch_bounds__(256) void native_invariant_moe_whole_kernel(const NativeInvariantMoeArgs p) {
#pragma clang fp contract(off)
    using L = NativeWholeLds<ACT>;
    constexpr unsigned kRowB = L::kRowB, U = L::U;
    constexpr int NA = native_inv_frag_units<ACT>(), MB = 2, NP = 2;
    __shared__ __attribute__((aligned(16))) char lds[2 * L::kBuf];
    const unsigned tid = threadIdx.x, lane = tid & 63u, m_l = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned ntiles = p.n / kTileN, pairs = ntiles / 2, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    const bool gated = p.act != 0;
    const unsigned nb = blockIdx.x % p.nblocks, mslot = blockIdx.x / p.nblocks;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, 64u, mslot, t))
        return; // (workgroup-uniform: before any barrier and any operand load)
    const unsigned slot = nb * 4u + wave;
    unsigned pair[NP];
    bool live[NP]; // (wave-uniform) pairs past N: empty descriptors, nothing stored.  Dead waves still walk the loop: they share the barriers.
    pair[0] = gated ? slot : 2u * slot, pair[1] = gated ? slot + pairs / 2 : 2u * slot + 1;
    live[0] = gated ? slot < pairs / 2 : pair[0] < pairs, live[1] = gated ? live[0] : pair[1] < pairs;
    const unsigned m0 = t.row0 + (mslot - t.first) * 64u, rows_valid = min(t.row0 + t.rows - m0, 64u);
    const char *const w_base = (const char *)p.w + t.expert * moe_w_bytes<kFmtMx>(p.n, p.k);
    const char *const s_base = (const char *)p.s + t.expert * moe_s_bytes<kFmtMx>(p.n, p.k);
    __amdgpu_buffer_rsrc_t w_rsrc[NP][2], s_rsrc[NP][2];
#pragma unroll
    for (int np = 0; np < NP; ++np)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned tt = live[np] ? 2u * pair[np] + j : 0u;
            w_rsrc[np][j] = make_rsrc(w_base + (size_t)tt * ktiles * kTileBytes, live[np] ? ktiles * kTileBytes : 0u);
            s_rsrc[np][j] = make_rsrc(s_base + (size_t)tt * ktiles * 64, live[np] ? ktiles * 64 : 0u);
        }
    const unsigned char *const qa_hi = p.qa + (size_t)p.m * (p.k / 2); // (MXFP6)
    const unsigned char *const qs = p.qa + (size_t)p.m * (p.k / 8 * ACT);

    // staging: 16-byte unit u = tid + 256 i of the tile's run is row u / U, position u % U, which lands at position (u % U) ^ swz(row);
    // MXFP6's second image (32 bytes per row): unit tid < 128 is row tid / 2; the scale dwords: one per row, tid < 64
    auto swz = [](unsigned row) -> unsigned { return ACT == 8 ? (row >> 1) & 7u : (row >> 2) & 3u; };
    constexpr int kDataLoads = (int)(64 * U / 256); // 2 (MXFP8) / 1
    struct AStage {
        u32x4 d[kDataLoads];
        u32x4 hi;
        unsigned sc;
    };
    auto fetch_a = [&](AStage &r, unsigned kt) {
        const size_t tile_row = (size_t)kt * p.m + m0;
        const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.qa + tile_row * kRowB, rows_valid * kRowB);
#pragma unroll
        for (int i = 0; i < kDataLoads; ++i)
            r.d[i] = buf_load16(a_rsrc, (tid + 256u * i) * 16u, 0, kAuxDefault);
        if constexpr (ACT == 6) {
            const __amdgpu_buffer_rsrc_t h_rsrc = make_rsrc(qa_hi + tile_row * 32, rows_valid * 32u);
            if (wave < 2u)
                r.hi = buf_load16(h_rsrc, tid * 16u, 0, kAuxDefault);
        }
        const __amdgpu_buffer_rsrc_t q_rsrc = make_rsrc(qs + tile_row * 4, rows_valid * 4u);
        if (wave == 0u)
            r.sc = __builtin_amdgcn_raw_buffer_load_b32(q_rsrc, tid * 4u, 0, kAuxDefault);
    };
    auto put_a = [&](const AStage &r, unsigned buf) {
        char *const base = lds + buf * L::kBuf;
#pragma unroll
        for (int i = 0; i < kDataLoads; ++i) {
            const unsigned u = tid + 256u * i, row = u / U, pos = u % U;
            *reinterpret_cast<u32x4 *>(base + (row * U + (pos ^ swz(row))) * 16u) = r.d[i];
        }
        if constexpr (ACT == 6) {
            if (wave < 2u) {
                const unsigned row = tid >> 1, pos = tid & 1u;
                *reinterpret_cast<u32x4 *>(base + L::kData + (row * 2u + (pos ^ ((row >> 3) & 1u))) * 16u) = r.hi;
            }
        }
        if (wave == 0u)
            *reinterpret_cast<unsigned *>(base + L::kData + L::kHi + tid * 4u) = r.sc;
    };
    struct WStage {
        u32x4 w[NP][2];
        unsigned sc[NP][2];
    };
    auto load_w = [&](WStage &st, unsigned kt) {
        const unsigned sp = kt / ks, tt = kt - sp * ks;
        const unsigned s_voff = (sp * 64u + lane) * ks + tt;
#pragma unroll
        for (int np = 0; np < NP; ++np)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                st.w[np][j] = buf_load16(w_rsrc[np][j], kt * kTileBytes + lane * 16u, 0, kAuxDefault);
                st.sc[np][j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[np][j], s_voff, 0, kAuxDefault);
            }
    };

    f32x16 total[MB][NP], acc[MB][NP];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int np = 0; np < NP; ++np)
#pragma unroll
            for (int v = 0; v < 16; ++v)
                acc[mb][np][v] = 0.f, total[mb][np][v] = 0.f;
    auto join = [&](bool first) { // a slice is done: the accumulators leave the loop's MFMA block (mfma_join_pin, device_common.hpp)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int np = 0; np < NP; ++np)
                mfma_join_pin(acc[mb][np]);
        mfma_join_settle();
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int np = 0; np < NP; ++np) {
                mfma_join_pin(acc[mb][np]);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    total[mb][np][v] = first ? acc[mb][np][v] : total[mb][np][v] + acc[mb][np][v];
                    acc[mb][np][v] = 0.f;
                }
            }
    };

    WStage ring[kNativeWholeRing];
#pragma unroll
    for (int d = 0; d < kNativeWholeRing; ++d)
        load_w(ring[d], (unsigned)d < ktiles ? d : ktiles - 1);
    {
        AStage r;
        fetch_a(r, 0);
        put_a(r, 0);
    }
    __syncthreads();
    const unsigned slice_tiles = p.slice_k / kTileK;
    unsigned boundary = slice_tiles; // the k-tile that opens the next slice
    const unsigned my_swz = swz(m_l), hi_swz = (m_l >> 3) & 1u; // (32 mb is a multiple of every swizzle period)
    for (unsigned kt = 0; kt < ktiles; ++kt) {
        if (kt == boundary) {
            join(boundary == slice_tiles);
            boundary += slice_tiles;
        }
        AStage nxt;
        fetch_a(nxt, kt + 1 < ktiles ? kt + 1 : kt);
        const WStage cur = ring[0];
#pragma unroll
        for (int d = 0; d + 1 < kNativeWholeRing; ++d)
            ring[d] = ring[d + 1];
        load_w(ring[kNativeWholeRing - 1], kt + kNativeWholeRing < ktiles ? kt + kNativeWholeRing : ktiles - 1);
        i32x8 wop[NP][2];
        unsigned wsc[NP][2];
#pragma unroll
        for (int np = 0; np < NP; ++np)
            native_inv_merge(cur.w[np][0], cur.w[np][1], cur.sc[np][0], cur.sc[np][1], wop[np], wsc[np]);
        const char *const img = lds + (kt & 1u) * L::kBuf;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const unsigned row = mb * 32u + m_l;
            const u32x4 *const a_row = reinterpret_cast<const u32x4 *>(img) + row * U;
            u32x4 a[NA];
            if constexpr (ACT == 8) {
#pragma unroll
                for (int e = 0; e < 4; ++e) // P1: units 2 h, 2 h + 1; P2: units 4 + 2 h, 4 + 2 h + 1
                    a[e] = a_row[(4u * (e >> 1) + 2u * h + (e & 1)) ^ my_swz];
            } else {
                a[0] = a_row[h ^ my_swz], a[1] = a_row[(2u + h) ^ my_swz];
                if constexpr (ACT == 6)
                    a[2] = *reinterpret_cast<const u32x4 *>(img + L::kData + (row * 2u + (h ^ hi_swz)) * 16u);
            }
            const unsigned char *const sc = reinterpret_cast<const unsigned char *>(img + L::kData + L::kHi) + row * 4u;
            const unsigned a_sc1 = sc[h], a_sc2 = sc[2u + h];
#pragma unroll
            for (int np = 0; np < NP; ++np)
                acc[mb][np] = native_inv_ktile<ACT>(acc[mb][np], wop[np], wsc[np], a, a_sc1, a_sc2);
        }
        put_a(nxt, (kt + 1u) & 1u); // the other half: everybody left it at the barrier that ended the previous step
        __syncthreads();
    }
    join(boundary == slice_tiles);

    // lane (m_l, h) holds row m_l of each m-block; register 4 u + i is column 16 (u >> 1) + 8 (u & 1) + 4 h + i of the pair's 32
    const float *const gs = p.gs + t.expert;
    const void *const bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const unsigned local = mb * 32u + m_l;
        if (local >= rows_valid) // rows past the expert's end
            continue;
        const unsigned cm = native_moe_c_row(p, m0 + local);
        if (cm == ~0u)
            continue;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned nl = (u >> 1) * 16u + (u & 1) * 8u + 4u * h;
            if (gated) {
                if (live[0]) {
                    const unsigned n_half = p.n / 2, n = slot * 32u + nl;
                    const f32x16 &tg = total[mb][0], &tu = total[mb][1];
                    *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)cm * n_half + n) * 2) =
                        finish4_silu_mul<AT>(f32x4{tg[4 * u], tg[4 * u + 1], tg[4 * u + 2], tg[4 * u + 3]},
                                             f32x4{tu[4 * u], tu[4 * u + 1], tu[4 * u + 2], tu[4 * u + 3]}, *gs, bias, n, n_half, p.act);
                }
            } else {
#pragma unroll
                for (int np = 0; np < NP; ++np)
                    if (live[np]) {
                        const unsigned n = pair[np] * 32u + nl;
                        const f32x16 &tt = total[mb][np];
                        *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)cm * p.n + n) * 2) =
                            invariant_finish4<AT>(f32x4{tt[4 * u], tt[4 * u + 1], tt[4 * u + 2], tt[4 * u + 3]}, gs, bias, n);
                    }
            }
        }
    }
}

// one activation type's launches; instantiated by gemm_native_invariant_moe_{bf16,f16}.hip.  The grids were bounded by the host (moe_grid,
// gemm_native_invariant_moe_host.h).
template <class AT, int ACT> void native_invariant_moe_launch_fmt(NativeInvariantMoeArgs p, bool split, hipStream_t stream) {
    const unsigned pairs = p.n / (2 * kTileN), active = p.experts < p.m ? p.experts : p.m;
    if (split) {
        const unsigned slots = (p.m + 31) / 32 + active;
        p.nblocks = (pairs + 3) / 4;
        hipLaunchKernelGGL((native_invariant_moe_split_kernel<AT, ACT, kNativeInvariantSplitDepth>), dim3(slots * p.slices * p.nblocks), dim3(256), 0,
                           stream, p);
        // the fold of the exact MoE launch, over its own 16-row slot map of the same offsets
        InvariantMoeArgs f{};
        f.c = p.c, f.gs = p.gs, f.bias = p.bias, f.slabs = p.slabs, f.offsets = p.offsets, f.c_idx = p.c_idx;
        f.m = p.m, f.n = p.n, f.k = p.k, f.slice_k = p.slice_k, f.slices = p.slices, f.act = p.act, f.experts = p.experts, f.c_rows = p.c_rows;
        const unsigned n_out = p.act ? p.n / 2 : p.n, fold_slots = (p.m + 15) / 16 + active;
        f.nblocks = (16u * (n_out / 4) + 1023) / 1024; // a thread folds at most 4 units of its m-tile
        hipLaunchKernelGGL((invariant_moe_fold_kernel<AT>), dim3(fold_slots * f.nblocks), dim3(256), 0, stream, f);
    } else {
        const unsigned slots = (p.m + 63) / 64 + active;
        const unsigned nslots = p.act ? pairs / 2 : (pairs + 1) / 2;
        p.nblocks = (nslots + 3) / 4;
        hipLaunchKernelGGL((native_invariant_moe_whole_kernel<AT, ACT>), dim3(slots * p.nblocks), dim3(256), 0, stream, p);
    }
}
template <class AT> void native_invariant_moe_launch(const NativeInvariantMoeArgs &p, int act_format, bool split, hipStream_t stream) {
    if (act_format == 8)
        native_invariant_moe_launch_fmt<AT, 8>(p, split, stream);
    else if (act_format == 6)
        native_invariant_moe_launch_fmt<AT, 6>(p, split, stream);
    else
        native_invariant_moe_launch_fmt<AT, 4>(p, split, stream);
}

} // namespace petit_amd
