// gemm_native_invariant.hpp -- the batch-invariant GEMM on the native class (include/petit_amd.h "Batch-invariant GEMM on the native class"):
// raw MXFP4 weights against MXFP8 / MXFP6 / MXFP4 activations ("petit-qact/1" bytes) on v_mfma_scale_f32_32x32x64_f8f6f4, every output element a
// pure function of its quantised activation row, the weights, the scales and the bias -- never of M, of the row's position, or of the launch form.
//
// K is cut into S slices of L (invariant_geometry, gemm_invariant_host.h: a function of (n, k) alone).  The partial sum p_s of a slice is ONE
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
template <int ACT> constexpr unsigned native_inv_row_bytes() { return ACT == 8 ? 128u : 64u; }
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

// one k-tile of one accumulator's chain: P1, then P2.  w0 / w1: the packed words of the pair's two n-tiles, s0 / s1 their span-record bytes.
template <int ACT>
__device__ __forceinline__ f32x16 native_inv_ktile(f32x16 acc, const i32x8 (&wop)[2], const unsigned (&wsc)[2],
                                                   const u32x4 (&a)[native_inv_frag_units<ACT>()], const unsigned a_sc1, const unsigned a_sc2) {
    constexpr int kBlgp = ACT == 8 ? 0 : ACT == 6 ? 2 : 4; // the activation operand's format: e4m3 / e2m3 / e2m1
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wop[0], native_inv_aop<ACT>(a, 0), acc, 4 /* A = FP4 */, kBlgp, 0, (int)wsc[0], 0, (int)a_sc1);
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wop[1], native_inv_aop<ACT>(a, 1), acc, 4, kBlgp, 0, (int)wsc[1], 0, (int)a_sc2);
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

// The split form.  ACT: 8 / 6 / 4.  kDepth: k-tiles in flight per wave.  (AT does not enter the arithmetic: the slabs are fp32.)
template <class AT, int ACT, int kDepth> __global__ __launch_bounds__(256) void native_invariant_split_kernel(const NativeInvariantArgs p) {
    constexpr unsigned kRowB = native_inv_row_bytes<ACT>();
    constexpr int NA = native_inv_frag_units<ACT>();
    const unsigned lane = threadIdx.x & 63u, m_l = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned ntiles = p.n / kTileN, pairs = ntiles / 2, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k);
    const unsigned slot = blockIdx.x * 4u + wave; // a wave's slot is its pair of n-tiles
    if (slot >= pairs)
        return; // (wave-uniform; the loop has no barrier)
    const unsigned m0 = blockIdx.z * 32u, s = blockIdx.y;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 32u ? rows_left : 32u; // (the grid keeps m0 < m)

    __amdgpu_buffer_rsrc_t w_rsrc[2], s_rsrc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned tile = 2u * slot + j;
        w_rsrc[j] = make_rsrc((const char *)p.w + (size_t)tile * ktiles * kTileBytes, ktiles * kTileBytes);
        s_rsrc[j] = make_rsrc((const char *)p.s + (size_t)tile * ktiles * 64, ktiles * 64);
    }
    const unsigned char *const qa_hi = p.qa + (size_t)p.m * (p.k / 2);        // (MXFP6)
    const unsigned char *const qs = p.qa + (size_t)p.m * (p.k / 8 * ACT);
    const unsigned a_voff = m_l * kRowB + h * (ACT == 8 ? 32u : 16u);

    struct Stage {
        u32x4 w[2];
        unsigned sc[2];
        u32x4 a[NA];
        unsigned asc;
    };
    auto load_stage = [&](Stage &st, unsigned kt) {
        const unsigned sp = kt / ks, t = kt - sp * ks;
        const unsigned s_voff = (sp * 64u + lane) * ks + t;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            st.w[j] = buf_load16(w_rsrc[j], kt * kTileBytes + lane * 16u, 0, kAuxNt);
            st.sc[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[j], s_voff, 0, kAuxNt);
        }
        // the k-tile's rows m0 .. m0 + rows_valid - 1 of every image: rows past M are out of range -> zeros
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
    const unsigned row = m0 + m_l;
    if (row >= p.m)
        return;
    float *const out = p.slabs + ((size_t)s * p.m + row) * p.n + slot * 32u + 4u * h;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        *reinterpret_cast<f32x4 *>(out + (u >> 1) * 16 + (u & 1) * 8) = f32x4{acc[4 * u], acc[4 * u + 1], acc[4 * u + 2], acc[4 * u + 3]};
}

// The whole form.  A workgroup owns 64 rows x 4 slots (one per wave); a slot is two pairs of n-tiles: pairs 2 t and 2 t + 1, or (gated) gate pair t
// and up pair t + ntiles / 4.  Per k-tile the 256 threads fetch the 64-row activation tile once (one k-tile ahead; the tile is ONE contiguous run
// of the k-tile-major layout, rows past M read zeros through the descriptor) and drop it into the other half of a double-buffered LDS image with
// the unit swizzle of gemm_native32.hpp (the 16 lanes of a ds_read_b128 group hit 16 different slots); one barrier per k-tile.  The weights stream
// into a register ring kNativeWholeRing k-tiles deep.  Every accumulator keeps ONE chain per slice; at a slice boundary it joins the running total.
constexpr int kNativeWholeRing = 2;
template <int ACT> struct NativeWholeLds {
    static constexpr unsigned kRowB = native_inv_row_bytes<ACT>(), U = kRowB / 16;
    static constexpr unsigned kData = 64 * kRowB, kHi = ACT == 6 ? 64 * 32 : 0, kScale = 64 * 4;
    static constexpr unsigned kBuf = kData + kHi + kScale;
};
template <class AT, int ACT> __global__ __launch_bounds__(256) void native_invariant_whole_kernel(const NativeInvariantArgs p) {
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
    const unsigned slot = blockIdx.x * 4u + wave;
    unsigned pair[NP];
    bool live[NP]; // (wave-uniform) pairs past N: empty descriptors, nothing stored.  Dead waves still walk the loop: they share the barriers.
    pair[0] = gated ? slot : 2u * slot, pair[1] = gated ? slot + pairs / 2 : 2u * slot + 1;
    live[0] = gated ? slot < pairs / 2 : pair[0] < pairs, live[1] = gated ? live[0] : pair[1] < pairs;
    const unsigned m0 = blockIdx.y * 64u;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 64u ? rows_left : 64u;
    __amdgpu_buffer_rsrc_t w_rsrc[NP][2], s_rsrc[NP][2];
#pragma unroll
    for (int np = 0; np < NP; ++np)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned t = live[np] ? 2u * pair[np] + j : 0u;
            w_rsrc[np][j] = make_rsrc((const char *)p.w + (size_t)t * ktiles * kTileBytes, live[np] ? ktiles * kTileBytes : 0u);
            s_rsrc[np][j] = make_rsrc((const char *)p.s + (size_t)t * ktiles * 64, live[np] ? ktiles * 64 : 0u);
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
        const unsigned sp = kt / ks, t = kt - sp * ks;
        const unsigned s_voff = (sp * 64u + lane) * ks + t;
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
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const unsigned row = m0 + mb * 32u + m_l;
        if (row >= p.m)
            continue;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned nl = (u >> 1) * 16u + (u & 1) * 8u + 4u * h;
            if (gated) {
                if (live[0]) {
                    const unsigned n_half = p.n / 2, n = slot * 32u + nl;
                    const float g = p.gs ? *p.gs : 1.0f;
                    const f32x16 &tg = total[mb][0], &tu = total[mb][1];
                    *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * n_half + n) * 2) =
                        finish4_silu_mul<AT>(f32x4{tg[4 * u], tg[4 * u + 1], tg[4 * u + 2], tg[4 * u + 3]},
                                             f32x4{tu[4 * u], tu[4 * u + 1], tu[4 * u + 2], tu[4 * u + 3]}, g, p.bias, n, n_half, p.act);
                }
            } else {
#pragma unroll
                for (int np = 0; np < NP; ++np)
                    if (live[np]) {
                        const unsigned n = pair[np] * 32u + nl;
                        const f32x16 &t = total[mb][np];
                        *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * p.n + n) * 2) =
                            invariant_finish4<AT>(f32x4{t[4 * u], t[4 * u + 1], t[4 * u + 2], t[4 * u + 3]}, p.gs, p.bias, n);
                    }
            }
        }
    }
}

constexpr int kNativeInvariantSplitDepth = 3;

// one activation type's launches; instantiated by gemm_native_invariant_{bf16,f16}.hip
template <class AT, int ACT> void native_invariant_launch_fmt(const NativeInvariantArgs &p, bool whole, hipStream_t stream) {
    const unsigned pairs = p.n / (2 * kTileN);
    if (!whole) {
        const dim3 grid((pairs + 3) / 4, p.slices, (p.m + 31) / 32);
        hipLaunchKernelGGL((native_invariant_split_kernel<AT, ACT, kNativeInvariantSplitDepth>), grid, dim3(256), 0, stream, p);
        InvariantArgs f{};
        f.c = p.c, f.gs = p.gs, f.bias = p.bias, f.slabs = p.slabs, f.m = p.m, f.n = p.n, f.k = p.k, f.slice_k = p.slice_k, f.slices = p.slices,
        f.act = p.act;
        const unsigned n_out = p.act ? p.n / 2 : p.n;
        const size_t count = (size_t)p.m * (n_out / 4);
        const unsigned blocks = (unsigned)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
        hipLaunchKernelGGL((invariant_fold_kernel<AT>), dim3(blocks), dim3(256), 0, stream, f);
    } else {
        const unsigned slots = p.act ? pairs / 2 : (pairs + 1) / 2;
        const dim3 grid((slots + 3) / 4, (p.m + 63) / 64);
        hipLaunchKernelGGL((native_invariant_whole_kernel<AT, ACT>), grid, dim3(256), 0, stream, p);
    }
}
template <class AT> void native_invariant_launch(const NativeInvariantArgs &p, int act_format, bool whole, hipStream_t stream) {
    if (act_format == 8)
        native_invariant_launch_fmt<AT, 8>(p, whole, stream);
    else if (act_format == 6)
        native_invariant_launch_fmt<AT, 6>(p, whole, stream);
    else
        native_invariant_launch_fmt<AT, 4>(p, whole, stream);
}

} // namespace petit_amd
