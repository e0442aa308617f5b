// gemm_invariant.hpp -- the batch-invariant dense GEMM (include/petit_amd.h "Batch-invariant GEMM"): every output element is a pure function of
// its activation row, the weights, the scales and the bias -- never of M, of the row's position, or of the launch form.
//
// K is cut into S slices of L (invariant_geometry, gemm_invariant_host.h: a function of (n, k, a_type, b_type) alone).  The partial sum p_s of a
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
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.hpp"

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
    constexpr int MT = 1, NT = 1; // one 16 x 16 tile per wave
    using Frag = typename AT::frag;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned ntiles = p.n / kTileN, ktiles = p.k / kTileK;
    const unsigned ks = (unsigned)span_tiles_for_k(p.k), spans = ktiles / ks;
    constexpr unsigned kRec = FMT == kFmtNv ? 2u : 1u; // scale bytes per lane and k-tile

    // a wave's slot is its n-tile
    const unsigned slot = blockIdx.x * 4u + wave, slots = ntiles / NT;
    const bool live = slot < slots; // (wave-uniform) a ragged last n-block: dead waves read zeros through empty descriptors and store nothing
    const unsigned m0 = blockIdx.z * (16u * MT), s_lo = blockIdx.y, s_hi = s_lo + 1;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 16u * MT ? rows_left : 16u * MT; // (the grid keeps m0 < m)

    // descriptors of this wave's own rows: activations [rows_valid][k] from row m0 on (rows past M: out of range -> zeros), one n-tile's
    // k-tiles, one n-tile's scale records
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc((const char *)p.a + (size_t)m0 * p.k * 2, rows_valid * p.k * 2);
    __amdgpu_buffer_rsrc_t w_rsrc[NT], s_rsrc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const unsigned tile = live ? slot + j * (ntiles / 2) : 0u;
        w_rsrc[j] = make_rsrc((const char *)p.w + (size_t)tile * ktiles * kTileBytes, live ? ktiles * kTileBytes : 0u);
        s_rsrc[j] = make_rsrc((const char *)p.s + (size_t)tile * ktiles * (64 * kRec), live ? ktiles * (64 * kRec) : 0u);
    }
    const unsigned a_voff = (lane & 15u) * p.k * 2 + (lane >> 4) * (kLaneK * 2); // row (lane & 15) of an m-tile, 32 consecutive k

    struct Stage {
        u32x4 w[NT];
        unsigned sc[NT];
        u32x4 a[MT][4];
    };
    auto load_stage = [&](Stage &st, unsigned kt) {
        const unsigned sp = kt / ks, t = kt - sp * ks;
        const unsigned s_voff = ((sp * 64u + lane) * ks + t) * kRec;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            st.w[j] = buf_load16(w_rsrc[j], kt * kTileBytes + lane * 16u, 0, kAuxNt);
            if constexpr (FMT == kFmtNv)
                st.sc[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(s_rsrc[j], s_voff, 0, kAuxNt);
            else
                st.sc[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[j], s_voff, 0, kAuxNt);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4)
                st.a[mt][j4] = buf_load16(a_rsrc, a_voff + mt * 16u * p.k * 2 + kt * (kTileK * 2) + j4 * 16u, 0, kAuxDefault);
    };

    f32x4 total[MT][NT];
    for (unsigned s = s_lo; s < s_hi; ++s) {
        const unsigned kt0 = s * (p.slice_k / kTileK);
        const unsigned kt_end = (s + 1) * (p.slice_k / kTileK), kt1 = kt_end < ktiles ? kt_end : ktiles;
        f32x4 acc[MT][NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[mt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
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
            // the chain of every accumulator: k-tiles ascending, the tile's words in order
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[mt][j] = mfma16(wf[j][j4], __builtin_bit_cast(Frag, cur.a[mt][j4]), acc[mt][j]);
        }
        // the accumulators leave the loop's basic block: see mfma_join_pin (device_common.hpp)
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
                if (s == s_lo)
                    total[mt][j] = acc[mt][j];
                else
                    total[mt][j] = total[mt][j] + acc[mt][j];
            }
    }
    if (!live)
        return;

    // a lane holds 4 consecutive n (4 (lane >> 4) + i) of row (lane & 15) of each tile
    const unsigned nq = (lane >> 4) * 4u;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const unsigned row = m0 + mt * 16u + (lane & 15u);
        if (row >= p.m)
            continue;
        float *out = p.slabs + ((size_t)s_lo * p.m + row) * p.n + slot * 16u + nq;
        *reinterpret_cast<f32x4 *>(out) = total[mt][0];
    }
}

// The whole form.  A workgroup owns 64 rows x 8 n-tiles (4 waves x 2): wave w takes the tile pair of slot 4 blockIdx.x + w -- tiles 2 t and 2 t + 1,
// or (gated) gate tile t and up tile t + ntiles / 2 -- against all four m-tiles.  Per k-tile the 256 threads fetch the 64 x 128 activation tile
// once (4 buffer_load_dwordx4 each, one k-tile ahead, rows past M read zeros through the descriptor) and drop it into the other half of a
// double-buffered LDS image (rows padded by 16 B: the fragment reads of 16 rows are conflict-free); one barrier per k-tile.  The weights stream
// into a register ring kWholeRing k-tiles deep.  Every accumulator keeps ONE chain per slice; at a slice boundary it joins the running total.
constexpr int kWholeRing = 3, kWholeRowBytes = kTileK * 2 + 16, kWholeBufBytes = 64 * kWholeRowBytes;
template <class AT, int FMT> __global__ __launch_bounds__(256) void gemm_invariant_whole_kernel(const InvariantArgs p) {
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
    const unsigned slot = blockIdx.x * 4u + wave;
    unsigned tile[NT];
    bool live[NT]; // (wave-uniform) tiles past N: empty descriptors, nothing stored.  Dead waves still walk the loop: they share the barriers.
    tile[0] = gated ? slot : 2u * slot, tile[1] = gated ? slot + ntiles / 2 : 2u * slot + 1;
    live[0] = gated ? slot < ntiles / 2 : tile[0] < ntiles, live[1] = gated ? live[0] : tile[1] < ntiles;
    const unsigned m0 = blockIdx.y * 64u;
    const unsigned rows_left = p.m - m0, rows_valid = rows_left < 64u ? rows_left : 64u;
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc((const char *)p.a + (size_t)m0 * p.k * 2, rows_valid * p.k * 2);
    __amdgpu_buffer_rsrc_t w_rsrc[NT], s_rsrc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const unsigned t = live[j] ? tile[j] : 0u;
        w_rsrc[j] = make_rsrc((const char *)p.w + (size_t)t * ktiles * kTileBytes, live[j] ? ktiles * kTileBytes : 0u);
        s_rsrc[j] = make_rsrc((const char *)p.s + (size_t)t * ktiles * (64 * kRec), live[j] ? ktiles * (64 * kRec) : 0u);
    }
    // staging: 16-byte unit u = tid + 256 i of the tile is row u / 16, bytes 16 (u % 16) of the row's 256
    unsigned st_voff[4], st_lds[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned u = tid + 256u * i, row = u >> 4, cu = u & 15u;
        st_voff[i] = row * p.k * 2 + cu * 16u, st_lds[i] = row * kWholeRowBytes + cu * 16u;
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
        const unsigned sp = kt / ks, t = kt - sp * ks;
        const unsigned s_voff = ((sp * 64u + lane) * ks + t) * kRec;
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
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const unsigned row = m0 + mt * 16u + (lane & 15u);
        if (row >= p.m)
            continue;
        if (gated) {
            if (live[0]) {
                const unsigned n_half = p.n / 2, n = slot * 16u + nq;
                const float g = p.gs ? *p.gs : 1.0f;
                *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * n_half + n) * 2) =
                    finish4_silu_mul<AT>(total[mt][0], total[mt][1], g, p.bias, n, n_half, p.act);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (live[j]) {
                    const unsigned n = tile[j] * 16u + nq;
                    *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * p.n + n) * 2) = invariant_finish4<AT>(total[mt][j], p.gs, p.bias, n);
                }
        }
    }
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

// one (format, type) pair's launches; instantiated by gemm_invariant_*.hip
template <class AT, int FMT> void invariant_launch(const InvariantArgs &p, bool whole, hipStream_t stream) {
    const unsigned ntiles = p.n / kTileN;
    if (!whole) {
        const dim3 grid((ntiles + 3) / 4, p.slices, (p.m + 15) / 16);
        hipLaunchKernelGGL((gemm_invariant_split_kernel<AT, FMT, kInvariantSplitDepth>), grid, dim3(256), 0, stream, p);
        const unsigned n_out = p.act ? p.n / 2 : p.n;
        const size_t count = (size_t)p.m * (n_out / 4);
        const unsigned blocks = (unsigned)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
        hipLaunchKernelGGL((invariant_fold_kernel<AT>), dim3(blocks), dim3(256), 0, stream, p);
    } else {
        const unsigned slots = p.act ? ntiles / 2 : (ntiles + 1) / 2; // tile pairs
        const dim3 grid((slots + 3) / 4, (p.m + 63) / 64);
        hipLaunchKernelGGL((gemm_invariant_whole_kernel<AT, FMT>), grid, dim3(256), 0, stream, p);
    }
}

} // namespace petit_amd
