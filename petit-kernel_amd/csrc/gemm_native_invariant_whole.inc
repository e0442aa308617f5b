// gemm_native_invariant_whole.inc -- the body of the native class's whole form, staging to epilogue, stated once: included by
// native_invariant_whole_kernel (gemm_native_invariant.hpp) and native_invariant_moe_whole_kernel (gemm_native_invariant_moe.hpp) after their
// prologues.  A text fragment and not a function: behind a call, inlined or not, the compiler rotates the weight ring elsewhere in the k-loop
// (profiles/invariant_shared_bodies.md).  It reads AT, ACT and the kernel's `p` (c, qa, m, n, k, slice_k, act) and expects the prologue's
//   WF                the weight operand (gemm_native_invariant.hpp): 4 raw MXFP4, 6 the NVFP4 image
//   tid, lane, wave   thread, lane and (uniform) wave index
//   slot              the wave's slot: two pairs of n-tiles (WF = 6: two blocks of 32 weight rows, `pair` below) of the tensors at w_base /
//                     s_base (const char *; WF = 6: the image's elements and its scale region)
//   m0, rows_valid    the tile's first row of the m quantised rows and how many of its 64 are there
//   gs, bias          const float * (null: no multiply) and const void * (null: no add) of the epilogue
//   c_row(row)        the row of C that row `row` is written to, or ~0u: not written
using L = NativeWholeLds<ACT>;
constexpr unsigned kRowB = L::kRowB, U = L::U;
constexpr int NA = native_inv_frag_units<ACT>(), MB = 2, NP = 2, NW = native_inv_w_units<WF>(), NR = WF == 6 ? 1 : 2;
__shared__ __attribute__((aligned(16))) char lds[2 * L::kBuf];
const unsigned m_l = lane & 31u, h = lane >> 5;
const unsigned ntiles = p.n / kTileN, pairs = ntiles / 2, ktiles = p.k / kTileK;
const unsigned ks = (unsigned)span_tiles_for_k(p.k);
const bool gated = p.act != 0;
unsigned pair[NP];
bool live[NP]; // (wave-uniform) pairs past N: empty descriptors, nothing stored.  Dead waves still walk the loop: they share the barriers.
pair[0] = gated ? slot : 2u * slot, pair[1] = gated ? slot + pairs / 2 : 2u * slot + 1;
live[0] = gated ? slot < pairs / 2 : pair[0] < pairs, live[1] = gated ? live[0] : pair[1] < pairs;
__amdgpu_buffer_rsrc_t w_rsrc[NP][NR], s_rsrc[NP][NR];
#pragma unroll
for (int np = 0; np < NP; ++np)
    if constexpr (WF == 6) { // the block's stream along K: 3 KiB of elements and 128 scale bytes per k-tile
        const unsigned b = live[np] ? pair[np] : 0u;
        w_rsrc[np][0] = make_rsrc(w_base + (size_t)b * ktiles * kNv6TileBytes, live[np] ? ktiles * kNv6TileBytes : 0u);
        s_rsrc[np][0] = make_rsrc(s_base + (size_t)b * ktiles * 128, live[np] ? ktiles * 128 : 0u);
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned t = live[np] ? 2u * pair[np] + j : 0u;
            w_rsrc[np][j] = make_rsrc(w_base + (size_t)t * ktiles * kTileBytes, live[np] ? ktiles * kTileBytes : 0u);
            s_rsrc[np][j] = make_rsrc(s_base + (size_t)t * ktiles * 64, live[np] ? ktiles * 64 : 0u);
        }
    }
const unsigned char *const qa_hi = p.qa + qact_hi_offset(p.m, p.k); // (MXFP6; "petit-qact/1": layout.h)
const unsigned char *const qs = p.qa + qact_elem_bytes(p.m, p.k, ACT);

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
    const size_t tile_row = qact_tile_row(p.m, kt, m0);
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.qa + tile_row * kRowB, rows_valid * kRowB);
#pragma unroll
    for (int i = 0; i < kDataLoads; ++i)
        r.d[i] = buf_load16(a_rsrc, (tid + 256u * i) * 16u, 0, kAuxDefault);
    if constexpr (ACT == 6) {
        const __amdgpu_buffer_rsrc_t h_rsrc = make_rsrc(qa_hi + tile_row * kQactHiRowBytes, rows_valid * kQactHiRowBytes);
        if (wave < 2u)
            r.hi = buf_load16(h_rsrc, tid * 16u, 0, kAuxDefault);
    }
    const __amdgpu_buffer_rsrc_t q_rsrc = make_rsrc(qs + tile_row * kQactScaleRowBytes, rows_valid * kQactScaleRowBytes);
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
    u32x4 w[NP][NW];
    unsigned sc[NP][2];
};
auto load_w = [&](WStage &st, unsigned kt) {
    const unsigned sp = kt / ks, t = kt - sp * ks;
    if constexpr (WF == 6) { // the lane's unit of planes 0, 1, 2 (nv6_unit_offset) and its bytes [q][t] (nv6_scale_offset), q = 0, 1
        const unsigned s_voff = (sp * 64u + lane) * (2u * ks) + t;
#pragma unroll
        for (int np = 0; np < NP; ++np) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
                st.w[np][i] = buf_load16(w_rsrc[np][0], kt * kNv6TileBytes + i * 1024u + lane * 16u, 0, kAuxDefault);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                st.sc[np][q] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[np][0], s_voff + q * ks, 0, kAuxDefault);
        }
    } else {
        const unsigned s_voff = (sp * 64u + lane) * ks + t;
#pragma unroll
        for (int np = 0; np < NP; ++np)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                st.w[np][j] = buf_load16(w_rsrc[np][j], kt * kTileBytes + lane * 16u, 0, kAuxDefault);
                st.sc[np][j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[np][j], s_voff, 0, kAuxDefault);
            }
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
        if constexpr (WF == 6)
            native_inv_image_ops(cur.w[np], cur.sc[np], wop[np], wsc[np]);
        else
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
            acc[mb][np] = native_inv_ktile<ACT, WF>(acc[mb][np], wop[np], wsc[np], a, a_sc1, a_sc2);
    }
    put_a(nxt, (kt + 1u) & 1u); // the other half: everybody left it at the barrier that ended the previous step
    __syncthreads();
}
join(boundary == slice_tiles);

// lane (m_l, h) holds row m_l of each m-block; register 4 u + i is column 16 (u >> 1) + 8 (u & 1) + 4 h + i of the pair's 32
#pragma unroll
for (int mb = 0; mb < MB; ++mb) {
    const unsigned local = mb * 32u + m_l;
    if (local >= rows_valid) // rows past the tile's last valid row
        continue;
    const unsigned row = c_row(m0 + local);
    if (row == ~0u)
        continue;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned nl = (u >> 1) * 16u + (u & 1) * 8u + 4u * h;
        if (gated) {
            if (live[0]) {
                const unsigned n_half = p.n / 2, n = slot * 32u + nl;
                const float g = gs ? *gs : 1.0f;
                const f32x16 &tg = total[mb][0], &tu = total[mb][1];
                *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * n_half + n) * 2) =
                    finish4_silu_mul<AT>(f32x4{tg[4 * u], tg[4 * u + 1], tg[4 * u + 2], tg[4 * u + 3]},
                                         f32x4{tu[4 * u], tu[4 * u + 1], tu[4 * u + 2], tu[4 * u + 3]}, g, bias, n, n_half, p.act);
            }
        } else {
#pragma unroll
            for (int np = 0; np < NP; ++np)
                if (live[np]) {
                    const unsigned n = pair[np] * 32u + nl;
                    const f32x16 &t = total[mb][np];
                    *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * p.n + n) * 2) =
                        invariant_finish4<AT>(f32x4{t[4 * u], t[4 * u + 1], t[4 * u + 2], t[4 * u + 3]}, gs, bias, n);
                }
        }
    }
}
