// gemm_invariant_whole.inc -- the body of the exact class's whole form, staging to epilogue, stated once: included by
// gemm_invariant_whole_kernel (gemm_invariant.hpp) and gemm_invariant_moe_whole_kernel (gemm_invariant_moe.hpp) after their prologues (a text
// fragment, not a function: see gemm_native_invariant_whole.inc).  It reads AT, FMT and the kernel's `p` (c, n, k, slice_k, act) and expects
// the prologue's
//   tid, lane           thread and lane index
//   a_rsrc              the activation descriptor
//   a_row_off(row)      the byte offset in it of the tile's row `row` (0 .. 63); a row that is not there reads zeros
//   slot                the wave's tile pair of the tensors at w_base / s_base (const char *)
//   m0, rows_valid      the tile's first row and how many of its 64 are there
//   gs, bias            const float * (null: no multiply) and const void * (null: no add) of the epilogue
//   c_row(row)          the row of C that row `row` is written to, or ~0u: not written
using Frag = typename AT::frag;
constexpr int MT = 4, NT = 2;
__shared__ __attribute__((aligned(16))) char lds[2 * kWholeBufBytes];
const unsigned ntiles = p.n / kTileN, ktiles = p.k / kTileK;
const unsigned ks = (unsigned)span_tiles_for_k(p.k);
constexpr unsigned kRec = FMT == kFmtNv ? 2u : 1u;
const bool gated = p.act != 0;
unsigned tile[NT];
bool live[NT]; // (wave-uniform) tiles past N: empty descriptors, nothing stored.  Dead waves still walk the loop: they share the barriers.
tile[0] = gated ? slot : 2u * slot, tile[1] = gated ? slot + ntiles / 2 : 2u * slot + 1;
live[0] = gated ? slot < ntiles / 2 : tile[0] < ntiles, live[1] = gated ? live[0] : tile[1] < ntiles;
__amdgpu_buffer_rsrc_t w_rsrc[NT], s_rsrc[NT];
#pragma unroll
for (int j = 0; j < NT; ++j) {
    const unsigned t = live[j] ? tile[j] : 0u;
    w_rsrc[j] = make_rsrc(w_base + (size_t)t * ktiles * kTileBytes, live[j] ? ktiles * kTileBytes : 0u);
    s_rsrc[j] = make_rsrc(s_base + (size_t)t * ktiles * (64 * kRec), live[j] ? ktiles * (64 * kRec) : 0u);
}
// staging: 16-byte unit u = tid + 256 i of the tile is row u / 16, bytes 16 (u % 16) of the row's 256
unsigned st_voff[4], st_lds[4];
#pragma unroll
for (int i = 0; i < 4; ++i) {
    const unsigned u = tid + 256u * i, row = u >> 4, cu = u & 15u;
    st_voff[i] = a_row_off(row) + cu * 16u, st_lds[i] = row * kWholeRowBytes + cu * 16u;
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
    const unsigned local = mt * 16u + (lane & 15u);
    if (local >= rows_valid) // rows past the tile's last valid row
        continue;
    const unsigned row = c_row(m0 + local);
    if (row == ~0u)
        continue;
    if (gated) {
        if (live[0]) {
            const unsigned n_half = p.n / 2, n = slot * 16u + nq;
            const float g = gs ? *gs : 1.0f;
            *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * n_half + n) * 2) =
                finish4_silu_mul<AT>(total[mt][0], total[mt][1], g, bias, n, n_half, p.act);
        }
    } else {
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (live[j]) {
                const unsigned n = tile[j] * 16u + nq;
                *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)row * p.n + n) * 2) = invariant_finish4<AT>(total[mt][j], gs, bias, n);
            }
    }
}
