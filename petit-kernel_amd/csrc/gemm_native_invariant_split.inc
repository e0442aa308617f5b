// gemm_native_invariant_split.inc -- the body of the native class's split form, descriptors to slab store, stated once: included by
// native_invariant_split_kernel (gemm_native_invariant.hpp) and native_invariant_moe_split_kernel (gemm_native_invariant_moe.hpp) after their
// prologues (a text fragment, not a function: see gemm_native_invariant_whole.inc).  It reads ACT, kDepth and the kernel's `p` (qa, slabs, m,
// n, k, slice_k) and expects the prologue's
//   WF                the weight operand (gemm_native_invariant.hpp): 4 raw MXFP4, 6 the NVFP4 image
//   lane, m_l, h      the lane index, lane & 31 (the lane's row of the tile) and lane >> 5
//   ktiles, ks        k / 128 and span_tiles_for_k(k)
//   pair, s           the wave's pair of n-tiles (WF = 6: its block of 32 weight rows) of the tensors at w_base / s_base (const char *; WF = 6:
//                     the image's elements and its scale region) and its slice
//   m0, rows_valid    the tile's first row of the m quantised rows and how many of its 32 are there
constexpr unsigned kRowB = native_inv_row_bytes<ACT>();
constexpr int NA = native_inv_frag_units<ACT>(), NW = native_inv_w_units<WF>(), NR = WF == 6 ? 1 : 2;
__amdgpu_buffer_rsrc_t w_rsrc[NR], s_rsrc[NR];
if constexpr (WF == 6) { // the block's stream along K: 3 KiB of elements and 128 scale bytes per k-tile
    w_rsrc[0] = make_rsrc(w_base + (size_t)pair * ktiles * kNv6TileBytes, ktiles * kNv6TileBytes);
    s_rsrc[0] = make_rsrc(s_base + (size_t)pair * ktiles * 128, ktiles * 128);
} else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned tile = 2u * pair + j;
        w_rsrc[j] = make_rsrc(w_base + (size_t)tile * ktiles * kTileBytes, ktiles * kTileBytes);
        s_rsrc[j] = make_rsrc(s_base + (size_t)tile * ktiles * 64, ktiles * 64);
    }
}
const unsigned char *const qa_hi = p.qa + qact_hi_offset(p.m, p.k); // (MXFP6; "petit-qact/1": layout.h)
const unsigned char *const qs = p.qa + qact_elem_bytes(p.m, p.k, ACT);
const unsigned a_voff = m_l * kRowB + h * (ACT == 8 ? 32u : 16u);

struct Stage {
    u32x4 w[NW];
    unsigned sc[2];
    u32x4 a[NA];
    unsigned asc;
};
auto load_stage = [&](Stage &st, unsigned kt) {
    const unsigned sp = kt / ks, t = kt - sp * ks;
    if constexpr (WF == 6) { // the lane's unit of planes 0, 1, 2 (nv6_unit_offset) and its bytes [q][t] (nv6_scale_offset), q = 0, 1
        const unsigned s_voff = (sp * 64u + lane) * (2u * ks) + t;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            st.w[i] = buf_load16(w_rsrc[0], kt * kNv6TileBytes + i * 1024u + lane * 16u, 0, kAuxNt);
#pragma unroll
        for (int q = 0; q < 2; ++q)
            st.sc[q] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[0], s_voff + q * ks, 0, kAuxNt);
    } else {
        const unsigned s_voff = (sp * 64u + lane) * ks + t;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            st.w[j] = buf_load16(w_rsrc[j], kt * kTileBytes + lane * 16u, 0, kAuxNt);
            st.sc[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[j], s_voff, 0, kAuxNt);
        }
    }
    // the k-tile's rows m0 .. m0 + rows_valid - 1 of every image: rows past the tile's last valid row are out of range -> zeros
    const size_t tile_row = qact_tile_row(p.m, kt, m0);
    const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(p.qa + tile_row * kRowB, rows_valid * kRowB);
    const __amdgpu_buffer_rsrc_t q_rsrc = make_rsrc(qs + tile_row * kQactScaleRowBytes, rows_valid * kQactScaleRowBytes);
    if constexpr (ACT == 8) {
        st.a[0] = buf_load16(a_rsrc, a_voff, 0, kAuxDefault), st.a[1] = buf_load16(a_rsrc, a_voff + 16u, 0, kAuxDefault);
        st.a[2] = buf_load16(a_rsrc, a_voff + 64u, 0, kAuxDefault), st.a[3] = buf_load16(a_rsrc, a_voff + 80u, 0, kAuxDefault);
    } else {
        st.a[0] = buf_load16(a_rsrc, a_voff, 0, kAuxDefault), st.a[1] = buf_load16(a_rsrc, a_voff + 32u, 0, kAuxDefault);
        if constexpr (ACT == 6) {
            const __amdgpu_buffer_rsrc_t h_rsrc = make_rsrc(qa_hi + tile_row * kQactHiRowBytes, rows_valid * kQactHiRowBytes);
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
    if constexpr (WF == 6)
        native_inv_image_ops(cur.w, cur.sc, wop, wsc);
    else
        native_inv_merge(cur.w[0], cur.w[1], cur.sc[0], cur.sc[1], wop, wsc);
    // this lane's block is 2 q + h of the k-tile's four
    acc = native_inv_ktile<ACT, WF>(acc, wop, wsc, cur.a, (cur.asc >> (8u * h)) & 0xffu, (cur.asc >> (16u + 8u * h)) & 0xffu);
}
// the accumulator leaves the loop's basic block (mfma_join_pin, device_common.hpp), and every MFMA executes with all 64 lanes before the
// lane-divergent stores (pin_acc, gemm_native.hpp)
mfma_join_pin(acc);
mfma_join_settle();
mfma_join_pin(acc);

// lane (m_l, h) holds row m_l of the tile; register 4 u + i is column 16 (u >> 1) + 8 (u & 1) + 4 h + i of the pair's 32
if (m_l >= rows_valid)
    return;
float *const out = p.slabs + ((size_t)s * p.m + m0 + m_l) * p.n + pair * 32u + 4u * h;
#pragma unroll
for (int u = 0; u < 4; ++u)
    *reinterpret_cast<f32x4 *>(out + (u >> 1) * 16 + (u & 1) * 8) = f32x4{acc[4 * u], acc[4 * u + 1], acc[4 * u + 2], acc[4 * u + 3]};
