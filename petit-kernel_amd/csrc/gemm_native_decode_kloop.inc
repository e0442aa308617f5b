// gemm_native_decode_kloop.inc -- the K loop of the decode kernels on the native image, rings to the waves' tiles in LDS, stated once: included
// by native_decode_kernel (gemm_native_decode.hpp) and native_moe_decode_kernel (gemm_native_moe_decode.hpp) after their prologues (a text
// fragment, not a function: see gemm_native_invariant_whole.inc).  It reads AT, ACT, QIN, NB, NA and kRowB and expects the prologue's
//   red                      the workgroup's LDS, [wave][nb][register][lane] floats
//   lane, r, h, wave         the lane index, lane & 31 (the lane's row of the m-tile), lane >> 5, and the wave of the workgroup
//   ktiles, ks               k / 128 and span_tiles_for_k(k)
//   kt0, kt1                 the wave's run of k-tiles, at least one
//   w_rsrc[NB], s_rsrc[NB]   each block's elements from k-tile kt0 on, ending with the run, and the block's whole scale region
//   QIN:  qa, qa_hi, qs      the regions of the "petit-qact/1" image, which holds qa_m rows; the m-tile is its rows qa_m0 .. qa_m0 + qa_rows - 1
//   !QIN: a16_rsrc, a16_voff the 16-bit matrix and the byte offset of the lane's first unit of k-tile 0 in it (out of range: a zero row)
// and leaves acc[NB] stored to red, behind a barrier; decode_sum4 (gemm_native_decode.hpp) then adds the waves' tiles.
struct WStage {
    u32x4 w[NB][3];
    unsigned sc[NB][2];
};
struct AStage {
    DecodeRawA raw;  // 16-bit input
    u32x4 a[NA];     // quantised input
    unsigned asc;
};
// (kt may run past the wave's last k-tile in both loads: such a stage is never used)
auto load_w = [&](WStage &st, unsigned kt) {
    const unsigned rel = kt - kt0, sp = kt / ks, t = kt - sp * ks;
    const unsigned s_voff = (sp * 64u + lane) * (2u * ks) + t;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            st.w[nb][i] = buf_load16(w_rsrc[nb], rel * kNv6TileBytes + i * 1024u + lane * 16u, 0, kAuxNt);
#pragma unroll
        for (int q = 0; q < 2; ++q)
            st.sc[nb][q] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(s_rsrc[nb], s_voff + q * ks, 0, kAuxDefault);
    }
};
auto load_a = [&](AStage &st, unsigned kt) {
    if constexpr (QIN) { // the k-tile's rows of the m-tile in every region; rows past the tile's last valid row are out of range -> zeros
        const size_t tile_row = qact_tile_row(qa_m, kt < ktiles ? kt : ktiles - 1u, qa_m0);
        const __amdgpu_buffer_rsrc_t a_rsrc = make_rsrc(qa + tile_row * kRowB, qa_rows * kRowB);
        const __amdgpu_buffer_rsrc_t q_rsrc = make_rsrc(qs + tile_row * kQactScaleRowBytes, qa_rows * kQactScaleRowBytes);
        const unsigned a_voff = r * kRowB + h * (ACT == 8 ? 32u : 16u);
        if constexpr (ACT == 8) {
            st.a[0] = buf_load16(a_rsrc, a_voff, 0, kAuxDefault), st.a[1] = buf_load16(a_rsrc, a_voff + 16u, 0, kAuxDefault);
            st.a[2] = buf_load16(a_rsrc, a_voff + 64u, 0, kAuxDefault), st.a[3] = buf_load16(a_rsrc, a_voff + 80u, 0, kAuxDefault);
        } else {
            st.a[0] = buf_load16(a_rsrc, a_voff, 0, kAuxDefault), st.a[1] = buf_load16(a_rsrc, a_voff + 32u, 0, kAuxDefault);
            if constexpr (ACT == 6) {
                const __amdgpu_buffer_rsrc_t h_rsrc = make_rsrc(qa_hi + tile_row * kQactHiRowBytes, qa_rows * kQactHiRowBytes);
                st.a[2] = buf_load16(h_rsrc, r * 32u + h * 16u, 0, kAuxDefault);
            }
        }
        st.asc = __builtin_amdgcn_raw_buffer_load_b32(q_rsrc, r * 4u, 0, kAuxDefault);
    } else {
        const unsigned voff = a16_voff + kt * (kTileK * 2u);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) // MXFP8: units 2, 3 are the lane's 16 elements of the instruction's second block, 32 k further
                st.raw.u[q][j] = buf_load16(a16_rsrc, voff + q * 128u + (ACT == 8 ? (j >> 1) * 64u + (j & 1) * 16u : j * 16u), 0, kAuxDefault);
    }
};

f32x16 acc[NB];
#pragma unroll
for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int v = 0; v < 16; ++v)
        acc[nb][v] = 0.f;
// two rings: the weights DW k-tiles deep (the same bytes in flight for one block or two), the activations DA (raw 16-bit rows are 32
// registers per k-tile and come from the L2)
constexpr int DW = kDecodeRing / NB, DA = QIN ? DW : 2;
WStage wring[DW];
AStage aring[DA];
#pragma unroll
for (int d = 0; d < DW; ++d)
    load_w(wring[d], kt0 + d);
#pragma unroll
for (int d = 0; d < DA; ++d)
    load_a(aring[d], kt0 + d);
for (unsigned kt = kt0; kt < kt1; ++kt) {
    const WStage cur = wring[0];
    const AStage cur_a = aring[0];
#pragma unroll
    for (int d = 0; d + 1 < DW; ++d)
        wring[d] = wring[d + 1];
#pragma unroll
    for (int d = 0; d + 1 < DA; ++d)
        aring[d] = aring[d + 1];
    load_w(wring[DW - 1], kt + DW);
    load_a(aring[DA - 1], kt + DA);
    u32x4 a[NA];
    unsigned a_sc[2];
    if constexpr (QIN) {
#pragma unroll
        for (int i = 0; i < NA; ++i)
            a[i] = cur_a.a[i];
        a_sc[0] = (cur_a.asc >> (8u * h)) & 0xffu, a_sc[1] = (cur_a.asc >> (16u + 8u * h)) & 0xffu; // this lane's block is 2 q + h
    } else {
        decode_quantize<AT, ACT>(cur_a.raw, h, a, a_sc);
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        i32x8 wop[2];
        unsigned wsc[2];
        native_inv_image_ops(cur.w[nb], cur.sc[nb], wop, wsc);
        acc[nb] = native_inv_ktile<ACT, 6>(acc[nb], wop, wsc, a, a_sc[0], a_sc[1]);
    }
}
// the accumulators leave the loop's basic block (mfma_join_pin, device_common.hpp)
#pragma unroll
for (int nb = 0; nb < NB; ++nb)
    mfma_join_pin(acc[nb]);
mfma_join_settle();
#pragma unroll
for (int nb = 0; nb < NB; ++nb)
    mfma_join_pin(acc[nb]);

// the waves' tiles meet in LDS: red[wave][nb][register][lane]
#pragma unroll
for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int v = 0; v < 16; ++v)
        red[((wave * NB + nb) * 16u + v) * 64u + lane] = acc[nb][v];
__syncthreads();
