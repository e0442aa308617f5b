// gemm_invariant_split.inc -- the body of the exact class's split form, descriptors to slab store, stated once: included by
// gemm_invariant_split_kernel (gemm_invariant.hpp) and gemm_invariant_moe_split_kernel (gemm_invariant_moe.hpp) after their prologues (a
// text fragment, not a function: see gemm_native_invariant_whole.inc).  It reads AT, FMT, kDepth and the kernel's `p` (slabs, m, n, k,
// slice_k) and expects the prologue's
//   lane              the lane index
//   a_rsrc, a_voff    the activation descriptor and the lane's byte offset in it: row (lane & 15) of the m-tile, 32 consecutive k from
//                     32 (lane >> 4) on; a row that is not there reads zeros
//   tile, live, s     the wave's n-tile of the tensors at w_base / s_base (const char *), whether it exists (wave-uniform: dead waves of a
//                     ragged last n-block read zeros through empty descriptors and store nothing), and its slice
//   m0, rows_valid    the tile's first row (of the slabs' m) and how many of its 16 are there
using Frag = typename AT::frag;
const unsigned ktiles = p.k / kTileK;
const unsigned ks = (unsigned)span_tiles_for_k(p.k);
constexpr unsigned kRec = FMT == kFmtNv ? 2u : 1u; // scale bytes per lane and k-tile

const unsigned wt = live ? tile : 0u;
const __amdgpu_buffer_rsrc_t w_rsrc = make_rsrc(w_base + (size_t)wt * ktiles * kTileBytes, live ? ktiles * kTileBytes : 0u);
const __amdgpu_buffer_rsrc_t s_rsrc = make_rsrc(s_base + (size_t)wt * ktiles * (64 * kRec), live ? ktiles * (64 * kRec) : 0u);

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

const unsigned kt0 = s * (p.slice_k / kTileK);
const unsigned kt_end = (s + 1) * (p.slice_k / kTileK), kt1 = kt_end < ktiles ? kt_end : ktiles;
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
    const unsigned row = m0 + (lane & 15u);
    float *out = p.slabs + ((size_t)s * p.m + row) * p.n + tile * 16u + (lane >> 4) * 4u;
    *reinterpret_cast<f32x4 *>(out) = acc;
}
