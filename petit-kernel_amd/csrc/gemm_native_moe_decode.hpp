// gemm_native_moe_decode.hpp -- the routed-expert (MoE) decode GEMM on the native images (include/petit_amd.h "MoE decode on the native
// image"): a decode step puts 0-4 rows on each expert and none on most, so the launch streams only the images of the experts that have rows,
// spreads a block's K over the waves of a workgroup, and runs nothing before itself -- no quantiser, no scratch, no second launch.
//
// Grid: (n-blocks) x (slots), slots = ceil(m / 32) + min(E, m), sized on the host from (m, E, n) alone.  moe_locate (gemm_moe.hpp; the clamp
//   rule on malformed offsets is the project's one) maps a slot to (expert, m-tile of 32 of that expert's grouped rows); a slot past the last
//   tile returns before any operand load, so an expert without rows costs no weight traffic.  An expert with more than 32 rows has more
//   m-tiles and its weights are streamed once per tile: correct for any routing, efficient for the decode case.  n-blocks: n / 32 plain;
//   gated n / 64, gate block b with up block b + n / 64.
// Workgroup: ONE block of 32 weight rows (gated: a gate and its up block) of ONE expert and one m-tile, W = decode_waves(k / 128, 1) =
//   min(4, k / 128) waves, wave w on the k-tiles [w T / W, (w + 1) T / W).  No K split across workgroups: no slabs, no fold, no workspace.
// Weights: expert e's image starts e * nv6_image_bytes(n, k) into `images`, its scale region after its own elements (what
//   gemm_native_invariant_moe.hpp reads).  The stream, the ring, the MFMA and the waves' meeting in LDS are the dense decode kernel's, one text
//   for both: gemm_native_decode_kloop.inc.
// Activations: lane 32 h + r holds grouped row m0 + r.  16-bit input: row a_idx[m0 + r] (null: m0 + r) of [a_rows][k], the index read once
//   per lane; an index outside [0, a_rows) and a row >= rows_valid get an out-of-range offset (2^31, past the one descriptor over A) and so
//   load zeros -- no branch in the loop -- and are quantised in the lane's registers by decode_quantize.  Quantised input: "petit-qact/1" of
//   the m grouped rows, k-tile-major; the descriptors of a k-tile start at the tile's first grouped row and end with the tile's last valid
//   row of this expert, so rows of the next expert read zeros.
// Epilogue: thread (u, lane) adds the W tiles in ascending wave order (decode_sum4) and finishes four consecutive columns with gs[e] (null
//   global_scales: no multiply) and bias + e n: invariant_finish4, or finish4_silu_mul (SiLU-mul, SwiGLU-OAI).  C row c_idx[row] (null: row);
//   an index outside [0, c_rows) stores nothing (native_moe_c_row).  Rows of the tile's own expert and columns < n only; vector stores only.
// A row's result is, bit for bit, row 0 of the dense decode kernel with m = 1 and P = 1 on that row: W is a function of k alone, the wave
//   runs and the order of the additions are the same, and the instruction computes a row from that row alone.
//
// Not here: a quantising or rotating gated epilogue; a K split across workgroups; a workgroup that keeps its quantised rows across several
// n-blocks; packed MXFP4 experts and the transient form; any batch-invariance promise beyond the per-row identity above.
#pragma once

#include "gemm_native_decode.hpp"
#include "gemm_native_invariant_moe.hpp"

namespace petit_amd {

struct NativeMoeDecodeArgs {
    void *c;              // [c_rows][n] (gated: [c_rows][n/2]) 16-bit
    const void *a;        // 16-bit [a_rows][k], or the "petit-qact/1" bytes of the m grouped rows
    const void *w;        // the experts' images, back to back
    const float *gs;      // [E], or null: no multiply
    const void *bias;     // [E][n] in c's type, or null
    const int *offsets;   // [E + 1], device
    const int *a_idx;     // [m] or null: the identity (16-bit input only)
    const int *c_idx;     // [m] or null: the identity
    unsigned m, n, k;
    unsigned act;         // PETIT_ACTIVATION_*
    unsigned experts, a_rows, c_rows;
};

// slots of a launch: an m-tile per 32 rows and a partial one per expert that can have rows
PETIT_HD unsigned moe_decode_slots(unsigned m, unsigned num_experts) { return (m + 31u) / 32u + (num_experts < m ? num_experts : m); }

// blockDim.x = 64 W (decode_waves(k / 128, 1)), grid = (n-blocks, slots)
template <class AT, int ACT, bool QIN, bool GATED> __global__ __launch_bounds__(256) void native_moe_decode_kernel(const NativeMoeDecodeArgs p) {
#pragma clang fp contract(off)
    constexpr int NB = GATED ? 2 : 1, NA = native_inv_frag_units<ACT>();
    constexpr unsigned kRowB = native_inv_row_bytes<ACT>();
    __shared__ __attribute__((aligned(16))) float red[kDecodeMaxWaves * NB * 1024];
    const unsigned tid = threadIdx.x, lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = blockDim.x >> 6;
    MoeTile t;
    if (!moe_locate(p.offsets, p.experts, p.m, kDecodeMaxM, blockIdx.y, t))
        return; // a slot past the last tile: workgroup-uniform, before any barrier and any operand load
    // (m0 + rows_valid <= m: the clamp rule keeps every expert's rows inside [0, m))
    const unsigned m0 = t.row0 + (blockIdx.y - t.first) * kDecodeMaxM, rows_valid = min(t.row0 + t.rows - m0, kDecodeMaxM);
    const unsigned ktiles = p.k / kTileK, ks = (unsigned)span_tiles_for_k(p.k);
    const unsigned kt0 = wave * ktiles / waves, kt1 = (wave + 1u) * ktiles / waves, run = kt1 - kt0; // (run >= 1: decode_waves)
    unsigned blk[NB];
    blk[0] = blockIdx.x;
    if constexpr (GATED)
        blk[1] = blockIdx.x + p.n / 64u;

    // the expert's image and the wave's run of each block's stream in it (as the dense kernel's)
    const char *const w_base = (const char *)p.w + (size_t)t.expert * nv6_image_bytes(p.n, p.k);
    const char *const s_base = w_base + nv6_elem_bytes(p.n, p.k);
    __amdgpu_buffer_rsrc_t w_rsrc[NB], s_rsrc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        w_rsrc[nb] = make_rsrc(w_base + ((size_t)blk[nb] * ktiles + kt0) * kNv6TileBytes, run * kNv6TileBytes);
        s_rsrc[nb] = make_rsrc(s_base + (size_t)blk[nb] * ktiles * 128, ktiles * 128);
    }
    // quantised input: the m grouped rows' image, the tile its rows m0 .. m0 + rows_valid - 1
    const unsigned char *const qa = (const unsigned char *)p.a;
    const unsigned char *const qa_hi = qa + qact_hi_offset(p.m, p.k); // (MXFP6; "petit-qact/1": layout.h)
    const unsigned char *const qs = qa + qact_elem_bytes(p.m, p.k, ACT);
    const unsigned qa_m = p.m, qa_m0 = m0, qa_rows = rows_valid;
    // 16-bit input: one descriptor over the caller's matrix (the host keeps a_rows k 2 <= 2^31); a lane without a row starts out of its range
    const __amdgpu_buffer_rsrc_t a16_rsrc = make_rsrc(p.a, QIN ? 0u : p.a_rows * p.k * 2u);
    unsigned a16_voff = 0x80000000u;
    if (!QIN && r < rows_valid) {
        const unsigned src = p.a_idx ? (unsigned)p.a_idx[m0 + r] : m0 + r;
        if (src < p.a_rows)
            a16_voff = src * p.k * 2u + h * (ACT == 8 ? 32u : 64u);
    }
#include "gemm_native_decode_kloop.inc"
    // lane (r, h) holds grouped row m0 + r; register 4 u + i is column 16 (u >> 1) + 8 (u & 1) + 4 h + i of the block's 32
    if (r >= rows_valid)
        return;
    const unsigned crow = native_moe_c_row(p, m0 + r);
    if (crow == ~0u)
        return;
    const float *const gs = p.gs ? p.gs + t.expert : nullptr;
    const void *const bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
    for (unsigned u = wave; u < 4u; u += waves) {
        f32x4 sum[NB];
        decode_sum4<NB>(red, waves, u, lane, sum);
        const unsigned n = blk[0] * 32u + (u >> 1) * 16u + (u & 1u) * 8u + 4u * h; // (n % 32 == 0: every column of the block exists)
        if constexpr (GATED) {
            const unsigned n_half = p.n / 2u;
            const float g = gs ? *gs : 1.0f;
            *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)crow * n_half + n) * 2) = finish4_silu_mul<AT>(sum[0], sum[1], g, bias, n, n_half, p.act);
        } else {
            *reinterpret_cast<uint2 *>((char *)p.c + ((size_t)crow * p.n + n) * 2) = invariant_finish4<AT>(sum[0], gs, bias, n);
        }
    }
}

// one 16-bit type's launches; instantiated by gemm_native_moe_decode_{bf16,f16}.hip
template <class AT, int ACT, bool QIN> void native_moe_decode_launch_fmt(const NativeMoeDecodeArgs &p, hipStream_t stream) {
    const dim3 grid(p.act ? p.n / 64u : p.n / 32u, moe_decode_slots(p.m, p.experts)), block(64u * decode_waves(p.k / kTileK, 1));
    if (p.act)
        hipLaunchKernelGGL((native_moe_decode_kernel<AT, ACT, QIN, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((native_moe_decode_kernel<AT, ACT, QIN, false>), grid, block, 0, stream, p);
}
template <class AT> void native_moe_decode_launch(const NativeMoeDecodeArgs &p, int act_format, bool quantized, hipStream_t stream) {
    if (act_format == 8)
        quantized ? native_moe_decode_launch_fmt<AT, 8, true>(p, stream) : native_moe_decode_launch_fmt<AT, 8, false>(p, stream);
    else if (act_format == 6)
        quantized ? native_moe_decode_launch_fmt<AT, 6, true>(p, stream) : native_moe_decode_launch_fmt<AT, 6, false>(p, stream);
    else
        quantized ? native_moe_decode_launch_fmt<AT, 4, true>(p, stream) : native_moe_decode_launch_fmt<AT, 4, false>(p, stream);
}

} // namespace petit_amd
