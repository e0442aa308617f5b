// gemm_moe_native.hpp -- the routed-expert (MoE) form of the 32x32x64 native kernel (gemm_native32.hpp): all experts of a layer in ONE
// launch on the block-scaled MFMA, activations quantised to MXFP8 / MXFP6 / MXFP4 (petit_gemm_native_moe, include/petit_amd.h).
//
// The activations arrive as ONE quantised matrix of the grouped rows (the k-tile-major layout of gemm_native32.hpp, m = all grouped rows):
// from the gathering quantiser (quantize_act32_kernel with a QuantGather: row r from token row a_idx[r]) or from the quantising SiLU-mul epilogue of the
// gate_up launch.  The grid and the slot -> (expert, m-block) mapping are gemm_tiled_moe_kernel's (gemm_moe.hpp): plain raster over the
// linear workgroup index, the expert's m-blocks fastest, slots past the last tile exit before any load.  The workgroup then runs the dense
// kernel (gemm_native32_kernel with this file's locator) on its expert's operands (64-bit bases) with the layout of the TOTAL rows and the
// row limit of its EXPERT:
//   - an m-block starts at the expert's first grouped row, as a dense call's start at row 0, so within an expert the numbers are those of a
//     dense call on that expert's rows with the same kernel, bit for bit;
//   - tile rows past the expert's end read the next expert's activation rows (or zeros past the layout) and feed only outputs that are not
//     stored -- the next expert's rows belong to another workgroup, so the row limit is a must for every epilogue, not a saving.
// Weights: raw MXFP4 (WF = 4) -- the stacked packed tensors, expert e at e * moe_w_bytes / e * moe_s_bytes; the NV6 image (WF = 6) -- E
// per-expert images back to back (a stacked [E n, k] image is NOT that: its scale region follows all the elements), expert e's at
// e * nv6_image_bytes(n, k), its scales nv6_elem_bytes(n, k) into it.
#pragma once

#include "gemm_moe.hpp"
#include "gemm_native32.hpp"

namespace petit_amd {

// The MoE locator of gemm_native32_kernel<Cfg, Native32MoeLocator<Cfg>> (the kernel's p: the call's arguments with the stacked bases, p.m = total
// grouped rows; its ws: the quantised grouped rows).  c_idx null: the identity (c_rows = p.m).
template <class Cfg> struct Native32MoeLocator {
    const int *offsets;
    unsigned experts;
    const int *c_idx;
    unsigned c_rows;
    static_assert(Cfg::KG == 1 && Cfg::LW == 0, "MoE form: one K group, no loader wave");
    __device__ __forceinline__ bool locate(const GemmArgs &p, unsigned &bn, unsigned &m0, unsigned &m_lim, const void *&w, const void *&s,
                                           const float *&gs, const void *&bias, RowIndex &ix) const {
        const unsigned nb = gridDim.x;
        const unsigned lin = blockIdx.y * nb + blockIdx.x;
        MoeTile t;
        if (!moe_locate(offsets, experts, p.m, Cfg::BM, lin / nb, t))
            return false;
        const unsigned local = lin - t.first * nb;
        bn = local / t.tiles, m0 = t.row0 + (local % t.tiles) * Cfg::BM, m_lim = t.row0 + t.rows;
        if constexpr (Cfg::WF == 6) {
            w = (const char *)p.w + t.expert * nv6_image_bytes(p.n, p.k);
            s = (const char *)w + nv6_elem_bytes(p.n, p.k);
        } else {
            w = (const char *)p.w + t.expert * moe_w_bytes<kFmtMx>(p.n, p.k);
            s = (const char *)p.s + t.expert * moe_s_bytes<kFmtMx>(p.n, p.k);
        }
        gs = p.gs + t.expert;
        bias = p.bias ? (const char *)p.bias + (size_t)t.expert * p.n * 2 : nullptr;
        ix = RowIndex{nullptr, c_idx, 0u, 0u, c_rows};
        return true;
    }
};

} // namespace petit_amd
