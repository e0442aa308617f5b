// Body of the native MoE translation units (gemm_moe_native_<family>.hip): the routed-expert forms (gemm_moe_native.hpp) of a curated set of
// the family's 32x32x64 native kernels, for PETIT_TU_AT and the weight form PETIT_TU_WF (4 = raw MXFP4, 6 = the NV6 image of NVFP4 weights),
// exported as PETIT_TU_MOE_FORMS (solutions.hip attaches them to the table entries of the same shape: no ids of their own).  With
// PETIT_TU_QUANTIZE_ROWS the TU also exports the gathering activation quantiser for PETIT_TU_AT.  Included exactly once per TU.
#include "gemm_moe_native.hpp"
#include "solution.h"

namespace petit_amd {
namespace {

// (geo: the unsplit geometry of the kernel on (m, n, k): solution.h)
template <class Cfg> int launch_native32_moe(const MoeArgs &g, const LaunchGeometry &geo, hipStream_t stream) {
    // the quantising SiLU-mul epilogue: full 256-column workgroup tiles, identity rows (its output is the next launch's grouped input)
    if (g.out_format && (!g.act || g.n % 512 != 0 || g.c_idx || (g.out_format != 8 && g.out_format != 6 && g.out_format != 4)))
        return kErrKernelShape;
    const unsigned slots = moe_slots(g.m, geo.moe_rows(), g.num_experts);
    if (!slots)
        return kErrKernelShape;
    GemmArgs a{};
    a.c = g.c, a.a = g.a, a.w = g.w, a.s = g.s, a.gs = g.gs, a.bias = g.bias, a.act = g.act;
    a.m = g.m, a.n = g.n, a.k = g.k;
    a.spans_per_wave = geo.spans_per_part;       // (one K slice: the whole K range)
    a.qa = g.a, a.qa_format = Cfg::ACT, a.out_format = g.out_format;
    hipLaunchKernelGGL((gemm_native32_kernel<Cfg, Native32MoeLocator<Cfg>>), dim3(geo.grid_x, slots), dim3(Cfg::kThreads), 0,
                       stream, a, (const unsigned char *)g.a, Native32MoeLocator<Cfg>{g.offsets, g.num_experts, g.c_idx, g.c_rows});
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// The 128 x 256 tile (MB = 4, NP = 2, four waves, one K group, no loader wave: the tile the quantising epilogue needs), for every activation
// format at span sizes 8, 4 and 2 (every k % 256 == 0 has a form; Qwen3's down, k = 768, needs KS = 2).  Per (ACT, KS) the entry of the
// family's list (stream_instances.inc) the native arch table picks most; MXFP4 weights have no D = 2 form at KS = 4 with MXFP8 activations.
// Arguments as PETIT_N32: (KS, MB, NP, WAVES, D, ACT, KT, PF, WM).
#define PETIT_MOE_N32(KS, MB, NP, WAVES, D, ACT, KT, PF, WM)                                                                         \
    MoeForm{table_shape<StreamShape{KS, MB * WM, 2 * NP, WAVES, 4 * KT + PF, D, kNative32Am, ACT == 4 ? 2 : ACT == 6 ? 4 : 1, WM}, \
                        32 * MB * WM, 32 * NP * WAVES, 1, true>(),                                                                   \
            &launch_native32_moe<Native32Cfg<PETIT_TU_AT, KS, MB, NP, WAVES, D, ACT, KT, PF, WM, 1, 0, PETIT_TU_WF>>},
#if PETIT_TU_WF == 6
#define PETIT_MOE_N32_KS4_FP8 PETIT_MOE_N32(4, 4, 2, 4, 2, 8, 1, 1, 1)
#else
#define PETIT_MOE_N32_KS4_FP8 PETIT_MOE_N32(4, 4, 2, 4, 4, 8, 1, 1, 1)
#endif
const MoeForm kForms[] = {
    PETIT_MOE_N32(8, 4, 2, 4, 2, 8, 1, 1, 1) PETIT_MOE_N32_KS4_FP8 PETIT_MOE_N32(2, 4, 2, 4, 2, 8, 1, 1, 1)
    PETIT_MOE_N32(8, 4, 2, 4, 2, 6, 2, 2, 1) PETIT_MOE_N32(4, 4, 2, 4, 2, 6, 1, 1, 1) PETIT_MOE_N32(2, 4, 2, 4, 2, 6, 1, 1, 1)
    PETIT_MOE_N32(8, 4, 2, 4, 2, 4, 2, 2, 1) PETIT_MOE_N32(4, 4, 2, 4, 2, 4, 1, 1, 1) PETIT_MOE_N32(2, 4, 2, 4, 2, 4, 1, 1, 1)};

} // namespace

const MoeForm *PETIT_TU_MOE_FORMS(int *count) {
    *count = (int)(sizeof(kForms) / sizeof(kForms[0]));
    return kForms;
}

#ifdef PETIT_TU_QUANTIZE_ROWS
// the gathering quantiser (petit_quantize_activations_rows): row r of the layout from row a_idx[r] of a [a_rows][k]; one workgroup row per
// 1024 (FP8 / FP4) or 8192 (FP6) k of a layout row, all of them along grid x
int PETIT_TU_QUANTIZE_ROWS(const void *a, const int *a_idx, unsigned a_rows, void *qa, unsigned m, unsigned k, int format, hipStream_t stream) {
    if (format != 8 && format != 6 && format != 4)
        return kErrKernelShape;
    const unsigned xb = format == 6 ? (k / 32 + 255) / 256 : (k / 8 + 1023) / 1024;
    if ((uint64_t)xb * m >= (1ull << 31))
        return kErrProblemShape;
    const dim3 grid(xb * m);
    unsigned char *const ws = (unsigned char *)qa;
    const QuantGather g{a_idx, a_rows, xb};
    if (format == 6)
        hipLaunchKernelGGL((quantize_act32_fp6_kernel<PETIT_TU_AT, QuantGather>), grid, dim3(256), 0, stream, a, ws, m, k, g);
    else if (format == 8)
        hipLaunchKernelGGL((quantize_act32_kernel<PETIT_TU_AT, 8, QuantGather>), grid, dim3(256), 0, stream, a, ws, m, k, g);
    else
        hipLaunchKernelGGL((quantize_act32_kernel<PETIT_TU_AT, 4, QuantGather>), grid, dim3(256), 0, stream, a, ws, m, k, g);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}
#endif

} // namespace petit_amd
