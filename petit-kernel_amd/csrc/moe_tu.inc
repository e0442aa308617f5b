// Body of the MoE translation units (gemm_moe_<family>.hip): the MoE forms (gemm_moe.hpp) of the family's decode, staged streaming and
// tiled kernels, for PETIT_TU_AT / PETIT_TU_FMT, exported as moe_forms_<family> (solutions.hip attaches them to the
// table entries of the same shape).  Included exactly once per TU.  With PETIT_TU_MOE_INDEXED (gemm_moe_idx_<family>.hip) the same
// list of shapes gets the indexed forms instead (gathered A rows, scattered C rows: gemm_moe.hpp), exported as moe_idx_forms_<family>:
// every kernel with a MoE form has an indexed one, and the pick is shared.
#include "gemm_moe.hpp"
#include "solution.h"
#include "stream_instances.inc"

namespace petit_amd {
namespace {

#ifdef PETIT_TU_MOE_INDEXED
constexpr bool kIndexed = true;
#else
constexpr bool kIndexed = false;
#endif
RowIndex row_index(const MoeArgs &g) { return RowIndex{g.a_idx, g.c_idx, 0u, g.a_rows, g.c_rows}; }

// (geo: the unsplit geometry of the kernel on (m, n, k) -- rows per workgroup, workgroups along N, the one K slice's spans per part: solution.h)
template <class Cfg> int launch_stream_moe(const MoeArgs &g, const LaunchGeometry &geo, hipStream_t stream) {
    if (g.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    const unsigned slots = moe_slots(g.m, geo.moe_rows(), g.num_experts);
    if (!slots)
        return kErrKernelShape;
    if constexpr (kIndexed)
        hipLaunchKernelGGL(gemm_stream_moe_idx_kernel<Cfg>, dim3(geo.grid_x, slots), dim3(Cfg::kThreads), 0, stream, g.w, g.s, g.a,
                           g.k, g.n, g.m, geo.spans_per_part, g.act, g.c, g.gs, g.bias, g.offsets, g.num_experts, row_index(g));
    else
        hipLaunchKernelGGL(gemm_stream_moe_kernel<Cfg>, dim3(geo.grid_x, slots), dim3(Cfg::kThreads), 0, stream, g.w, g.s, g.a,
                           g.k, g.n, g.m, geo.spans_per_part, g.act, g.c, g.gs, g.bias, g.offsets, g.num_experts);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

template <class Cfg> int launch_decode_moe(const MoeArgs &g, const LaunchGeometry &geo, hipStream_t stream) {
    if (g.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    const unsigned slots = moe_slots(g.m, geo.moe_rows(), g.num_experts);
    if (!slots)
        return kErrKernelShape;
    if constexpr (kIndexed)
        hipLaunchKernelGGL(gemm_decode_moe_idx_kernel<Cfg>, dim3(geo.grid_x, slots), dim3(Cfg::kThreads), 0, stream, g.w, g.s,
                           g.a, g.k, g.n, g.m, geo.spans_per_part, g.act, g.c, g.gs, g.bias, g.offsets, g.num_experts, row_index(g));
    else
        hipLaunchKernelGGL(gemm_decode_moe_kernel<Cfg>, dim3(geo.grid_x, slots), dim3(Cfg::kThreads), 0, stream, g.w, g.s,
                           g.a, g.k, g.n, g.m, geo.spans_per_part, g.act, g.c, g.gs, g.bias, g.offsets, g.num_experts);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

template <class Cfg> int launch_tiled_moe(const MoeArgs &g, const LaunchGeometry &geo, hipStream_t stream) {
    if (g.act && Cfg::NTW % 2 != 0)
        return kErrKernelShape;
    const unsigned slots = moe_slots(g.m, geo.moe_rows(), g.num_experts);
    if (!slots)
        return kErrKernelShape;
    GemmArgs a{};
    a.c = g.c, a.a = g.a, a.w = g.w, a.s = g.s, a.gs = g.gs, a.bias = g.bias, a.act = g.act;
    a.m = g.m, a.n = g.n, a.k = g.k;
    a.spans_per_wave = geo.spans_per_part;       // (one K slice: the whole K range)
    a.flags = kFlagPrio;                         // (the raster order is the MoE kernel's own: no XCD raster bits)
    if constexpr (kIndexed)
        hipLaunchKernelGGL(gemm_tiled_moe_idx_kernel<Cfg>, dim3(geo.grid_x, slots), dim3(Cfg::kThreads), 0, stream, a, g.offsets,
                           g.num_experts, row_index(g));
    else
        hipLaunchKernelGGL(gemm_tiled_moe_kernel<Cfg>, dim3(geo.grid_x, slots), dim3(Cfg::kThreads), 0, stream, a, g.offsets,
                           g.num_experts);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// Which kernels have a MoE form: every decode kernel and every staged streaming kernel of the M <= 4 list (stream_instances.inc: what the
// arch tables pick for 1 to 4 rows), the 8- and 16-row staged kernels the tables pick most, and tiled kernels of 32, 64 and 128 rows per
// span size.  Forms for every kernel with a grouped form and every tiled kernel made a full build 41 % longer; this set
// costs about 7 %.  Shapes as the table entries of stream_tu.inc spell them; a shape without a MoE form (direct path, MT > 1) gives a null launcher.
template <class Cfg> constexpr LaunchMoeFn stream_moe_fn() {
    if constexpr (Cfg::AM > 0 && Cfg::MT == 1 && Cfg::ABL == 0)
        return &launch_stream_moe<Cfg>;
    else
        return nullptr;
}
#define PETIT_MOE_X(KS, MT, NT, WN, WK, D, AM) \
    MoeForm{table_shape<StreamShape{KS, MT, NT, WN, WK, D, AM}, AM ? AM : 16 * MT, 16 * WN * NT, WK, true>(),                                      \
            stream_moe_fn<StreamCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NT, WN, WK, D, AM>>()},
#define PETIT_MOE_G(KS, NT, WK, D, R) \
    MoeForm{table_shape<StreamShape{KS, 1, NT, 1, WK, D, kDecodeAm + R, 1, R == 8 ? 2 : 1}, R, 16 * NT, WK, true>(),                               \
            &launch_decode_moe<DecodeCfg<PETIT_TU_AT, KS, NT, WK, D, R>>},
#define PETIT_MOE_T(KS, MT, NTW, WAVES, D) \
    MoeForm{table_shape<StreamShape{KS, MT, NTW, WAVES, 1, D, kTiledAm}, TiledCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NTW, WAVES, D>::BM, 16 * WAVES * NTW, 1, true>(), \
            &launch_tiled_moe<TiledCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NTW, WAVES, D>>},

// (a subset of PETIT_WIDE_SHAPES)
#define PETIT_MOE_WIDE_SHAPES(X) \
    X(8, 1, 1, 1, 8, 8, 16)      \
    X(8, 1, 2, 1, 4, 8, 16)      \
    X(8, 1, 4, 1, 4, 4, 16)      \
    X(8, 1, 1, 1, 8, 8, 8)       \
    X(8, 1, 2, 1, 4, 4, 8)       \
    X(4, 1, 2, 1, 4, 4, 16)      \
    X(2, 1, 2, 1, 4, 2, 16)
// (a subset of PETIT_TILED_SHAPES)
#define PETIT_MOE_TILED_SHAPES(T) \
    T(8, 2, 4, 4, 2)              \
    T(8, 4, 4, 4, 2)              \
    T(8, 8, 2, 4, 2)              \
    T(8, 8, 4, 4, 2)              \
    T(4, 4, 2, 4, 2)              \
    T(4, 8, 2, 4, 2)              \
    T(2, 4, 2, 4, 2)              \
    T(2, 8, 4, 4, 2)

#ifdef PETIT_TU_DECODE
#define PETIT_MOE_DECODE_ENTRIES PETIT_DECODE_SHAPES(PETIT_MOE_G)
#else
#define PETIT_MOE_DECODE_ENTRIES
#endif
const MoeForm kForms[] = {PETIT_MOE_DECODE_ENTRIES PETIT_STREAM_SHAPES(PETIT_MOE_X) PETIT_MOE_WIDE_SHAPES(PETIT_MOE_X) PETIT_MOE_TILED_SHAPES(PETIT_MOE_T)};

} // namespace

const MoeForm *PETIT_TU_MOE_FORMS(int *count) {
    *count = (int)(sizeof(kForms) / sizeof(kForms[0]));
    return kForms;
}

} // namespace petit_amd
