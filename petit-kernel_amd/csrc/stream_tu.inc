// Body shared by the per-(dtype, format, part) translation units: instantiate the shapes of stream_instances.inc that belong to
// PETIT_TU_PART for PETIT_TU_AT / PETIT_TU_FMT and export that part of the family's table (solutions.hip concatenates the parts).
// Included exactly once per TU.  Parts (one TU each, so that a full build spreads over the machine's cores):
//   1 streaming kernels with M <= 4 rows staged or fragments straight from L2 (X, P)      2 staged 8 / 16 rows (+ block floating point)
//   3 decode (scale after the MFMA) + shared-tile                                          4 large M: tiled 16x16x32, 32x32x16
//   5 native FP4 MFMA (+ the stand-alone activation quantiser)            6 batched decode, 17 <= M <= 128 (gemm_batch.hpp)
#include <cstdlib>

#include "gemm_stream.hpp"
#include "gemm_tiled.hpp"
#include "gemm_native.hpp"
#include "gemm_wide.hpp"
#include "gemm_shared.hpp"
#include "gemm_native32.hpp"
#include "gemm_decode.hpp"
#include "gemm_mid.hpp"
#include "gemm_batch.hpp"
#include "solution.h"
#include "stream_instances.inc"

namespace petit_amd {
namespace {

template <class AT> int launch_splitk_reduce(const GemmArgs &args, unsigned parts, hipStream_t stream);

// The launchers launch the geometry they are handed (launch_geometry, solution.h: grid, spans per K part, K slices -- decided in plan_gemm) and keep the
// refusals only their Cfg can make.
template <class Cfg> int launch_stream(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    using AT = typename Cfg::AT;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape; // SiLU-mul in the kernel's epilogue needs the gate and the up tile in one wave (dispatch.h act_ok); never a silent no-op
    hipLaunchKernelGGL(gemm_stream_kernel<Cfg>, dim3(geo.grid_x, geo.grid_y, geo.slices), dim3(Cfg::kThreads), 0, stream, args.w, args.s, args.a, args.k,
                       args.n, args.m, geo.spans_per_part, args.act, args.c, args.gs, args.bias, args.workspace);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return geo.slices > 1 ? launch_splitk_reduce<AT>(args, geo.slices, stream) : kOk;
}

template <class Cfg> int launch_decode(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    if (geo.splitk > 1 || args.m > (unsigned)Cfg::R)
        return kErrKernelShape;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    hipLaunchKernelGGL(gemm_decode_kernel<Cfg>, dim3(geo.grid_x), dim3(Cfg::kThreads), 0, stream, args.w,
                       args.s, args.a, args.k, args.n, args.m, geo.spans_per_part, args.act, args.c, args.gs, args.bias);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// grouped launches: the members' grids concatenated along x (gemm_*_grouped_kernel)
template <class Cfg> int launch_stream_grouped(GroupTable g, const void *a, unsigned m, unsigned k, hipStream_t stream) {
    if (m > (unsigned)(Cfg::AM > 0 ? am_rows(Cfg::AM) : 16 * Cfg::MT) || g.count == 0 || g.count > (unsigned)kMaxGroup)
        return kErrKernelShape;
    unsigned total = 0;
    for (unsigned i = 0; i < g.count; ++i) {
        const unsigned per_wg = Cfg::WN * Cfg::NT;
        total += (g.n[i] / kTileN + per_wg - 1) / per_wg;
        g.wg_end[i] = total;
    }
    const unsigned nspans = k / (kTileK * Cfg::KS);
    hipLaunchKernelGGL(gemm_stream_grouped_kernel<Cfg>, dim3(total), dim3(Cfg::kThreads), 0, stream, g, a, k, m, (nspans + Cfg::WK - 1) / Cfg::WK);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}
template <class Cfg> constexpr LaunchGroupedFn stream_grouped_fn() {
    if constexpr (Cfg::AM > 0 && Cfg::MT == 1 && Cfg::ABL == 0)
        return &launch_stream_grouped<Cfg>;
    else
        return nullptr;
}
template <class Cfg> int launch_decode_grouped(GroupTable g, const void *a, unsigned m, unsigned k, hipStream_t stream) {
    if (m > (unsigned)Cfg::R || g.count == 0 || g.count > (unsigned)kMaxGroup)
        return kErrKernelShape;
    unsigned total = 0;
    for (unsigned i = 0; i < g.count; ++i) {
        total += (g.n[i] / kTileN + Cfg::NT - 1) / Cfg::NT;
        g.wg_end[i] = total;
    }
    const unsigned nspans = k / (kTileK * Cfg::KS);
    hipLaunchKernelGGL(gemm_decode_grouped_kernel<Cfg>, dim3(total), dim3(Cfg::kThreads), 0, stream, g, a, k, m, (nspans + Cfg::WK - 1) / Cfg::WK);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

inline unsigned mid_debug_flags() {
#ifndef PETIT_AMD_DEBUG_WAITS
    return 0u; // release builds carry no debug branch in the kernel (gemm_mid.hpp)
#endif
    static const unsigned flags = [] {
        const char *e = getenv("PETIT_AMD_MID_DEBUG");
        return e && *e ? (unsigned)strtoul(e, nullptr, 0) : 0u;
    }();
    return flags;
}
template <class Cfg> int launch_mid(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    if (geo.splitk > 1 || args.m > (unsigned)Cfg::AM)
        return kErrKernelShape;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    hipLaunchKernelGGL(gemm_mid_kernel<Cfg>, dim3(geo.grid_x), dim3(Cfg::kThreads), 0, stream, args.w, args.s,
                       args.a, args.k, args.n, args.m, geo.spans_per_part, args.act, args.c, args.gs, args.bias, mid_debug_flags());
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// 17 <= M <= 128 (gemm_batch.hpp): grid (n-blocks, m-blocks, K slices); the K slices of one workgroup's WK parts are whole spans
template <class Cfg> int launch_batch(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    using AT = typename Cfg::AT;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    if (args.out_format || args.qa)
        return kErrKernelShape;
    if (geo.slices > 1 && !args.workspace)
        return kErrKernelShape;
    hipLaunchKernelGGL(gemm_batch_kernel<Cfg>, dim3(geo.grid_x, geo.grid_y, geo.slices), dim3(Cfg::kThreads), 0, stream, args.w, args.s, args.a, args.k,
                       args.n, args.m, geo.spans_per_part, args.act, args.c, args.gs, args.bias, args.workspace);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return geo.slices > 1 ? launch_splitk_reduce<AT>(args, geo.slices, stream) : kOk;
}

// Second pass of a cross-workgroup K split (fixed summation order: deterministic).
template <class AT> int launch_splitk_reduce(const GemmArgs &args, unsigned parts, hipStream_t stream) {
    const size_t total4 = (size_t)args.m * args.n / (args.reduce_act ? 8 : 4);
    size_t blocks = (total4 + 255) / 256;
    if (blocks > 2048)
        blocks = 2048;
    if (args.reduce_act) {
        hipLaunchKernelGGL(splitk_reduce_silu_kernel<AT>, dim3((unsigned)blocks), dim3(256), 0, stream, args.c, args.workspace,
                           args.gs, args.bias, args.m, args.n, parts, args.reduce_act);
        return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
    }
    hipLaunchKernelGGL(splitk_reduce_kernel<AT>, dim3((unsigned)blocks), dim3(256), 0, stream, args.c, args.workspace,
                       args.gs, args.bias, args.m, args.n, parts);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// Launch flags of the large-M kernels (device_common.hpp: stagger_priority, tile_of_block).  On by default;
// $PETIT_AMD_LARGEM_FLAGS=<bits> overrides (A/B measurements: 0 = round-1 behaviour, 1 = priority only, 2 = raster only).
// The raster band (m-tiles per band) balances what the 32 tiles an XCD runs at a time pull into its L2 per k-step:
// ph A panels of bm rows x a_bits per element against 32 / ph W panels of bn columns x 4.5 bits (nibbles + scales).
// $PETIT_AMD_RASTER_BAND=<n> overrides (0 = whole columns, the round-2..4 order).
inline unsigned launch_flags(unsigned bm, unsigned bn, unsigned a_bits = 16) {
    static const unsigned flags = [] {
        const char *e = getenv("PETIT_AMD_LARGEM_FLAGS");
        return e && *e ? (unsigned)strtoul(e, nullptr, 0) : (kFlagPrio | kFlagXcdRaster);
    }();
    static const int band_override = [] {
        const char *e = getenv("PETIT_AMD_RASTER_BAND");
        return e && *e ? (int)strtol(e, nullptr, 0) : -1;
    }();
    unsigned ph = 1;
    if (band_override >= 0) {
        ph = (unsigned)band_override & 0xffu;
    } else {
        unsigned long best = ~0ul;
        for (unsigned c = 1; c <= 32; c *= 2) {
            const unsigned long cost = 2ul * c * bm * a_bits + 9ul * (32 / c) * bn; // (twice the bits per k of the 32 tiles)
            if (cost < best)
                best = cost, ph = c;
        }
    }
    return flags | (ph << kFlagBandShift);
}

// the large-M kernels (GemmArgs by value): the planned grid, its spans per part and the raster flags of the tile; a_bits as launch_flags.  (The reduce pass
// of a K split stays with each launcher: called from here, the kernels are emitted in another order.)
template <class Kernel, class... Extra>
int launch_large(Kernel kernel, unsigned threads, const GemmArgs &args, const LaunchGeometry &geo, unsigned a_bits, hipStream_t stream, Extra... extra) {
    if (geo.slices > 1 && !args.workspace)
        return kErrKernelShape;
    GemmArgs a = args;
    a.flags = launch_flags(geo.bm, geo.bn, a_bits);
    a.spans_per_wave = geo.spans_per_part;
    hipLaunchKernelGGL(kernel, dim3(geo.grid_x, geo.grid_y, geo.slices), dim3(threads), 0, stream, a, extra...);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

template <class Cfg> int launch_tiled(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    if (args.act && Cfg::NTW % 2 != 0)
        return kErrKernelShape; // (the epilogue would store nothing: dispatch.h act_ok keeps such a kernel away from SiLU-mul, this is the backstop)
    const int rc = launch_large(gemm_tiled_kernel<Cfg>, Cfg::kThreads, args, geo, 16, stream);
    return rc == kOk && geo.slices > 1 ? launch_splitk_reduce<typename Cfg::AT>(args, geo.slices, stream) : rc;
}

template <class Cfg> int launch_wide(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    const int rc = launch_large(gemm_wide_kernel<Cfg>, Cfg::kThreads, args, geo, 16, stream);
    return rc == kOk && geo.slices > 1 ? launch_splitk_reduce<typename Cfg::AT>(args, geo.slices, stream) : rc;
}

template <class Cfg> int launch_shared(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    if (args.act || args.out_format || args.qa)
        return kErrKernelShape; // (plain / bias epilogue only)
    const int rc = launch_large(gemm_shared_kernel<Cfg>, Cfg::kThreads, args, geo, 16, stream);
    return rc == kOk && geo.slices > 1 ? launch_splitk_reduce<typename Cfg::AT>(args, geo.slices, stream) : rc;
}

#if defined(PETIT_TU_NATIVE_AT) && PETIT_TU_PART == 5
template <class Cfg> int launch_native(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    using AT = typename Cfg::AT;
    if (!args.workspace || args.qa || args.out_format)
        return kErrKernelShape; // (pre-quantised input / quantised output are the 32x32x64 kernels' interface)
    if (args.act && Cfg::NTW % 2 != 0)
        return kErrKernelShape; // (ADVICE r04: this kernel's SiLU-mul epilogue exists for even NTW only; it returned kOk with C unwritten)
    // workspace: [quantised activations + their scales | fp32 slabs of a K split]  (dispatch.hip sizes it: workspace_need)
    unsigned char *ws = reinterpret_cast<unsigned char *>(args.workspace);
    const size_t units = (size_t)args.m * (args.k / 8);
    size_t blocks = (units + 255) / 256;
    if (blocks > 4096)
        blocks = 4096;
    hipLaunchKernelGGL(quantize_act_kernel<AT>, dim3((unsigned)blocks), dim3(256), 0, stream, args.a, ws, args.m, args.k);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    GemmArgs a = args;
    a.workspace = reinterpret_cast<float *>(ws + native_ws_aligned(args.m, args.k));
    const int rc = launch_large(gemm_native_kernel<Cfg>, Cfg::kThreads, a, geo, 8, stream, (const unsigned char *)ws);
    return rc == kOk && geo.slices > 1 ? launch_splitk_reduce<AT>(a, geo.slices, stream) : rc;
}
template <class Cfg> int launch_native32(const GemmArgs &args, const LaunchGeometry &geo, hipStream_t stream) {
    using AT = typename Cfg::AT;
    // activations: quantised here into the call's scratch, or handed over already quantised (args.qa, same layout: the
    // output of petit_quantize_activations or of a producer GEMM's quantising epilogue)
    if (args.qa ? args.qa_format != (unsigned)Cfg::ACT : !args.workspace)
        return kErrKernelShape;
    if (args.out_format) { // quantising SiLU-mul epilogue: 256-column workgroup tiles that are all full, no K split
        if (!args.act || Cfg::NP != 2 || Cfg::WAVES != 4 || Cfg::WM != 1 || geo.splitk != 1 || args.n % 512 != 0 ||
            (args.out_format != 8 && args.out_format != 6 && args.out_format != 4))
            return kErrKernelShape;
    }
    // workspace: [quantised activations + their scales | fp32 slabs of a K split]  (sized for the FP8 form: dispatch.hip workspace_need)
    unsigned char *ws = reinterpret_cast<unsigned char *>(args.workspace);
    const unsigned char *qa = reinterpret_cast<const unsigned char *>(args.qa);
    if (!qa) {
        if (args.m > 65535)
            return kErrKernelShape; // (one grid row per activation row)
        if constexpr (Cfg::ACT == 6)
            hipLaunchKernelGGL(quantize_act32_fp6_kernel<AT>, dim3((args.k / 32 + 255) / 256, args.m), dim3(256), 0, stream, args.a, ws, args.m, args.k);
        else
            hipLaunchKernelGGL((quantize_act32_kernel<AT, Cfg::ACT>), dim3((args.k / 8 + 1023) / 1024, args.m), dim3(256), 0, stream, args.a, ws,
                               args.m, args.k);
        if (hipGetLastError() != hipSuccess)
            return kErrLaunch;
        qa = ws;
    }
    GemmArgs a = args;
    a.workspace = args.qa ? args.workspace : reinterpret_cast<float *>(ws + native_ws_aligned(args.m, args.k));
    void (*const kernel)(GemmArgs, const unsigned char *) = gemm_native32_kernel<Cfg>; // (the dense form: no MoE locator)
    const int rc = launch_large(kernel, Cfg::kThreads, a, geo, Cfg::ACT, stream, qa);
    return rc == kOk && geo.slices > 1 ? launch_splitk_reduce<AT>(a, geo.slices, stream) : rc;
}
// the stand-alone quantiser of the 32x32x64 kernels' activation layout (petit_quantize_activations)
template <class AT> int launch_quantize32(const void *a, void *qa, unsigned m, unsigned k, int format, hipStream_t stream) {
    if (m > 65535 || (format != 8 && format != 6 && format != 4))
        return kErrKernelShape;
    const dim3 grid((k / 8 + 1023) / 1024, m);
    if (format == 6)
        hipLaunchKernelGGL(quantize_act32_fp6_kernel<AT>, dim3((k / 32 + 255) / 256, m), dim3(256), 0, stream, a, (unsigned char *)qa, m, k);
    else if (format == 8)
        hipLaunchKernelGGL((quantize_act32_kernel<AT, 8>), grid, dim3(256), 0, stream, a, (unsigned char *)qa, m, k);
    else
        hipLaunchKernelGGL((quantize_act32_kernel<AT, 4>), grid, dim3(256), 0, stream, a, (unsigned char *)qa, m, k);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}
// (id: the pa field packs ACT, KT and PF: pa = 1 / 2 = MXFP8 / MXFP4 activations with KT = PF = 1; 4 / 8 = the same with the
//  KT x PF given in warp_partition_k: wk = 1 + 2 (KT - 1) + (PF - 1) ... kept simple: wk carries 4 KT + PF)
// PETIT_TU_NV6 (gemm_nv_*_p5.hip): the same kernels on the MFMA-native image of NVFP4 weights (Native32Cfg WF = 6; nvnative.hip) -- the family's
// element_b nibble tells the ids apart
#ifdef PETIT_TU_NV6
#define PETIT_TU_NATIVE_FMT kFmtNv
#define PETIT_TU_NATIVE_WF 6
#else
#define PETIT_TU_NATIVE_FMT kFmtMx
#define PETIT_TU_NATIVE_WF 4
#endif
// The table entries, here and below: kernel Cfg, the shape its id spells, and -- stated once, at compile time (table_shape, solution.h) -- that the rows
// and columns per workgroup and the in-workgroup K parts the host reads from that shape are the Cfg's own; then activation type, format and launchers.
#define PETIT_N32_CFG(KS_, MB_, NP_, WAVES_, D_, ACT_, KT_, PF_, WM_, KG_, LW_, WM_NIBBLE_)                                                  \
    ([] { \
        using Cfg = Native32Cfg<PETIT_TU_NATIVE_AT, KS_, MB_, NP_, WAVES_, D_, ACT_, KT_, PF_, WM_, KG_, LW_, PETIT_TU_NATIVE_WF>; \
        return SolutionEntry{table_shape<StreamShape{KS_, MB_ * WM_, 2 * NP_, WAVES_, 4 * KT_ + PF_, D_, kNative32Am, ACT_ == 4 ? 2 : ACT_ == 6 ? 4 : 1, WM_NIBBLE_}, Cfg::BM, 32 * Cfg::NP * Cfg::WAVES, Cfg::KG>(), \
                             PETIT_TU_NATIVE_AT::kType, PETIT_TU_NATIVE_FMT, &launch_native32<Cfg>}; \
    }()),
#define PETIT_N32(KS, MB, NP, WAVES, D, ACT, KT, PF, WM) PETIT_N32_CFG(KS, MB, NP, WAVES, D, ACT, KT, PF, WM, 1, 0, WM)
// two K groups per workgroup (Native32Cfg KG = 2): warp_partition_m nibble 3
#define PETIT_N32K(KS, MB, NP, WAVES, D, ACT, KT, PF) PETIT_N32_CFG(KS, MB, NP, WAVES, D, ACT, KT, PF, 1, 2, 0, 3)
// a loader wave stages the activation tiles (Native32Cfg LW = 1): warp_partition_m nibble 4
#define PETIT_N32L(KS, MB, NP, WAVES, D, ACT, KT, PF) PETIT_N32_CFG(KS, MB, NP, WAVES, D, ACT, KT, PF, 1, 1, 1, 4)
#define PETIT_N(KS_, MT_, NTW_, WAVES_, D_)                                                                                      \
    ([] { \
        using Cfg = NativeCfg<PETIT_TU_NATIVE_AT, KS_, MT_, NTW_, WAVES_, D_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, MT_, NTW_, WAVES_, 1, D_, kNativeAm}, Cfg::BM, 16 * Cfg::WAVES * Cfg::NTW, 1>(), \
                             PETIT_TU_NATIVE_AT::kType, kFmtMx, &launch_native<Cfg>}; \
    }()),
#ifdef PETIT_TU_NV6
#define PETIT_NATIVE_ENTRIES PETIT_NVNATIVE32_SHAPES(PETIT_N32) PETIT_NVNATIVE32_KG_SHAPES(PETIT_N32K)
#else
#define PETIT_NATIVE_ENTRIES PETIT_NATIVE_SHAPES(PETIT_N) PETIT_NATIVE32_SHAPES(PETIT_N32) PETIT_NATIVE32_KG_SHAPES(PETIT_N32K) PETIT_NATIVE32_LW_SHAPES(PETIT_N32L)
#endif
#else
#define PETIT_NATIVE_ENTRIES
#endif

#define PETIT_X(KS_, MT_, NT_, WN_, WK_, D_, AM_)                                                                                          \
    ([] { \
        using Cfg = StreamCfg<PETIT_TU_AT, PETIT_TU_FMT, KS_, MT_, NT_, WN_, WK_, D_, AM_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, MT_, NT_, WN_, WK_, D_, AM_}, 16 * Cfg::MT, 16 * Cfg::WN * Cfg::NT, Cfg::WK>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_stream<Cfg>, stream_grouped_fn<Cfg>()}; \
    }()),
#define PETIT_P(KS_, MT_, NT_, WN_, WK_, D_, PA_)                                                                                                 \
    ([] { \
        using Cfg = StreamCfg<PETIT_TU_AT, PETIT_TU_FMT, KS_, MT_, NT_, WN_, WK_, D_, 0, 0, PA_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, MT_, NT_, WN_, WK_, D_, 0, PA_}, 16 * Cfg::MT, 16 * Cfg::WN * Cfg::NT, Cfg::WK>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_stream<Cfg>}; \
    }()),
#define PETIT_T(KS_, MT_, NTW_, WAVES_, D_)                                                                                               \
    ([] { \
        using Cfg = TiledCfg<PETIT_TU_AT, PETIT_TU_FMT, KS_, MT_, NTW_, WAVES_, D_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, MT_, NTW_, WAVES_, 1, D_, kTiledAm}, Cfg::BM, 16 * Cfg::WAVES * Cfg::NTW, 1>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_tiled<Cfg>}; \
    }()),
#define PETIT_WIDE_CFG(KS_, MB_, NP_, WAVES_, D_, PF_, KG_, GA_, WM_NIBBLE_)                                                                      \
    ([] { \
        using Cfg = WideCfg<PETIT_TU_AT, PETIT_TU_FMT, KS_, MB_, NP_, WAVES_, D_, PF_, KG_, GA_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, MB_, 2 * NP_, WAVES_, 1, D_, kWideAm, PF_, WM_NIBBLE_}, Cfg::BM, Cfg::BN, Cfg::KG>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_wide<Cfg>}; \
    }()),
#define PETIT_W(KS, MB, NP, WAVES, D, PF) PETIT_WIDE_CFG(KS, MB, NP, WAVES, D, PF, 1, 0, 1)
// two K groups per workgroup (WideCfg KG = 2): warp_partition_m nibble 3
#define PETIT_WK2(KS, MB, NP, WAVES, D, PF) PETIT_WIDE_CFG(KS, MB, NP, WAVES, D, PF, 2, 0, 3)
// the group-ahead form (WideCfg GA = 1): warp_partition_m nibble 6
#define PETIT_WGA(KS, MB, NP, WAVES, D) PETIT_WIDE_CFG(KS, MB, NP, WAVES, D, 1, 1, 1, 6)
// W unpacked once per workgroup into LDS (gemm_shared.hpp): the 32x32x16 family's nibble, warp_partition_m nibble 5; tile_m = 8 m32-blocks
// (256 rows), 2 NB n-tiles per workgroup, listed as one "wave" along N
#if !defined(PETIT_TU_NO_GA) && PETIT_TU_PART == 4
#define PETIT_WGA_ENTRIES PETIT_WIDE32_GA_SHAPES(PETIT_WGA)
#else
#define PETIT_WGA_ENTRIES
#endif
#if defined(PETIT_TU_SHARED) && PETIT_TU_PART == 4
#define PETIT_S(KS_, NB_)                                                                                                            \
    ([] { \
        using Cfg = SharedCfg<PETIT_TU_AT, PETIT_TU_FMT, KS_, NB_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, 8, 2 * NB_, 1, 1, 2, kWideAm, 1, 5}, Cfg::BM, Cfg::BN, 1>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_shared<Cfg>}; \
    }()),
#define PETIT_SHARED_ENTRIES PETIT_SHARED_SHAPES(PETIT_S)
#else
#define PETIT_SHARED_ENTRIES
#endif
#if defined(PETIT_TU_DECODE) && PETIT_TU_PART == 3
#define PETIT_G(KS_, NT_, WK_, D_, R_)                                                                                                      \
    ([] { \
        using Cfg = DecodeCfg<PETIT_TU_AT, KS_, NT_, WK_, D_, R_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, 1, NT_, 1, WK_, D_, kDecodeAm + R_, 1, R_ == 8 ? 2 : 1}, 16, 16 * Cfg::NT, Cfg::WK>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_decode<Cfg>, &launch_decode_grouped<Cfg>}; \
    }()),
#define PETIT_DECODE_ENTRIES PETIT_DECODE_SHAPES(PETIT_G)
#else
#define PETIT_DECODE_ENTRIES
#endif
#define PETIT_M(KS_, NT_, WN_, WK_, D_, AM_)                                                                                             \
    ([] { \
        using Cfg = MidCfg<PETIT_TU_AT, PETIT_TU_FMT, KS_, NT_, WN_, WK_, D_, AM_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, 1, NT_, WN_, WK_, D_, AM_, 1, 2}, 16, 16 * Cfg::WN * Cfg::NT, Cfg::WK>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_mid<Cfg>}; \
    }()),
#define PETIT_MID_ENTRIES PETIT_MID_SHAPES(PETIT_M)
#define PETIT_BATCH_CFG(KS_, MT_, NT_, WN_, WK_, D_, DA_, PA_)                                                                                  \
    ([] { \
        using Cfg = BatchCfg<PETIT_TU_AT, PETIT_TU_FMT, KS_, MT_, NT_, WN_, WK_, D_, DA_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, MT_, NT_, WN_, WK_, D_, 0, PA_, 2}, Cfg::BM, 16 * Cfg::WN * Cfg::NT, Cfg::WK>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_batch<Cfg>}; \
    }()),
#define PETIT_BT(KS, MT, NT, WN, WK, D) PETIT_BATCH_CFG(KS, MT, NT, WN, WK, D, 0, 1)
// ... with a loader wave per K part: the activation prefetch distance DA rides in the id's prefetch field (pa = 2 / 4 / 8 for DA = 1 / 2 / 4)
#define PETIT_BTL(KS, MT, NT, WN, WK, D, DA) PETIT_BATCH_CFG(KS, MT, NT, WN, WK, D, DA, DA == 1 ? 2 : DA == 2 ? 4 : 8)
#if PETIT_TU_PART == 1
const SolutionEntry kTable[] = {PETIT_STREAM_SHAPES(PETIT_X) PETIT_PREFETCH_SHAPES(PETIT_P)};
#elif PETIT_TU_PART == 2
#ifdef PETIT_TU_BFP_AT
#define PETIT_B(KS_, NT_, WN_, WK_, D_, AM_)                                                                                              \
    ([] { \
        using Cfg = StreamCfg<PETIT_TU_BFP_AT, PETIT_TU_FMT, KS_, 1, NT_, WN_, WK_, D_, AM_>; \
        return SolutionEntry{table_shape<StreamShape{KS_, 1, NT_, WN_, WK_, D_, kBfpAm + AM_}, 16 * Cfg::MT, 16 * Cfg::WN * Cfg::NT, Cfg::WK>(), \
                             PETIT_TU_AT::kType, PETIT_TU_FMT, &launch_stream<Cfg>, stream_grouped_fn<Cfg>()}; \
    }()),
const SolutionEntry kTable[] = {PETIT_WIDE_SHAPES(PETIT_X) PETIT_BFP_SHAPES(PETIT_B)};
#undef PETIT_B
#else
const SolutionEntry kTable[] = {PETIT_WIDE_SHAPES(PETIT_X)};
#endif
#elif PETIT_TU_PART == 3
const SolutionEntry kTable[] = {PETIT_DECODE_ENTRIES PETIT_MID_ENTRIES};
#elif PETIT_TU_PART == 4
const SolutionEntry kTable[] = {PETIT_TILED_SHAPES(PETIT_T) PETIT_WIDE32_SHAPES(PETIT_W) PETIT_WIDE32_KG_SHAPES(PETIT_WK2) PETIT_WGA_ENTRIES PETIT_SHARED_ENTRIES};
#elif PETIT_TU_PART == 5
const SolutionEntry kTable[] = {PETIT_NATIVE_ENTRIES};
#elif PETIT_TU_PART == 6
#ifdef PETIT_TU_BATCH_LW_ONLY
const SolutionEntry kTable[] = {PETIT_BATCH_LW_SHAPES(PETIT_BTL)};
#else
const SolutionEntry kTable[] = {PETIT_BATCH_SHAPES(PETIT_BT) PETIT_BATCH_LW_SHAPES(PETIT_BTL)};
#endif
#else
#error "PETIT_TU_PART must be 1 .. 6"
#endif
#undef PETIT_W
#undef PETIT_X
#undef PETIT_P
#undef PETIT_T

} // namespace

#define PETIT_TU_CAT2(a, b) a##_p##b
#define PETIT_TU_CAT(a, b) PETIT_TU_CAT2(a, b)
const SolutionEntry *PETIT_TU_CAT(PETIT_TU_TABLE, PETIT_TU_PART)(int *count) {
    *count = (int)(sizeof(kTable) / sizeof(kTable[0]));
    return kTable;
}
#if defined(PETIT_TU_QUANTIZE) && PETIT_TU_PART == 5
int PETIT_TU_QUANTIZE(const void *a, void *qa, unsigned m, unsigned k, int format, hipStream_t stream) {
    return launch_quantize32<PETIT_TU_NATIVE_AT>(a, qa, m, k, format, stream);
}
#endif

} // namespace petit_amd
