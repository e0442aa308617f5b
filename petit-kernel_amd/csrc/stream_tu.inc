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

template <class Cfg> int launch_stream(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    using AT = typename Cfg::AT;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape; // SiLU-mul in the kernel's epilogue needs the gate and the up tile in one wave (dispatch.h act_ok); never a silent no-op
    const unsigned ntiles = args.n / kTileN;
    const unsigned per_wg = Cfg::WN * Cfg::NT;
    dim3 grid((ntiles + per_wg - 1) / per_wg, (args.m + 16 * Cfg::MT - 1) / (16 * Cfg::MT), splitk);
    GemmArgs a = args;
    const unsigned nspans = args.k / (kTileK * Cfg::KS), kparts = splitk * Cfg::WK;
    a.spans_per_wave = (nspans + kparts - 1) / kparts;
    hipLaunchKernelGGL(gemm_stream_kernel<Cfg>, grid, dim3(Cfg::kThreads), 0, stream, a.w, a.s, a.a, a.k, a.n, a.m,
                       a.spans_per_wave, a.act, a.c, a.gs, a.bias, a.workspace);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return splitk > 1 ? launch_splitk_reduce<AT>(args, splitk, stream) : kOk;
}

template <class Cfg> int launch_decode(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    if (splitk > 1 || args.m > (unsigned)Cfg::R)
        return kErrKernelShape;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    const unsigned ntiles = args.n / kTileN;
    const unsigned nspans = args.k / (kTileK * Cfg::KS);
    const unsigned spw = (nspans + Cfg::WK - 1) / Cfg::WK;
    hipLaunchKernelGGL(gemm_decode_kernel<Cfg>, dim3((ntiles + Cfg::NT - 1) / Cfg::NT), dim3(Cfg::kThreads), 0, stream, args.w,
                       args.s, args.a, args.k, args.n, args.m, spw, args.act, args.c, args.gs, args.bias);
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
template <class Cfg> int launch_mid(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    if (splitk > 1 || args.m > (unsigned)Cfg::AM)
        return kErrKernelShape;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    const unsigned ntiles = args.n / kTileN;
    const unsigned per_wg = Cfg::WN * Cfg::NT;
    const unsigned nspans = args.k / (kTileK * Cfg::KS);
    const unsigned spw = (nspans + Cfg::WK - 1) / Cfg::WK;
    hipLaunchKernelGGL(gemm_mid_kernel<Cfg>, dim3((ntiles + per_wg - 1) / per_wg), dim3(Cfg::kThreads), 0, stream, args.w, args.s,
                       args.a, args.k, args.n, args.m, spw, args.act, args.c, args.gs, args.bias, mid_debug_flags());
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// 17 <= M <= 128 (gemm_batch.hpp): grid (n-blocks, m-blocks, K slices); the K slices of one workgroup's WK parts are whole spans
template <class Cfg> int launch_batch(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    using AT = typename Cfg::AT;
    if (args.act && Cfg::NT % 2 != 0)
        return kErrKernelShape;
    if (args.out_format || args.qa)
        return kErrKernelShape;
    const unsigned ntiles = args.n / kTileN;
    const unsigned per_wg = Cfg::WN * Cfg::NT;
    const unsigned nspans = args.k / (kTileK * Cfg::KS);
    const unsigned kparts = (splitk ? splitk : 1u) * Cfg::WK;
    const unsigned spw = (nspans + kparts - 1) / kparts;                              // spans per part
    const unsigned slices = (nspans + spw * Cfg::WK - 1) / (spw * Cfg::WK);           // workgroups along K that own at least one span
    if (slices > 1 && !args.workspace)
        return kErrKernelShape;
    if (args.reduce_act && slices <= 1)
        return kErrSplitCollapsed; // (nothing launched: dispatch.hip runs the kernel unsplit with SiLU-mul in its own epilogue)
    const dim3 grid((ntiles + per_wg - 1) / per_wg, (args.m + Cfg::BM - 1) / Cfg::BM, slices);
    hipLaunchKernelGGL(gemm_batch_kernel<Cfg>, grid, dim3(Cfg::kThreads), 0, stream, args.w, args.s, args.a, args.k, args.n, args.m, spw, args.act,
                       args.c, args.gs, args.bias, args.workspace);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return slices > 1 ? launch_splitk_reduce<AT>(args, slices, stream) : kOk;
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

// K slices of whole spans for the tiled / native kernels: `parts` non-empty slices of `chunk` spans (the last may be shorter).
inline void split_spans(unsigned nspans, unsigned splitk, unsigned *chunk, unsigned *parts) {
    if (splitk > nspans)
        splitk = nspans;
    *chunk = (nspans + splitk - 1) / splitk;
    *parts = (nspans + *chunk - 1) / *chunk;
}

template <class Cfg> int launch_tiled(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    using AT = typename Cfg::AT;
    if (args.act && Cfg::NTW % 2 != 0)
        return kErrKernelShape; // (the epilogue would store nothing: dispatch.h act_ok keeps such a kernel away from SiLU-mul, this is the backstop)
    const unsigned ntiles = args.n / kTileN;
    const unsigned per_wg = Cfg::WAVES * Cfg::NTW;
    GemmArgs a = args;
    a.flags = launch_flags(Cfg::BM, per_wg * kTileN);
    unsigned parts;
    split_spans(args.k / (kTileK * Cfg::KS), splitk, &a.spans_per_wave, &parts);
    if (parts > 1 && !args.workspace)
        return kErrKernelShape;
    if (args.reduce_act && parts <= 1)
        return kErrSplitCollapsed; // (nothing launched: dispatch.hip runs the kernel unsplit with SiLU-mul in its own epilogue)
    dim3 grid((ntiles + per_wg - 1) / per_wg, (args.m + Cfg::BM - 1) / Cfg::BM, parts);
    hipLaunchKernelGGL(gemm_tiled_kernel<Cfg>, grid, dim3(Cfg::kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return parts > 1 ? launch_splitk_reduce<AT>(args, parts, stream) : kOk;
}

template <class Cfg> int launch_wide(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    using AT = typename Cfg::AT;
    const unsigned ntiles = args.n / kTileN;
    const unsigned per_wg = Cfg::WAVES * 2 * Cfg::NP;
    GemmArgs a = args;
    a.flags = launch_flags(Cfg::BM, per_wg * kTileN);
    unsigned parts;
    split_spans(args.k / (kTileK * Cfg::KS), splitk * Cfg::KG, &a.spans_per_wave, &parts);
    parts = (parts + Cfg::KG - 1) / Cfg::KG; // workgroups along K: each walks KG parts (the last may find its second one empty)
    if (parts > 1 && !args.workspace)
        return kErrKernelShape;
    if (args.reduce_act && parts <= 1)
        return kErrSplitCollapsed; // (nothing launched: dispatch.hip runs the kernel unsplit with SiLU-mul in its own epilogue)
    dim3 grid((ntiles + per_wg - 1) / per_wg, (args.m + Cfg::BM - 1) / Cfg::BM, parts);
    hipLaunchKernelGGL(gemm_wide_kernel<Cfg>, grid, dim3(Cfg::kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return parts > 1 ? launch_splitk_reduce<AT>(args, parts, stream) : kOk;
}

template <class Cfg> int launch_shared(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    using AT = typename Cfg::AT;
    if (args.act || args.out_format || args.qa)
        return kErrKernelShape; // (plain / bias epilogue only)
    const unsigned ntiles = args.n / kTileN;
    GemmArgs a = args;
    a.flags = launch_flags(Cfg::BM, 2 * Cfg::NB * kTileN);
    unsigned parts;
    split_spans(args.k / (kTileK * Cfg::KS), splitk, &a.spans_per_wave, &parts);
    if (parts > 1 && !args.workspace)
        return kErrKernelShape;
    if (args.reduce_act && parts <= 1)
        return kErrSplitCollapsed; // (nothing launched: dispatch.hip runs the kernel unsplit with SiLU-mul in its own epilogue)
    dim3 grid((ntiles + 2 * Cfg::NB - 1) / (2 * Cfg::NB), (args.m + Cfg::BM - 1) / Cfg::BM, parts);
    hipLaunchKernelGGL(gemm_shared_kernel<Cfg>, grid, dim3(Cfg::kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return parts > 1 ? launch_splitk_reduce<AT>(args, parts, stream) : kOk;
}

#if defined(PETIT_TU_NATIVE_AT) && PETIT_TU_PART == 5
template <class Cfg> int launch_native(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
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
    const unsigned ntiles = args.n / kTileN;
    const unsigned per_wg = Cfg::WAVES * Cfg::NTW;
    GemmArgs a = args;
    a.flags = launch_flags(Cfg::BM, per_wg * kTileN, 8);
    unsigned parts;
    split_spans(args.k / (kTileK * Cfg::KS), splitk, &a.spans_per_wave, &parts);
    a.workspace = reinterpret_cast<float *>(ws + native_ws_aligned(args.m, args.k));
    if (args.reduce_act && parts <= 1)
        return kErrSplitCollapsed; // (only the quantiser has run: the retry repeats it)
    dim3 grid((ntiles + per_wg - 1) / per_wg, (args.m + Cfg::BM - 1) / Cfg::BM, parts);
    hipLaunchKernelGGL(gemm_native_kernel<Cfg>, grid, dim3(Cfg::kThreads), 0, stream, a, (const unsigned char *)ws);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return parts > 1 ? launch_splitk_reduce<AT>(a, parts, stream) : kOk;
}
template <class Cfg> int launch_native32(const GemmArgs &args, unsigned splitk, hipStream_t stream) {
    using AT = typename Cfg::AT;
    // activations: quantised here into the call's scratch, or handed over already quantised (args.qa, same layout: the
    // output of petit_quantize_activations or of a producer GEMM's quantising epilogue)
    if (args.qa ? args.qa_format != (unsigned)Cfg::ACT : !args.workspace)
        return kErrKernelShape;
    if (args.out_format) { // quantising SiLU-mul epilogue: 256-column workgroup tiles that are all full, no K split
        if (!args.act || Cfg::NP != 2 || Cfg::WAVES != 4 || Cfg::WM != 1 || splitk != 1 || args.n % 512 != 0 ||
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
    const unsigned ntiles = args.n / kTileN;
    const unsigned per_wg = Cfg::WAVES * 2 * Cfg::NP;
    GemmArgs a = args;
    a.flags = launch_flags(Cfg::BM, per_wg * kTileN, Cfg::ACT);
    unsigned parts;
    split_spans(args.k / (kTileK * Cfg::KS), splitk * Cfg::KG, &a.spans_per_wave, &parts);
    parts = (parts + Cfg::KG - 1) / Cfg::KG; // workgroups along K: each walks KG parts (the last may find its second one empty)
    a.workspace = args.qa ? args.workspace : reinterpret_cast<float *>(ws + native_ws_aligned(args.m, args.k));
    if (parts > 1 && !a.workspace)
        return kErrKernelShape;
    if (args.reduce_act && parts <= 1)
        return kErrSplitCollapsed; // (only the quantiser has run: the retry repeats it)
    dim3 grid((ntiles + per_wg - 1) / per_wg, (args.m + Cfg::BM - 1) / Cfg::BM, parts);
    hipLaunchKernelGGL(gemm_native32_kernel<Cfg>, grid, dim3(Cfg::kThreads), 0, stream, a, qa);
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    return parts > 1 ? launch_splitk_reduce<AT>(a, parts, stream) : kOk;
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
#define PETIT_N32(KS, MB, NP, WAVES, D, ACT, KT, PF, WM)                                                                      \
    SolutionEntry{StreamShape{KS, MB * WM, 2 * NP, WAVES, 4 * KT + PF, D, kNative32Am, ACT == 4 ? 2 : ACT == 6 ? 4 : 1, WM}, PETIT_TU_NATIVE_AT::kType, PETIT_TU_NATIVE_FMT, \
                  &launch_native32<Native32Cfg<PETIT_TU_NATIVE_AT, KS, MB, NP, WAVES, D, ACT, KT, PF, WM, 1, 0, PETIT_TU_NATIVE_WF>>},
// two K groups per workgroup (Native32Cfg KG = 2): warp_partition_m nibble 3
#define PETIT_N32K(KS, MB, NP, WAVES, D, ACT, KT, PF)                                                                          \
    SolutionEntry{StreamShape{KS, MB, 2 * NP, WAVES, 4 * KT + PF, D, kNative32Am, ACT == 4 ? 2 : ACT == 6 ? 4 : 1, 3}, PETIT_TU_NATIVE_AT::kType, PETIT_TU_NATIVE_FMT, \
                  &launch_native32<Native32Cfg<PETIT_TU_NATIVE_AT, KS, MB, NP, WAVES, D, ACT, KT, PF, 1, 2, 0, PETIT_TU_NATIVE_WF>>},
// a loader wave stages the activation tiles (Native32Cfg LW = 1): warp_partition_m nibble 4
#define PETIT_N32L(KS, MB, NP, WAVES, D, ACT, KT, PF)                                                                          \
    SolutionEntry{StreamShape{KS, MB, 2 * NP, WAVES, 4 * KT + PF, D, kNative32Am, ACT == 4 ? 2 : ACT == 6 ? 4 : 1, 4}, PETIT_TU_NATIVE_AT::kType, PETIT_TU_NATIVE_FMT, \
                  &launch_native32<Native32Cfg<PETIT_TU_NATIVE_AT, KS, MB, NP, WAVES, D, ACT, KT, PF, 1, 1, 1, PETIT_TU_NATIVE_WF>>},
#define PETIT_N(KS, MT, NTW, WAVES, D)                                                                  \
    SolutionEntry{StreamShape{KS, MT, NTW, WAVES, 1, D, kNativeAm}, PETIT_TU_NATIVE_AT::kType, kFmtMx,  \
                  &launch_native<NativeCfg<PETIT_TU_NATIVE_AT, KS, MT, NTW, WAVES, D>>},
#ifdef PETIT_TU_NV6
#define PETIT_NATIVE_ENTRIES PETIT_NVNATIVE32_SHAPES(PETIT_N32) PETIT_NVNATIVE32_KG_SHAPES(PETIT_N32K)
#else
#define PETIT_NATIVE_ENTRIES PETIT_NATIVE_SHAPES(PETIT_N) PETIT_NATIVE32_SHAPES(PETIT_N32) PETIT_NATIVE32_KG_SHAPES(PETIT_N32K) PETIT_NATIVE32_LW_SHAPES(PETIT_N32L)
#endif
#else
#define PETIT_NATIVE_ENTRIES
#endif

#define PETIT_X(KS, MT, NT, WN, WK, D, AM)                                                   \
    SolutionEntry{StreamShape{KS, MT, NT, WN, WK, D, AM}, PETIT_TU_AT::kType, PETIT_TU_FMT, \
                  &launch_stream<StreamCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NT, WN, WK, D, AM>>, \
                  stream_grouped_fn<StreamCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NT, WN, WK, D, AM>>()},
#define PETIT_P(KS, MT, NT, WN, WK, D, PA)                                                      \
    SolutionEntry{StreamShape{KS, MT, NT, WN, WK, D, 0, PA}, PETIT_TU_AT::kType, PETIT_TU_FMT, \
                  &launch_stream<StreamCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NT, WN, WK, D, 0, 0, PA>>},
#define PETIT_T(KS, MT, NTW, WAVES, D)                                                              \
    SolutionEntry{StreamShape{KS, MT, NTW, WAVES, 1, D, kTiledAm}, PETIT_TU_AT::kType, PETIT_TU_FMT,  \
                  &launch_tiled<TiledCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NTW, WAVES, D>>},
#define PETIT_W(KS, MB, NP, WAVES, D, PF)                                                                  \
    SolutionEntry{StreamShape{KS, MB, 2 * NP, WAVES, 1, D, kWideAm, PF}, PETIT_TU_AT::kType, PETIT_TU_FMT,   \
                  &launch_wide<WideCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MB, NP, WAVES, D, PF>>},
// two K groups per workgroup (WideCfg KG = 2): warp_partition_m nibble 3
#define PETIT_WK2(KS, MB, NP, WAVES, D, PF)                                                                \
    SolutionEntry{StreamShape{KS, MB, 2 * NP, WAVES, 1, D, kWideAm, PF, 3}, PETIT_TU_AT::kType, PETIT_TU_FMT, \
                  &launch_wide<WideCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MB, NP, WAVES, D, PF, 2>>},
// the group-ahead form (WideCfg GA = 1): warp_partition_m nibble 6
#define PETIT_WGA(KS, MB, NP, WAVES, D)                                                                    \
    SolutionEntry{StreamShape{KS, MB, 2 * NP, WAVES, 1, D, kWideAm, 1, 6}, PETIT_TU_AT::kType, PETIT_TU_FMT,  \
                  &launch_wide<WideCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MB, NP, WAVES, D, 1, 1, 1>>},
// W unpacked once per workgroup into LDS (gemm_shared.hpp): the 32x32x16 family's nibble, warp_partition_m nibble 5; tile_m = 8 m32-blocks
// (256 rows), 2 NB n-tiles per workgroup, listed as one "wave" along N
#if !defined(PETIT_TU_NO_GA) && PETIT_TU_PART == 4
#define PETIT_WGA_ENTRIES PETIT_WIDE32_GA_SHAPES(PETIT_WGA)
#else
#define PETIT_WGA_ENTRIES
#endif
#if defined(PETIT_TU_SHARED) && PETIT_TU_PART == 4
#define PETIT_S(KS, NB)                                                                                    \
    SolutionEntry{StreamShape{KS, 8, 2 * NB, 1, 1, 2, kWideAm, 1, 5}, PETIT_TU_AT::kType, PETIT_TU_FMT,     \
                  &launch_shared<SharedCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, NB>>},
#define PETIT_SHARED_ENTRIES PETIT_SHARED_SHAPES(PETIT_S)
#else
#define PETIT_SHARED_ENTRIES
#endif
#if defined(PETIT_TU_DECODE) && PETIT_TU_PART == 3
#define PETIT_G(KS, NT, WK, D, R)                                                                       \
    SolutionEntry{StreamShape{KS, 1, NT, 1, WK, D, kDecodeAm + R, 1, R == 8 ? 2 : 1}, PETIT_TU_AT::kType, PETIT_TU_FMT,     \
                  &launch_decode<DecodeCfg<PETIT_TU_AT, KS, NT, WK, D, R>>, &launch_decode_grouped<DecodeCfg<PETIT_TU_AT, KS, NT, WK, D, R>>},
#define PETIT_DECODE_ENTRIES PETIT_DECODE_SHAPES(PETIT_G)
#else
#define PETIT_DECODE_ENTRIES
#endif
#define PETIT_M(KS, NT, WN, WK, D, AM)                                                                  \
    SolutionEntry{StreamShape{KS, 1, NT, WN, WK, D, AM, 1, 2}, PETIT_TU_AT::kType, PETIT_TU_FMT,         \
                  &launch_mid<MidCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, NT, WN, WK, D, AM>>},
#define PETIT_MID_ENTRIES PETIT_MID_SHAPES(PETIT_M)
#define PETIT_BT(KS, MT, NT, WN, WK, D)                                                                 \
    SolutionEntry{StreamShape{KS, MT, NT, WN, WK, D, 0, 1, 2}, PETIT_TU_AT::kType, PETIT_TU_FMT,         \
                  &launch_batch<BatchCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NT, WN, WK, D>>},
// ... with a loader wave per K part: the activation prefetch distance DA rides in the id's prefetch field (pa = 2 / 4 / 8 for DA = 1 / 2 / 4)
#define PETIT_BTL(KS, MT, NT, WN, WK, D, DA)                                                            \
    SolutionEntry{StreamShape{KS, MT, NT, WN, WK, D, 0, DA == 1 ? 2 : DA == 2 ? 4 : 8, 2}, PETIT_TU_AT::kType, PETIT_TU_FMT, \
                  &launch_batch<BatchCfg<PETIT_TU_AT, PETIT_TU_FMT, KS, MT, NT, WN, WK, D, DA>>},
#if PETIT_TU_PART == 1
const SolutionEntry kTable[] = {PETIT_STREAM_SHAPES(PETIT_X) PETIT_PREFETCH_SHAPES(PETIT_P)};
#elif PETIT_TU_PART == 2
#ifdef PETIT_TU_BFP_AT
#define PETIT_B(KS, NT, WN, WK, D, AM)                                                                 \
    SolutionEntry{StreamShape{KS, 1, NT, WN, WK, D, kBfpAm + AM}, PETIT_TU_AT::kType, PETIT_TU_FMT,   \
                  &launch_stream<StreamCfg<PETIT_TU_BFP_AT, PETIT_TU_FMT, KS, 1, NT, WN, WK, D, AM>>,   \
                  stream_grouped_fn<StreamCfg<PETIT_TU_BFP_AT, PETIT_TU_FMT, KS, 1, NT, WN, WK, D, AM>>()},
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
