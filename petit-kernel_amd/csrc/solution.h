// solution.h -- 64-bit solution ids and the kernel table of libpetit_amd.so.
//
// Ids keep the bit layout of the reference's SolutionId bitfield
// (lib/gemm/rocm/quantization/gemm.h:33-66) so that tools which print or
// persist ids as hex keep working; the 12 bits the reference leaves as padding
// (:45) carry the knobs that only exist in the gfx950 kernels.
//
//   bits  0- 7  tile_m            m-tiles (of 16) per workgroup        = MT
//   bits  8-15  tile_n            n-tiles (of 16) per workgroup        = WN*NT
//   bits 16-23  tile_k            k per span in units of 64            = 2*KS (low 5 bits);
//                                 bits 21-23: log2 of the direct-path activation
//                                 prefetch distance PA
//   bits 24-27  features          Grid (1) | HighPrecision (2)  -- always 3 here:
//                                 every gfx950 kernel dequantises exactly
//   bits 28-31  element_b         1 NVFP4, 2 MXFP4          (MatmulElementB)
//   bits 32-35  mfma_type         0 fp16, 1 bf16            (MatmulMfmaType)
//   bits 36-39  warp_partition_m  1; 2 = the 5 <= M <= 16 kernel whose WN waves of a K part share one
//                                 activation tile in LDS (gemm_mid.hpp; warp_partition = 10 / 11 as the
//                                 staged streaming kernels: 8 / 16 rows), and with warp_partition = 0 the same
//                                 organisation for 17 <= M <= 128 (gemm_batch.hpp: tile_m = MT m-tiles per workgroup)
//   bits 40-43  warp_partition_n  WN
//   bits 44-47  warp_partition_k  WK
//   bits 48-51  warp_partition    the reference's NK(0)/Cooperative(1) enum, never 1 in
//                                 its shipped table; here: activation path,
//                                 0 = direct L2 fragments, 1/2/3 = 1/2/4 rows staged
//                                 through wave-private LDS (AM in gemm_stream.hpp),
//                                 10/11 = 8/16 rows staged the same way;
//                                 5/6/7 = the same staged paths on the fp16 pipeline
//                                 with block-floating-point activations (bf16 x NVFP4),
//                                 9 = the native-FP4 kernel (gemm_native.hpp; mfma_type
//                                 nibble = 2, the reference's unused kMatmulMfmaTypeFp8,
//                                 bit 35 set when the activations are fp16),
//                                 8 = the tiled large-M kernel (gemm_tiled.hpp), whose
//                                 fields read: tile_m = MT, warp_partition_n = WAVES,
//                                 bits 52-55 = NTW, warp_partition_k = 1;
//                                 12 = the 32x32x16-MFMA large-M kernel (gemm_wide.hpp):
//                                 tile_m = MB (m32-blocks), bits 52-55 = 2 NP;
//                                 13 = the 32x32x64 native-FP4 kernel (gemm_native32.hpp);
//                                 4 / 14 / 15 = the NVFP4 decode kernel that scales after the
//                                 MFMA (gemm_decode.hpp), 1 / 2 / 4 activation rows (15 with warp_partition_m = 2: 8 rows)
//   bits 52-55  [was padding]     NT  n-tiles per wave
//   bits 56-59  [was padding]     D   W ring depth (tiles in flight per n-tile)
//   bits 60-63  [was padding]     split-K across workgroups (gridDim.z), >= 1
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"
#include "petit_internal.h"

namespace petit_amd {

enum : unsigned { kFeatGrid = 1u, kFeatHighPrecision = 2u };
enum : unsigned { kElemBNvFp4 = 1u, kElemBMxFp4 = 2u }; // (3 was round 3's "MXFP4, scales promised in fp16's range": read as 2 now, find_explicit in solutions.hip)
enum : unsigned { kMfmaFp16 = 0u, kMfmaBf16 = 1u, kMfmaFp8 = 2u, kMfmaFp8ActFp16 = 2u | 8u, kMfmaFp4 = 6u, kMfmaFp4ActFp16 = 6u | 8u, kMfmaFp6 = 4u, kMfmaFp6ActFp16 = 4u | 8u };

struct StreamShape {
    int ks, mt, nt, wn, wk, d, am; // am == kTiledAm marks the tiled kernel
    int pa = 1;                    // direct-path activation prefetch distance (1, 2, 4 or 8 tiles)
    int wm = 1;                    // warp_partition_m nibble: 2 = the shared-activation-tile kernel (gemm_mid.hpp)
};
constexpr unsigned pa_code(int pa) { return pa == 8 ? 3u : pa == 4 ? 2u : pa == 2 ? 1u : 0u; }
constexpr int kTiledAm = -1;
// the native-FP4 kernels (gemm_native.hpp): MXFP4 weights straight into the block-scaled MFMA,
// activations quantised to MXFP8; opt-in, never a default
constexpr int kNativeAm = -2;
// the 32x32x16-MFMA large-M kernel (gemm_wide.hpp): code 12; fields read tile_m = MB (m32-blocks), bits 52-55 = n-tiles
// per wave (2 NP), warp_partition_n = WAVES
constexpr int kWideAm = -3;
// the native-FP4 kernels on the 32x32x64 block-scaled MFMA (gemm_native32.hpp): code 13; fields as kWideAm; pa = 1: activations
// quantised to MXFP8 (mfma_type 2), pa = 2: to MXFP4 (mfma_type 6: FP4 x FP4); warp_partition_m = WM waves along M (tile_m =
// MB * WM m32-blocks per workgroup); opt-in, never a default
constexpr int kNative32Am = -4;
constexpr bool is_native_am(int am) { return am == kNativeAm || am == kNative32Am; }
// am 101 / 102 / 104: staged activations (1 / 2 / 4 rows) converted to the fp16 pipeline with
// per-span block floating point (Bf16Bfp in gemm_stream.hpp); codes 5 / 6 / 7
constexpr int kBfpAm = 100;
// am 201 / 202 / 204 / 208: the NVFP4 decode kernel with the group scale applied after the MFMA (gemm_decode.hpp), holding
// 1 / 2 / 4 / 8 activation rows; codes 4 / 14 / 15 / 15 (the 16 codes of the nibble are taken: the 8-row form is code 15 with
// warp_partition_m = 2)
constexpr int kDecodeAm = 200;
constexpr int am_rows(int am) { return am >= kDecodeAm ? am - kDecodeAm : am >= kBfpAm ? am - kBfpAm : am; }
constexpr unsigned am_code(int am) {
    return am == kNativeAm ? 9u
           : am == kNative32Am ? 13u
           : am == kWideAm  ? 12u
           : am == kTiledAm ? 8u
           : am == 0        ? 0u
           : am == 8        ? 10u
           : am == 16       ? 11u
           : am >= kDecodeAm ? (am == kDecodeAm + 1 ? 4u : am == kDecodeAm + 2 ? 14u : 15u)
                            : (am_rows(am) == 1 ? 1u : am_rows(am) == 2 ? 2u : 3u) + (am >= kBfpAm ? 4u : 0u);
}

constexpr uint64_t make_solution_id(const StreamShape &s, unsigned elem_b, unsigned mfma, unsigned splitk) {
    return (uint64_t)(s.mt & 0xff) | ((uint64_t)((s.wn * s.nt) & 0xff) << 8) |
           ((uint64_t)(((2 * s.ks) & 0x1f) | (pa_code(s.pa) << 5)) << 16) | ((uint64_t)(kFeatGrid | kFeatHighPrecision) << 24) |
           ((uint64_t)(elem_b & 0xf) << 28) | ((uint64_t)(mfma & 0xf) << 32) | ((uint64_t)(s.wm & 0xf) << 36) |
           ((uint64_t)(s.wn & 0xf) << 40) | ((uint64_t)(s.wk & 0xf) << 44) | ((uint64_t)am_code(s.am) << 48) |
           ((uint64_t)(s.nt & 0xf) << 52) |
           ((uint64_t)(s.d & 0xf) << 56) | ((uint64_t)(splitk & 0xf) << 60);
}
constexpr unsigned solution_splitk(uint64_t id) { return (unsigned)(id >> 60) & 0xf; }
constexpr uint64_t solution_without_splitk(uint64_t id) { return (id & ~((uint64_t)0xf << 60)) | ((uint64_t)1 << 60); }

// --- Launch geometry: the ONE statement of how a kernel's grid and K range lie on a problem, read from the table entry's shape.  plan_gemm (dispatch.hip)
// decides a call's K split with it, the launchers (stream_tu.inc, moe_tu.inc, moe_native_tu.inc) launch what it says, and the cost model, the picks and the
// tuner's candidate list read their tiles from it.  The launcher TUs assert at compile time that tile and K parts are their Cfg's own (table_shape).
constexpr bool shape_is_shared(const StreamShape &s) { return s.am == kWideAm && s.wm == 5; }                 // gemm_shared.hpp
constexpr bool shape_is_batch(const StreamShape &s) { return s.am == 0 && s.wm == 2; }                        // gemm_batch.hpp
constexpr bool shape_is_decode(const StreamShape &s) { return s.am >= kDecodeAm; }                            // gemm_decode.hpp
constexpr bool shape_is_mid(const StreamShape &s) { return s.am > 0 && s.am < kBfpAm && s.wm == 2; }          // gemm_mid.hpp
constexpr bool shape_is_stream(const StreamShape &s) { return s.am >= 0 && s.am < kDecodeAm && s.wm == 1; }   // gemm_stream.hpp, direct and staged
struct WorkgroupTile {
    unsigned bm, bn;     // rows x columns of C per workgroup; the 32x32 MFMA kinds count tile_m in m32-blocks.  (The staged / decode kernels, one m-tile in the
                         // id, hold stage_rows rows: bm stays the m-tile for the readers that compare tiles across kinds.)
    unsigned kparts;     // K parts inside a workgroup: the K waves WK of the streaming / decode / mid / batch kinds, the K groups of wide / native32 (wm == 3: 2)
    unsigned stage_rows; // staged streaming / mid / decode kernels: the activation rows a workgroup holds -- all the M they run; else 0
    bool one_slice;      // decode / mid: the kinds that take no K split across workgroups
    bool even_split;     // streaming: grid z is the requested split whatever K (the other kinds drop empty slices)
    constexpr unsigned moe_rows() const { return stage_rows ? stage_rows : bm; } // rows per workgroup of the kernel's MoE form
};
constexpr WorkgroupTile workgroup_tile(const StreamShape &s) {
    const bool m32 = s.am == kWideAm || s.am == kNative32Am;
    const bool tile_kind = s.am == kTiledAm || s.am == kNativeAm || m32; // (these read warp_partition_k as something else: solution.h, stream_tu.inc)
    return WorkgroupTile{(m32 ? 32u : 16u) * (unsigned)s.mt,
                         16u * (unsigned)s.wn * (unsigned)s.nt,
                         tile_kind ? (m32 && s.wm == 3 ? 2u : 1u) : (unsigned)s.wk,
                         s.am > 0 ? (unsigned)am_rows(s.am) : 0u,
                         shape_is_decode(s) || shape_is_mid(s),
                         shape_is_stream(s)};
}
struct LaunchGeometry : WorkgroupTile {
    unsigned splitk;         // the split asked for (the launchers of the one-slice kinds refuse > 1)
    unsigned grid_x, grid_y; // workgroups along N and M (decode / mid: one row of workgroups)
    unsigned spans_per_part; // K spans one part walks (GemmArgs::spans_per_wave)
    unsigned slices;         // workgroups along K that own at least one span: grid z; > 1 = fp32 slabs and a reduce pass
};
// `splitk` K slices of whole spans over the kparts parts of each workgroup: spans_per_part = ceil(nspans / (splitk kparts)), and as many slices as then
// own a span (the last may be shorter, and the last workgroup may find its later parts empty) -- what the batch, tiled, wide, shared and native
// launchers each computed for themselves; the streaming kernels keep every requested slice; decode / mid have one.
constexpr LaunchGeometry launch_geometry(const StreamShape &s, unsigned splitk, unsigned m, unsigned n, unsigned k) {
    const WorkgroupTile t = workgroup_tile(s);
    const unsigned nspans = k / (unsigned)(kTileK * s.ks), split = t.one_slice || splitk == 0 ? 1u : splitk;
    const unsigned per_wg = t.bn / kTileN, ntiles = n / kTileN;
    const unsigned spp = (nspans + split * t.kparts - 1) / (split * t.kparts);
    const unsigned slices = t.even_split ? split : spp ? (nspans + spp * t.kparts - 1) / (spp * t.kparts) : 1u;
    return LaunchGeometry{t, splitk, (ntiles + per_wg - 1) / per_wg, t.one_slice ? 1u : (m + t.bm - 1) / t.bm, spp, slices};
}
// The shape of a table entry (or MoE form), written next to its Cfg from the same macro arguments: states once, at compile time, that the tile and the
// in-workgroup K parts read from the shape are the Cfg's own.  ROWS: the Cfg's rows per workgroup (kMoe: of its MoE form), COLS: its columns.
template <StreamShape S, int ROWS, int COLS, int KPARTS, bool kMoe = false> constexpr StreamShape table_shape() {
    constexpr WorkgroupTile t = workgroup_tile(S);
    static_assert((kMoe ? t.moe_rows() : t.bm) == (unsigned)ROWS && t.bn == (unsigned)COLS && t.kparts == (unsigned)KPARTS,
                  "launch geometry (workgroup_tile) disagrees with the kernel's Cfg");
    return S;
}

using LaunchFn = int (*)(const GemmArgs &, const LaunchGeometry &, hipStream_t);
// several GEMMs sharing the activation rows in one launch (GroupTable, petit_internal.h): the launcher fills wg_end
using LaunchGroupedFn = int (*)(GroupTable, const void *a, unsigned m, unsigned k, hipStream_t);

// all experts of a MoE layer in one launch (MoeArgs, petit_internal.h; gemm_moe.hpp); never a K split across workgroups, no scratch
// (the geometry of (shape, split 1, m, n, k): rows per workgroup, grid x, the one slice's spans)
using LaunchMoeFn = int (*)(const MoeArgs &, const LaunchGeometry &, hipStream_t);

struct SolutionEntry {
    StreamShape shape;
    int a_type; // kDataTypeBf16 / kDataTypeFp16
    int fmt;    // kFmtNv / kFmtMx (gemm_stream.hpp)
    LaunchFn launch;
    LaunchGroupedFn launch_grouped = nullptr; // the decode and the staged streaming kernels have one (M <= 16)
    LaunchMoeFn launch_moe = nullptr;         // the decode, staged streaming and tiled kernels of moe_tu.inc
    LaunchMoeFn launch_moe_idx = nullptr;     // their indexed forms (gathered A, scattered C): set exactly where launch_moe is
    LaunchMoeFn launch_moe_native = nullptr;  // 32x32x64 native kernels of moe_native_tu.inc: quantised grouped rows in, scattered C out
};

// The MoE forms of a family: compiled in translation units of their own (gemm_moe_<family>.hip) and attached to the table entries of the
// same shape when the family's table is assembled (solutions.hip) -- no table entries and no ids of their own.
struct MoeForm {
    StreamShape shape;
    LaunchMoeFn launch;
};
constexpr bool same_shape(const StreamShape &a, const StreamShape &b) {
    return a.ks == b.ks && a.mt == b.mt && a.nt == b.nt && a.wn == b.wn && a.wk == b.wk && a.d == b.d && a.am == b.am && a.pa == b.pa && a.wm == b.wm;
}
const MoeForm *moe_forms_nv_bf16(int *count);
const MoeForm *moe_forms_nv_f16(int *count);
const MoeForm *moe_forms_mx_bf16(int *count);
const MoeForm *moe_forms_mx_f16(int *count);
const MoeForm *moe_idx_forms_nv_bf16(int *count);
const MoeForm *moe_idx_forms_nv_f16(int *count);
const MoeForm *moe_idx_forms_mx_bf16(int *count);
const MoeForm *moe_idx_forms_mx_f16(int *count);
const MoeForm *moe_native_forms_nv_bf16(int *count); // (gemm_moe_native_<family>.hip)
const MoeForm *moe_native_forms_nv_f16(int *count);
const MoeForm *moe_native_forms_mx_bf16(int *count);
const MoeForm *moe_native_forms_mx_f16(int *count);

// one table per (activation type, weight format) family, concatenated once (solutions.hip) from the parts its translation units export
// (stream_tu.inc: gemm_<family>_p<part>.hip)
const SolutionEntry *solutions_nv_bf16(int *count);
const SolutionEntry *solutions_nv_f16(int *count);
const SolutionEntry *solutions_mx_bf16(int *count);
const SolutionEntry *solutions_mx_f16(int *count); // Fp16Mx kernels (device_common.hpp)
#define PETIT_DECLARE_PARTS(fam)                      \
    const SolutionEntry *solutions_##fam##_p1(int *); \
    const SolutionEntry *solutions_##fam##_p2(int *); \
    const SolutionEntry *solutions_##fam##_p3(int *); \
    const SolutionEntry *solutions_##fam##_p4(int *);
PETIT_DECLARE_PARTS(nv_bf16)
PETIT_DECLARE_PARTS(nv_f16)
PETIT_DECLARE_PARTS(mx_bf16)
PETIT_DECLARE_PARTS(mx_f16)
#undef PETIT_DECLARE_PARTS
const SolutionEntry *solutions_nv_bf16_p6(int *); // batched decode (gemm_batch.hpp); fp16 x MXFP4: the loader-wave form only (fast body + exact fallback)
const SolutionEntry *solutions_mx_f16_p6(int *);
const SolutionEntry *solutions_nv_f16_p6(int *);
const SolutionEntry *solutions_mx_bf16_p6(int *);
const SolutionEntry *solutions_mx_bf16_p5(int *); // native FP4 MFMA kernels: MXFP4 weights only
const SolutionEntry *solutions_mx_f16_p5(int *);
const SolutionEntry *solutions_nv_bf16_p5(int *); // the same kernels on the MFMA-native image of NVFP4 weights (nvnative.hip)
const SolutionEntry *solutions_nv_f16_p5(int *);
// the activation quantiser of the 32x32x64 native kernels, stand-alone (gemm_mx_{bf16,f16}.hip): format 8 = MXFP8, 4 = MXFP4
int quantize32_bf16(const void *a, void *qa, unsigned m, unsigned k, int format, hipStream_t stream);
int quantize32_f16(const void *a, void *qa, unsigned m, unsigned k, int format, hipStream_t stream);
// ... its gathering form (gemm_moe_native_mx_{bf16,f16}.hip): layout row r from row a_idx[r] of a [a_rows][k] (null: row r; outside: a zero row)
int quantize32_rows_bf16(const void *a, const int *a_idx, unsigned a_rows, void *qa, unsigned m, unsigned k, int format, hipStream_t stream);
int quantize32_rows_f16(const void *a, const int *a_idx, unsigned a_rows, void *qa, unsigned m, unsigned k, int format, hipStream_t stream);

} // namespace petit_amd
