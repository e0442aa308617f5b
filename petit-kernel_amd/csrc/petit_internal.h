// petit_internal.h -- declarations shared by the translation units of
// libpetit_amd.so.  Not installed; the public surface is include/petit_amd.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"

namespace petit_amd {

// Error codes.  0/1/2 are the reference's (quantization/gemm.h:107-108);
// the rest are additions of this library (launch failures are polled here,
// the reference never does -- SURVEY.md section 5).
enum : int {
    kOk = 0,
    kErrProblemShape = 1, // kErrorProblemShape
    kErrKernelShape = 2,  // kErrorKernelShape
    kErrLaunch = 3,       // hipGetLastError() != hipSuccess after a launch
    kErrBadArgument = 4,  // null pointer / unknown dtype
};

// Arithmetic / element types, numbered as the reference's C++ DataType
// (quantization/types.h:4-13).
enum DataType : int {
    kDataTypeInt4 = 0,
    kDataTypeFp8e4m3 = 1,
    kDataTypeFp8e8m0 = 2,
    kDataTypeFp4e2m1 = 3,
    kDataTypeFp16 = 4,
    kDataTypeBf16 = 5,
    kDataTypeFp8e5m2Fnuz = 6,
    kDataTypeMxFp4e2m1 = 7,
    // round 3's extension "MXFP4 whose every e8m0 block scale lies in 114..140" (PETIT_DTYPE_MXFP4_E2M1_F16RANGE, include/petit_amd.h): still
    // accepted, and means plain MXFP4 -- the fp16 kernels test the range themselves (Fp16Mx, device_common.hpp), so there is nothing to promise
    kDataTypeMxFp4e2m1F16Range = 8,
};

constexpr bool is_mx_type(int b_type) { return b_type == kDataTypeMxFp4e2m1 || b_type == kDataTypeMxFp4e2m1F16Range; }
constexpr int canonical_b_type(int b_type) { return b_type == kDataTypeMxFp4e2m1F16Range ? (int)kDataTypeMxFp4e2m1 : b_type; }

// the largest M any entry point accepts (PETIT_ERROR_PROBLEM_SHAPE beyond): the open-ended last bucket of the arch tables ends here, and every
// 32-bit quantity the kernels form from M (grid rows, row * k * 2 inside one workgroup's activation block) stays in range below it
constexpr unsigned kMaxM = 1u << 20;

// petit_epilogue.activation (PETIT_ACTIVATION_*): the values this library knows, and the gated ones -- SiLU-mul (1) and SwiGLU-OAI (2) share every
// shape rule, pick and refusal; the kind itself reaches only the epilogue arithmetic (GemmArgs::act / reduce_act, MoeArgs::act)
constexpr bool activation_known(int activation) { return activation >= 0 && activation <= 2; }
constexpr bool activation_gated(int activation) { return activation == 1 || activation == 2; }

struct GemmArgs {
    void *c;            // [m][n] 16-bit, row-major
    const void *a;      // [m][k] 16-bit, row-major
    const void *w;      // packed weights (layout.h)
    const void *s;      // packed scales  (layout.h)
    const float *gs;    // device pointer, one float
    const void *bias;   // optional fused epilogue: [n] in c's dtype, added before the single rounding; may be null
    unsigned act;       // 0 none; 1 SiLU-mul: c is [m][n/2], c[m][j] = silu(y[m][j]) * y[m][j + n/2]  (y = acc*gs + bias); 2 SwiGLU-OAI: same
                        // shape and tile pairing, the clamped gpt-oss formula (silu_mul4, device_common.hpp) -- the PETIT_ACTIVATION_* value
    unsigned reduce_act; // 1 / 2: that activation with a cross-workgroup K split -- the kernels see act = 0 (plain slabs), the reduce pass applies it
    float *workspace;   // fp32 split-K slabs (may be null when splitk == 1)
    unsigned m, n, k;
    unsigned spans_per_wave; // set by the launcher from the planned geometry (LaunchGeometry::spans_per_part, solution.h)
    unsigned flags;          // large-M kernels: kFlagPrio | kFlagXcdRaster | band << kFlagBandShift (launch_flags(), stream_tu.inc)
    // native-FP4 pipeline (gemm_native32.hpp): activations the CALLER already holds quantised (no quantiser launch), and a
    // SiLU-mul epilogue that emits the NEXT GEMM's quantised activations instead of a 16-bit matrix
    const void *qa;          // pre-quantised activations in the k-tile-major scratch layout of format qa_format, or null
    unsigned qa_format;      // 8 (MXFP8) / 4 (MXFP4) when qa is set
    unsigned out_format;     // 0: c is a 16-bit matrix; 8 / 4: c receives [m][n/2] activations quantised to MXFP8 / MXFP4 (act = 1 / 2 only)
};
enum : unsigned { kFlagPrio = 1u, kFlagXcdRaster = 2u, kFlagBandShift = 8 }; // bits 8..15: m-tiles per raster band (0 = whole columns)

// A group of GEMMs that share the activation rows, for the grouped kernels (petit_gemm_fp4_fp16_grouped): passed by value as a
// kernel argument; wg_end[i] = workgroups of members 0..i (prefix sums along grid x).
constexpr int kMaxGroup = 8;
struct GroupTable {
    unsigned count;
    unsigned wg_end[kMaxGroup];
    unsigned n[kMaxGroup];
    const void *w[kMaxGroup];
    const void *s[kMaxGroup];
    void *c[kMaxGroup];
    const float *gs[kMaxGroup];
    const void *bias[kMaxGroup];
};

// A routed-expert (MoE) GEMM (petit_gemm_fp4_fp16_moe, gemm_moe.hpp): E experts' packed weights / scales / global scales / biases
// stacked back to back, the activation rows grouped by expert (rows offsets[e] .. offsets[e+1]-1: expert e; a device array the host never reads).
constexpr unsigned kMoeMaxExperts = 1024;
struct MoeArgs {
    void *c;              // [m][n] (SiLU-mul: [m][n/2]) 16-bit, rows in a's order
    const void *a;        // [m][k] 16-bit
    const void *w, *s;    // E packed weight / scale blocks of one [n, k] matrix each
    const float *gs;      // [E]
    const void *bias;     // [E][n] in c's dtype, or null
    unsigned act;         // 0 none, 1 SiLU-mul, 2 SwiGLU-OAI (each expert's weight is [gate; up] along N)
    const int32_t *offsets; // [E + 1]
    unsigned num_experts, m, n, k;
    // the indexed forms only (petit_gemm_fp4_fp16_moe_ex): grouped row r reads a row a_idx[r] of a [a_rows][k] and writes c row
    // c_idx[r] of c [c_rows][.]; a null index is the identity
    const int32_t *a_idx = nullptr, *c_idx = nullptr;
    unsigned a_rows = 0, c_rows = 0;
    // the native forms only (petit_gemm_native_moe, gemm_moe_native.hpp): a holds the QUANTISED grouped rows (the kernel's own format), and
    // out_format 8 / 6 / 4 makes the SiLU-mul epilogue write c as the next launch's quantised grouped rows
    unsigned out_format = 0;
};
// the grid rows a MoE launch needs for any routing (gemm_moe.hpp), 0 when that exceeds the grid's y limit
inline unsigned moe_slots(unsigned m, unsigned bm, unsigned num_experts) {
    const uint64_t slots = ((uint64_t)m + bm - 1) / bm + (num_experts < m ? num_experts : m);
    return slots <= 65535u ? (unsigned)slots : 0u;
}

// The rows of an expert, as every MoE launch reads malformed offsets: each offset clamped into [its predecessor's clamped value, m] -- into
// [0, m], then a running maximum.  Stated here for the image builder's routing skip (nvnative.hip nv6_images_kernel, nv6_images_host), which
// must skip exactly the experts the launch gives no slot; moe_locate (gemm_moe.hpp) states the same rule as a wave-wide scan of its own -- two
// sites, change them together.  lo: the maximum of the clamped offsets[0 .. e]; raw_hi: offsets[e + 1]; the expert's upper end is lo + the result.
PETIT_HD unsigned moe_offset_clamped(int raw, unsigned m) {
    const unsigned v = raw > 0 ? (unsigned)raw : 0u;
    return v < m ? v : m;
}
PETIT_HD unsigned moe_expert_rows(unsigned lo, int raw_hi, unsigned m) {
    const unsigned hi = moe_offset_clamped(raw_hi, m);
    return hi > lo ? hi - lo : 0u;
}

// dispatch.hip: the dispatcher behind every GEMM entry point, which launches what plan_gemm (dispatch.h) decides (solution_id: explicit id or one of the AUTO sentinels)
} // namespace petit_amd
struct petit_solution_hints;
struct petit_epilogue;
namespace petit_amd {
// native pipeline options of a call (petit_gemm_mxfp4_native): a_format 8 / 4 = `a` already holds quantised activations,
// out_format 8 / 4 = the SiLU-mul epilogue emits quantised activations instead of a 16-bit matrix
struct NativeIo {
    unsigned a_format, out_format;
    const void *image = nullptr; // NVFP4 weights: their MFMA-native image (nvnative.hip), when the caller hands it over per call
    bool transient = false;      // NVFP4 weights: the image is built per call at the front of the call's scratch (petit_gemm_nvfp4_native_transient)
};
int gemm_impl(int b_type, unsigned *c, const unsigned *a, const unsigned *b, const unsigned *scales, const float *global_scale, unsigned m,
              unsigned n, unsigned k, const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue, void *call_ws,
              uint64_t call_ws_bytes, void *stream, const NativeIo *io = nullptr);
int tune_candidates(int a_type, int b_type, int klass, unsigned m, unsigned n, unsigned k, uint64_t max_ws, uint64_t *ids, uint64_t *needs,
                    int cap);

// tune.hip
struct TuneRequest {
    void *c;                 // [m][n] output buffer the candidates may overwrite
    const void *a;           // [m][k] activations
    const void *const *b;    // n_copies packed weight pointers
    const void *const *s;    // n_copies packed scale pointers
    unsigned n_copies;
    const float *gs;
    unsigned m, n, k;
    int a_type, b_type, klass;   // klass 0 exact, 8 / 4 native with MXFP8 / MXFP4 activations
    void *ws;
    uint64_t ws_bytes;
    bool own_workspace;      // allocate scratch for the largest candidate instead of using ws
    void *stream;
    unsigned launches, samples;
    float tolerance;
    bool persist;
    unsigned m_lo, m_hi;
    size_t rotate_bytes;     // n_copies == 1: clone the weights until the rotation covers this many bytes
};
int tune_problem(const TuneRequest &rq, uint64_t *best_solution, float *best_us);
bool autotune_enabled();
void autotune_on_first_sight(int b_type, unsigned *c, const unsigned *a, const unsigned *b, const unsigned *scales, const float *gs, unsigned m,
                             unsigned n, unsigned k, int a_type, void *ws, uint64_t ws_bytes, void *stream);

// repack.hip
int repack_weights(void *out, const void *in, unsigned k, unsigned n, hipStream_t stream);
int repack_nvscales(void *out, const void *in, unsigned k, unsigned n, hipStream_t stream);
int repack_mxscales(void *out, const void *in, unsigned k, unsigned n, hipStream_t stream);
int repack_weights_host(void *out, const void *in, unsigned k, unsigned n);
int repack_nvscales_host(void *out, const void *in, unsigned k, unsigned n);
int repack_mxscales_host(void *out, const void *in, unsigned k, unsigned n);
// reference-packed ("Petit" format of the reference wheel) -> this build's packed layout, host memory
int convert_reference_weights_host(void *out, const void *in, unsigned k, unsigned n);
int convert_reference_nvscales_host(void *out, const void *in, unsigned k, unsigned n);
int convert_reference_mxscales_host(void *out, const void *in, unsigned k, unsigned n);
// nvnative.hip: the MFMA-native image of NVFP4 weights ("petit-cdna4-nv6/1", layout.h) from the packed tensors; host twin; dense expansion (host)
int nv6_image(void *image, const void *pw, const void *ps, unsigned n, unsigned k, hipStream_t stream);
int nv6_image_host(void *image, const void *pw, const void *ps, unsigned n, unsigned k);
int nv6_image_dequant_host(float *out, const void *image, unsigned n, unsigned k);
// num_experts images back to back from the stacked packed tensors, ONE launch; offsets (int32 [E + 1], may be null) / m: experts without rows
// (moe_expert_rows == 0) are skipped, their regions untouched.  The host twin reads HOST offsets.
int nv6_images(void *images, const void *pw, const void *ps, unsigned num_experts, unsigned n, unsigned k, const int32_t *offsets, unsigned m,
               hipStream_t stream);
int nv6_images_host(void *images, const void *pw, const void *ps, unsigned num_experts, unsigned n, unsigned k, const int32_t *offsets, unsigned m);
// quantize_weights.hip: 16-bit weights [E][n][k] -> the packed tensors and one global scale per expert (include/petit_amd.h "Weight quantiser");
// host twin, bit-identical
uint64_t quantize_weights_workspace_bytes(int b_type, unsigned num_experts, bool gs_supplied);
int quantize_weights(const void *w, int a_type, int b_type, unsigned num_experts, unsigned n, unsigned k, const float *gs_in, void *out_b,
                     void *out_scales, float *out_gs, void *workspace, uint64_t workspace_bytes, hipStream_t stream);
int quantize_weights_host(const void *w, int a_type, int b_type, unsigned num_experts, unsigned n, unsigned k, const float *gs_in, void *out_b,
                          void *out_scales, float *out_gs);
// rmsnorm_quant.hip: (residual add +) RMSNorm -> "petit-qact/1" bytes in one launch (include/petit_amd.h "RMSNorm into quantised activations");
// host twin, bit-identical.  Both make every check of the contract.
int rmsnorm_quantize(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                     float weight_offset, unsigned m, unsigned k, int a_type, int format, hipStream_t stream);
int rmsnorm_quantize_host(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                          float weight_offset, unsigned m, unsigned k, int a_type, int format);
int rmsnorm_inv_host(float *inv, const void *x, const void *residual, float eps, unsigned m, unsigned k, int a_type); // (test aid: f32 inv per row)
int quantize_activations_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format); // the twins' quantiser on a 16-bit [m][k]
// the same three with the block-Hadamard rotation in front of the quantiser (include/petit_amd.h "Block-Hadamard rotation"); block 0: the above
int rmsnorm_quantize_rot(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                         float weight_offset, unsigned m, unsigned k, int a_type, int format, unsigned block, hipStream_t stream);
int rmsnorm_quantize_rot_host(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                              float weight_offset, unsigned m, unsigned k, int a_type, int format, unsigned block);
int quantize_activations_rot_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format, unsigned block);
// the MoE top-k combine as the front end of the same row (include/petit_amd.h "Top-k combine into the norm"); format 0: 16-bit outputs only
int moe_combine_rmsnorm(void *qa, void *y16, void *residual_out, const void *slot_out, const float *topk_weights, const void *topk_ids,
                        int ids_are_int64, const void *residual, const void *weight, float eps, float weight_offset, unsigned num_tokens,
                        unsigned topk, unsigned k, unsigned num_experts, int a_type, int format, hipStream_t stream);
int moe_combine_rmsnorm_host(void *qa, void *y16, void *residual_out, const void *slot_out, const float *topk_weights, const void *topk_ids,
                             int ids_are_int64, const void *residual, const void *weight, float eps, float weight_offset, unsigned num_tokens,
                             unsigned topk, unsigned k, unsigned num_experts, int a_type, int format);
// moe_router.hip: the router's GEMM (include/petit_amd.h "The router's GEMM"), as the route entries of moe_route.hip use it.  router_shape_rc:
// the shape / dtype refusals (kOk when the call can run).  router_slab_bytes: the fp32 slabs of the form T gets, rounded up to 256 bytes.
// router_gemm_launch writes router_slabs(T, ...) slabs [T][E] back to back; router_finish_launch sums n_slabs of them in order and adds the
// bias (null: none) into logits [T][E] -- the definition's additions, one thread per logit.
constexpr unsigned kRouterMaxSlices = 16; // S <= 16: what a route wave loads and adds per logit
int router_shape_rc(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type);
unsigned router_slabs(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type);
uint64_t router_slab_bytes(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type);
void router_gemm_launch(float *slabs, const void *hidden, const void *weight, int a_type, unsigned num_tokens, unsigned num_experts, unsigned k,
                        hipStream_t stream);
void router_finish_launch(float *logits, const float *slabs, unsigned n_slabs, const float *router_bias, unsigned num_tokens,
                          unsigned num_experts, hipStream_t stream);
// dequant.hip: dense expansion of packed weights (debug aid); out_kind 0 f32, 1 bf16, 2 fp16
int dequant_packed(void *out, const void *w, const void *s, float gs, unsigned n, unsigned k, int b_type, int out_kind, hipStream_t stream);

} // namespace petit_amd
