/*
 * petit_amd.h -- C ABI of libpetit_amd.so, the MI355X (gfx950) build of the
 * petit FP4 mixed-precision GEMM.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types, no
 * C++ in the signatures.  Every entry point names the reference interface it
 * replaces (paths relative to the reference tree, causalflow-ai/petit-kernel
 * v0.0.3).  The C++ namespace API of the reference
 * (lib/gemm/rocm/quantization/gemm.h:119-146) is provided as inline wrappers
 * over these symbols in include/causalflow/petit/gemm.h; the Python surface
 * (petit_kernel/__init__.py:8-79) binds them through ctypes.
 *
 * Ownership: the caller owns every buffer; the library keeps no pointers past
 * the call except the optional workspace registered with
 * petit_set_workspace().  All work is enqueued on `stream` (a hipStream_t);
 * nothing synchronises the host, so every call is HIP-graph capturable.
 * Thread safety: all entry points may be called concurrently from several
 * host threads and streams; kernels that need scratch memory take it per call
 * (petit_gemm_*_ws) or from the per-device registered workspace, which serves
 * ONE stream at a time (see "Scratch memory" below); petit_set_workspace()
 * itself must not race with GEMM calls on the same device.
 */
#ifndef PETIT_AMD_H_
#define PETIT_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes.  0/1/2 are the reference's (quantization/gemm.h:107-108):
 * kErrorProblemShape = 1, kErrorKernelShape = 2.  3 and 4 are additions: the
 * reference never polls launch errors (gemm_fp4_fp16_grid.cuh:556-559). */
#define PETIT_OK 0
#define PETIT_ERROR_PROBLEM_SHAPE 1
#define PETIT_ERROR_KERNEL_SHAPE 2
#define PETIT_ERROR_LAUNCH 3
#define PETIT_ERROR_BAD_ARGUMENT 4

/* Element types, numbered as the reference's C++ enum
 * (quantization/types.h:4-13).  NOTE: the reference's *Python* DataType enum
 * (petit_kernel/__init__.py:8-15) is numbered differently; the Python layer
 * of this build translates. */
typedef enum petit_data_type {
    PETIT_DTYPE_INT4 = 0,
    PETIT_DTYPE_FP8_E4M3 = 1,
    PETIT_DTYPE_FP8_E8M0 = 2,
    PETIT_DTYPE_FP4_E2M1 = 3, /* NVFP4: e4m3 scales, group 16 */
    PETIT_DTYPE_FP16 = 4,
    PETIT_DTYPE_BF16 = 5,
    PETIT_DTYPE_FP8_E5M2_FNUZ = 6,
    PETIT_DTYPE_MXFP4_E2M1 = 7, /* MXFP4: e8m0 scales, group 32 */
    /* Deprecated alias of PETIT_DTYPE_MXFP4_E2M1 (round 3: "MXFP4 whose every e8m0 block scale byte lies in 114..140", a caller's promise that
     * selected a faster fp16 kernel family).  Nobody has to promise anything any more: with fp16 activations every MXFP4 kernel tests, per wave
     * and span, the scale bytes it holds anyway, converts the weights straight to fp16 (one MFMA per fragment) while they lie in
     * PETIT_MXFP4_F16RANGE_SCALE_MIN .. _MAX (2^-13 .. 2^13: e2m1 x scale a normal fp16 number -- every real checkpoint), and finishes its K range
     * in an exact bf16 hi / lo fallback body from the first byte that does not.  Both bodies are exact, so the value 8 carries no information;
     * it is accepted wherever PETIT_DTYPE_MXFP4_E2M1 is and treated as it. */
    PETIT_DTYPE_MXFP4_E2M1_F16RANGE = 8
} petit_data_type;
#define PETIT_MXFP4_F16RANGE_SCALE_MIN 114
#define PETIT_MXFP4_F16RANGE_SCALE_MAX 140

/* PetitSolutionHints, quantization/gemm.h:112-117.  Ignored when an explicit
 * solution id is passed.  require_high_precision is accepted for
 * compatibility: every gfx950 kernel here dequantises exactly, so it never
 * changes the result. */
typedef struct petit_solution_hints {
    int32_t a_type; /* PETIT_DTYPE_FP16 or PETIT_DTYPE_BF16 */
    int32_t b_type; /* PETIT_DTYPE_FP4_E2M1 or PETIT_DTYPE_MXFP4_E2M1 */
    int32_t c_type; /* must equal a_type */
    int32_t require_high_precision;
} petit_solution_hints;

/* "Let the library choose": the reference's (unsigned long)-1 sentinel,
 * fp4/gemm_fp4_fp16_grid.cc:46-48. */
#define PETIT_SOLUTION_AUTO UINT64_MAX
/* "Let the library choose INSIDE the native-FP4 class" (MXFP4 entry points; NVFP4 entry points once the weights have an MFMA-native image attached --
 * "NVFP4 weights on the native class" below; see "Native-FP4 kernels"): the caller
 * opts into quantised activations by naming the sentinel -- MXFP8 activations (FP4 x FP8 block-scaled MFMA), MXFP6 (e2m3
 * elements: the three mantissa bits of e4m3 at the instruction's FP4 rate) or MXFP4 activations (FP4 x FP4).  Needs per-call scratch (petit_gemm_workspace_bytes with the same sentinel); without it the call
 * returns PETIT_ERROR_KERNEL_SHAPE rather than silently running another accuracy class.  The Python layers spell them
 * solution_id = -2 / -3 / -4. */
#define PETIT_SOLUTION_AUTO_NATIVE_MXFP8 (UINT64_MAX - 1)
#define PETIT_SOLUTION_AUTO_NATIVE_MXFP4 (UINT64_MAX - 2)
#define PETIT_SOLUTION_AUTO_NATIVE_MXFP6 (UINT64_MAX - 3)

/*
 * c[m][n] = a[m][k] . dequant(b)[n][k]^T * (*global_scale), f32 accumulate,
 * one round-to-nearest-even to the 16-bit output type.
 *   replaces fp4::GemmFp4Fp16Grid      quantization/gemm.h:120-124
 *            (impl fp4/gemm_fp4_fp16_grid.cc:36-77)
 *   c, a          device, row-major 16-bit (hints->a_type); a is [m][k]
 *   b             device, packed weights from petit_repack_nvfp4_weights
 *   scales        device, packed scales from petit_repack_nvfp4_scales
 *   global_scale  DEVICE pointer to one float (lib/pybind/fp4.cc:198)
 *   n % 16 == 0, k % 256 == 0, m arbitrary; m|n|k == 0 returns PETIT_OK
 *   solution_id   PETIT_SOLUTION_AUTO or an id from petit_gemm_get_solutions
 */
int petit_gemm_fp4_fp16_grid(unsigned *c, const unsigned *a, const unsigned *b,
                             const unsigned *scales, const float *global_scale,
                             unsigned m, unsigned n, unsigned k,
                             const petit_solution_hints *hints,
                             uint64_t solution_id, void *stream);

/* Same for MXFP4 weights (e8m0 scales, group 32).
 *   replaces fp4::GemmMxFp4Fp16Grid    quantization/gemm.h:126-130
 *            (impl fp4/gemm_fp4_fp16_grid.cc:79-95)
 * The reference accepts bf16 activations only (gemm_fp4_fp16_grid.cc:55-64);
 * this build also accepts fp16. */
int petit_gemm_mxfp4_fp16_grid(unsigned *c, const unsigned *a, const unsigned *b,
                               const unsigned *scales, const float *global_scale,
                               unsigned m, unsigned n, unsigned k,
                               const petit_solution_hints *hints,
                               uint64_t solution_id, void *stream);

/*
 * The same two GEMMs with a fused epilogue (no counterpart in the reference,
 * whose callers add the bias in a separate torch op after the kernel has already rounded to 16 bit):
 *   c[m][n] = round16( acc[m][n] * (*global_scale) + bias[n] )
 * bias: device pointer to n elements of c's type (hints->c_type), 8-byte aligned, or NULL.
 * epilogue == NULL or {NULL, 0, 0} is exactly the plain call.
 * activation = PETIT_ACTIVATION_SILU_MUL (the gate_up projection of a gated MLP, vLLM's SiluAndMul fused
 * in): with y = acc * (*global_scale) + bias, c is [m][n/2] and
 *   c[m][j] = round16( silu(y[m][j]) * y[m][j + n/2] ),   silu(x) = x / (1 + exp(-x)).
 * Needs n % 32 == 0 and a kernel with an even number of n-tiles per wave: PETIT_SOLUTION_AUTO picks one;
 * an explicit id without that property (or with a cross-workgroup K split) returns PETIT_ERROR_KERNEL_SHAPE.
 * activation = PETIT_ACTIVATION_SWIGLU_OAI (gpt-oss's gated MLP): the same contract -- c is [m][n/2], column j of the first
 * half of N is gate and column j + n/2 is up, y as above in f32 -- with the clamped formula
 *   g = min(y[m][j], 7.0f),  u = min(max(y[m][j + n/2], -7.0f), 7.0f),
 *   c[m][j] = round16( g / (1 + exp(-1.702f * g)) * (u + 1) ),   rounded once.
 * alpha = 1.702 and limit = 7.0 are gpt-oss's own and fixed by the activation value (`reserved` keeps its meaning: 0).
 * Every shape rule, pick and refusal of SILU_MUL holds for it unchanged (n % 32 == 0, the tile pairing or a cross-workgroup
 * K split, the quantised output's n % 512 == 0); a gate of -inf gives -0 / 0, NaN and +-inf propagate as in the SiLU form.
 * Any other activation value returns PETIT_ERROR_BAD_ARGUMENT.
 */
#define PETIT_ACTIVATION_NONE 0
#define PETIT_ACTIVATION_SILU_MUL 1
#define PETIT_ACTIVATION_SWIGLU_OAI 2
typedef struct petit_epilogue {
    const void *bias;
    int32_t activation;
    int32_t reserved;
} petit_epilogue;

int petit_gemm_fp4_fp16_grid_ex(unsigned *c, const unsigned *a, const unsigned *b,
                                const unsigned *scales, const float *global_scale,
                                unsigned m, unsigned n, unsigned k,
                                const petit_solution_hints *hints, uint64_t solution_id,
                                const petit_epilogue *epilogue, void *stream);
int petit_gemm_mxfp4_fp16_grid_ex(unsigned *c, const unsigned *a, const unsigned *b,
                                  const unsigned *scales, const float *global_scale,
                                  unsigned m, unsigned n, unsigned k,
                                  const petit_solution_hints *hints, uint64_t solution_id,
                                  const petit_epilogue *epilogue, void *stream);

/* Enumerate the kernels that can run (hints, m, n, k).  Count-then-fill: call
 * with sols == NULL to get *n_sols, then again with a buffer of that size.
 *   replaces fp4::GemmGetSolutions     quantization/gemm.h:132-133
 *            (impl fp4/algo_chooser.cc:14-62)
 * Returns 0, or -1 when hints->b_type is not an FP4 type (algo_chooser.cc:20-23).
 * Ids use the reference's 64-bit SolutionId bit layout (gemm.h:33-66). */
int petit_gemm_get_solutions(const petit_solution_hints *hints, unsigned m,
                             unsigned n, unsigned k, uint64_t *sols,
                             unsigned *n_sols);

/* The id the library would pick for PETIT_SOLUTION_AUTO (arch table first,
 * heuristic second); 0 when nothing fits.
 *   replaces fp4::ChooseDefaultFp4Fp16Solution  fp4/algo_chooser.cc:64-132 */
uint64_t petit_gemm_default_solution(const petit_solution_hints *hints,
                                     unsigned m, unsigned n, unsigned k);
/* The concrete id a call (hints, m, n, k, solution_id, epilogue) that hands over `workspace_bytes` of scratch would RUN, read
 * from the launcher's own plan: solution_id may be PETIT_SOLUTION_AUTO, one of the PETIT_SOLUTION_AUTO_NATIVE_* sentinels, or an
 * explicit id (returned normalised), and 0 means that call would be refused.  petit_gemm_default_solution() answers for "as much
 * scratch as the pick wants" (what the Python layers provide): possibly an id with a K split (bits 60-63 > 1), which a caller
 * WITHOUT scratch cannot run -- such a caller (petit_gemm_fp4_fp16_grid / _ex with no registered workspace) gets the kernel this
 * function names for workspace_bytes = 0.  A call that runs as bulk + tail (petit_gemm_row_split): the kernel of the problem as a
 * whole -- resolve (rows) and (m - rows) for the two launches.  epilogue may be NULL.
 * A K too short for the split an id or a table row names runs as ONE slice (no reduce pass); the id keeps its split nibble.  With a gated
 * activation that is then the kernel's own epilogue's job: an explicit id whose kernel cannot apply it resolves to 0, and a default pick
 * names the kernel re-picked for it (split nibble 1) -- the one launched.  (Before the plan knew the launch geometry this query named
 * the table row's kernel there, which was not the one launched.) */
uint64_t petit_gemm_resolve_solution(const petit_solution_hints *hints, unsigned m, unsigned n, unsigned k, uint64_t solution_id,
                                     const petit_epilogue *epilogue, uint64_t workspace_bytes);
/* Rows are independent, so a default-pick call (PETIT_SOLUTION_AUTO) at a prefill M whose tile grid ends a little past a whole number
 * of rounds of the chip runs as TWO launches on the caller's stream: the first `rows` rows with the kernel picked for them (a grid of
 * whole rounds), the remaining m - rows rows as a default-pick problem of their own (petit-kernel_amd/csrc/pick.hip plan_row_split;
 * petit_gemm_workspace_bytes covers both).  When the process-wide MXFP4 default class is taken (petit_set_mxfp4_default_class), the
 * split is that class's (petit_gemm_row_split).  Returns `rows` for a call that hands over as much scratch as petit_gemm_workspace_bytes
 * asks for, or 0 when the call runs as one launch (always for explicit ids, m <= 512, $PETIT_AMD_NO_ROW_SPLIT=1).
 * petit_gemm_default_solution / _resolve_solution name the kernel of the problem as a whole; resolve them at (rows) and (m - rows) for
 * the two launches.  No reference counterpart: the reference's 234-kernel chooser (fp4/algo_chooser.cc:64-132) takes the grid as it comes. */
unsigned petit_gemm_auto_row_split(const petit_solution_hints *hints, unsigned m, unsigned n, unsigned k, const petit_epilogue *epilogue);
/* The same for any solution_id (round 6).  PETIT_SOLUTION_AUTO: as above.  A native-class sentinel: the rows the call runs IN THE CLASS when its grid of 128-row tiles
 * ends a little past a whole number of rounds -- the remaining few dozen rows (<= 128) then go through the default pick PETIT_SOLUTION_AUTO (a batched-decode kernel: the
 * class has no small-M kernel), which computes them exactly unless the process-wide MXFP4 default class is set and the tail has $PETIT_AMD_NATIVE_MIN_M (64) rows or more;
 * both parts share the call's scratch (petit_gemm_workspace_bytes_ex / petit_gemm_native_workspace_bytes cover both).  Only for calls that hand over 16-bit activations and
 * take a 16-bit result (no petit_native_args formats) and, for NVFP4 weights, through the entry point that has the packed tensors (the attached image).  0 = one launch
 * (always for explicit ids). */
unsigned petit_gemm_row_split(const petit_solution_hints *hints, unsigned m, unsigned n, unsigned k, uint64_t solution_id, const petit_epilogue *epilogue);
/* A test aid: the C tile (n-tile column *bn, m-tile row *bm) that workgroup `block` (= blockIdx.y * gridDim.x + blockIdx.x) of an nx x ny grid of the
 * large-M kernels computes under the XCD-aware raster with bands of `band` m-tiles (0 = whole columns) -- the very function the kernels call
 * (csrc/device_common.hpp tile_of_linear), so that its bijection is checked without a GPU.  No reference counterpart (the reference's grid is
 * blockIdx as is, gemm_fp4_fp16_grid.cuh:554-555). */
void petit_raster_tile(unsigned nx, unsigned ny, unsigned band, unsigned block, unsigned *bn, unsigned *bm);

/*
 * Offline repack of checkpoint tensors into the packed layout the GEMM reads
 * (petit-kernel_amd/csrc/layout.h).  Same byte counts in and out.
 *   in_chan = K, out_chan = N (argument order of the reference).
 *
 * petit_repack_nvfp4_weights   replaces fp4::RepackNvFp4ToPetitFp4Weights
 *     quantization/gemm.h:135-137 (impl fp4/quantization_utils.cu:729-746)
 *     input  u32 [N][K/8], nibble i of word k8 = element 8*k8+i
 *     needs  N % 16 == 0, K % 128 == 0   (lib/pybind/fp4.cc:40-43)
 *     Also used for MXFP4 weights (petit_kernel/__init__.py:27-28).
 * petit_repack_nvfp4_scales    replaces fp4::RepackNvFp4ToPetitFp4Scales
 *     quantization/gemm.h:139-141 (impl quantization_utils.cu:748-760)
 *     input  e4m3 [N][K/16];  needs N % 16 == 0, K % 256 == 0 (fp4.cc:82-92)
 * petit_repack_mxfp4_scales    replaces fp4::RepackMxFp4ToPetitFp4Scales
 *     quantization/gemm.h:143-145 (impl quantization_utils.cu:762-773)
 *     input  e8m0 [N][K/32];  needs N % 16 == 0, K % 256 == 0 (fp4.cc:126-135)
 *
 * Unlike the reference (which returns void and silently skips remainders,
 * quantization_utils.cu:734), these return PETIT_ERROR_PROBLEM_SHAPE for a
 * shape they cannot honour.
 */
int petit_repack_nvfp4_weights(unsigned *output, const unsigned *input,
                               unsigned in_chan, unsigned out_chan, void *stream);
int petit_repack_nvfp4_scales(unsigned *out_scales, const unsigned *scales,
                              unsigned in_chan, unsigned out_chan, void *stream);
int petit_repack_mxfp4_scales(unsigned *out_scales, const unsigned *scales,
                              unsigned in_chan, unsigned out_chan, void *stream);

/*
 * Dense dequantisation of PACKED weights, a debug / test aid:
 *   out[n][k] = fp4(b[n][k]) * scale[n][k / g] * global_scale     row-major [n][k]
 *   replaces DequantPetitFp4 / DequantPetitMxFp4  fp4/quantization_utils.cu:542-727 (the reference's test-only GPU
 *            dequant kernels, quantization_utils_fp4_test.cc:103-133)
 *   b, scales   packed tensors from petit_repack_*; b_type PETIT_DTYPE_FP4_E2M1 (e4m3 scales, g = 16) or
 *               PETIT_DTYPE_MXFP4_E2M1 (e8m0, g = 32); n % 16 == 0, k % 256 == 0
 *   out_type    PETIT_DTYPE_FP32 (exact for every code x scale), PETIT_DTYPE_BF16 or PETIT_DTYPE_FP16 (one RNE rounding)
 * Uses the same hardware converts and scale decode as the GEMM kernels; the GEMM never calls it.
 */
#define PETIT_DTYPE_FP32 100 /* (not in the reference's enum: only this entry point takes it) */
int petit_dequant_packed_weights(void *out, const unsigned *b, const unsigned *scales, float global_scale,
                                 unsigned n, unsigned k, int b_type, int out_type, void *stream);

/*
 * Offline twins of the three repack entry points for HOST memory: convert a checkpoint's native
 * NVFP4 / MXFP4 tensors into the packed layout on the CPU, so load-time GPU repack becomes
 * optional (the reference has no counterpart -- its repack exists only as
 * GPU kernels, quantization_utils.cu:208-304).  Same shapes, same bytes out as the device
 * versions (tests compare them bit for bit); out of place only.  These are NOT a CPU fallback of
 * the GEMM: the packed tensors are consumed by the GPU kernels alone.
 */
int petit_repack_nvfp4_weights_host(unsigned *output, const unsigned *input, unsigned in_chan, unsigned out_chan);
int petit_repack_nvfp4_scales_host(unsigned *out_scales, const unsigned *scales, unsigned in_chan, unsigned out_chan);
int petit_repack_mxfp4_scales_host(unsigned *out_scales, const unsigned *scales, unsigned in_chan, unsigned out_chan);

/*
 * Ingest of tensors that were already packed by the REFERENCE build (host memory, offline): a checkpoint repacked with
 * the reference wheel's repack_nvfp4 / process_*_scales is converted to this build's layout without going back to the
 * native tensors.  Input formats: RepackQWeightLayout64x32 + PetitFormat (quantization_utils.cu:20-87,183-253),
 * RepackScaleLayout64x32 with the e4m3 -> "e5m3" byte transform (:89-162,255-304), RepackMxScaleLayout64x32 (:165-181).
 * Same byte counts in and out, out of place only.  Weights: out_chan % 32 == 0, in_chan % 128 == 0; NV scales
 * out_chan % 64 == 0 (the reference's kernel tiles 64 x 64, :755); MX scales out_chan % 32 == 0; in_chan % 256 == 0.
 * The reference stores -0 as +0 (PetitFormat), which the conversion cannot and need not undo.
 */
int petit_convert_reference_weights_host(unsigned *output, const unsigned *input, unsigned in_chan, unsigned out_chan);
int petit_convert_reference_nvfp4_scales_host(unsigned *out_scales, const unsigned *scales, unsigned in_chan, unsigned out_chan);
int petit_convert_reference_mxfp4_scales_host(unsigned *out_scales, const unsigned *scales, unsigned in_chan, unsigned out_chan);

/*
 * Scratch memory ("workspace").  The reference API has no workspace argument (SURVEY.md section 8b "Ownership"); two
 * kinds of kernels here need device scratch: those that split K across workgroups (fp32 partial slabs, summed in a
 * fixed order by a second pass: deterministic, no float atomics) and the native-FP4 kernels (quantised activations).
 * petit_gemm_workspace_bytes() says how much a call needs; 0 for most kernels.
 *
 * Per call (preferred; the only form that is safe with several streams or concurrently running graphs):
 *   petit_gemm_*_ws(..., epilogue, workspace, workspace_bytes, stream) -- caller-owned device memory that must stay
 *   untouched until the work enqueued on `stream` by this call has finished (stream-ordered allocators give exactly
 *   that).  With PETIT_SOLUTION_AUTO a missing / too small workspace selects a kernel that needs none; with an
 *   explicit id that needs scratch it is PETIT_ERROR_KERNEL_SHAPE (none) / PETIT_ERROR_BAD_ARGUMENT (too small).
 *   epilogue may be NULL.  The Python layer allocates this per call from torch's caching allocator.
 * Registered (legacy convenience for single-stream programs): petit_set_workspace(ptr, bytes) per device; used by the
 *   entry points without a workspace argument.  One buffer cannot serve two streams at once: it binds to the first
 *   stream that uses it and calls from any other stream are refused with PETIT_ERROR_BAD_ARGUMENT (explicit ids) or
 *   fall back to a kernel without scratch (AUTO) until petit_set_workspace is called again.  Pass (NULL, 0) to
 *   unregister.  The memory stays owned by the caller.
 * Alignment: a workspace pointer (per call or registered) must be 256-byte aligned -- the kernels store f32x4 slabs
 *   and read the quantised activations with 16-byte loads at 256-byte-aligned offsets from it; a misaligned pointer is
 *   PETIT_ERROR_BAD_ARGUMENT, never a misaligned access.  (hipMalloc and torch allocations are 256 / 512-byte aligned.)
 */
int petit_gemm_fp4_fp16_grid_ws(unsigned *c, const unsigned *a, const unsigned *b,
                                const unsigned *scales, const float *global_scale,
                                unsigned m, unsigned n, unsigned k,
                                const petit_solution_hints *hints, uint64_t solution_id,
                                const petit_epilogue *epilogue, void *workspace, uint64_t workspace_bytes, void *stream);
int petit_gemm_mxfp4_fp16_grid_ws(unsigned *c, const unsigned *a, const unsigned *b,
                                  const unsigned *scales, const float *global_scale,
                                  unsigned m, unsigned n, unsigned k,
                                  const petit_solution_hints *hints, uint64_t solution_id,
                                  const petit_epilogue *epilogue, void *workspace, uint64_t workspace_bytes, void *stream);
/* Bytes of scratch the call (hints, m, n, k, solution_id) uses when it is given enough; solution_id may be
 * PETIT_SOLUTION_AUTO (the arch table may name a K-split kernel for the shape).  A call that runs as bulk + tail
 * (petit_gemm_row_split): the larger part's, and no less than the process-wide default class was taken for.  0: none
 * needed, or the call would be refused (an NVFP4 native-class call is taken to have its image attached). */
uint64_t petit_gemm_workspace_bytes(const petit_solution_hints *hints, unsigned m, unsigned n, unsigned k,
                                    uint64_t solution_id);
/* The same with the epilogue of the call taken into account: PETIT_SOLUTION_AUTO resolves differently under
 * PETIT_ACTIVATION_SILU_MUL (unsplit, only kernels that hold a gate / up tile pair per wave qualify; with a cross-workgroup K
 * split any kernel does -- the slabs hold the plain [m][n] product and the reduce pass applies SiLU-mul); PETIT_ACTIVATION_SWIGLU_OAI
 * resolves exactly as SILU_MUL does.  0 also for an explicit id that petit_gemm_resolve_solution refuses because its K split gives one
 * slice and its kernel cannot apply the gated activation itself (the launch step made that refusal before; this query named slab bytes). */
uint64_t petit_gemm_workspace_bytes_ex(const petit_solution_hints *hints, unsigned m, unsigned n, unsigned k,
                                       uint64_t solution_id, const petit_epilogue *epilogue);
int petit_set_workspace(void *device_ptr, uint64_t bytes);
/* fp32-slab bytes the split-K nibble of an id implies for (m, n) (kept for round-1 callers; prefer
 * petit_gemm_workspace_bytes, which also covers the native kernels). */
uint64_t petit_workspace_bytes(uint64_t solution_id, unsigned m, unsigned n);

/*
 * Native-FP4 kernels (no counterpart in the reference): MXFP4 weights go straight into the CDNA4
 * block-scaled MFMA and the 16-bit activations are quantised on the fly to MXFP8 (e4m3 + one e8m0
 * scale per 32 k), MXFP6 (e2m3: the same three mantissa bits over three binades, at the instruction's
 * FP4 rate; mfma_type 4) or MXFP4 (e2m1; mfma_type 6: experimental accuracy).  That quantisation costs
 * ~2^-4 (e4m3, e2m3) / 2^-2 (e2m1) relative per activation, so these kernels are a
 * different accuracy class: they are NEVER chosen by PETIT_SOLUTION_AUTO and are only enumerated
 * by petit_gemm_get_solutions after petit_enable_native_fp4(1) (or $PETIT_AMD_NATIVE_FP4=1).  Their
 * ids carry mfma_type = 2 (the reference's unused kMatmulMfmaTypeFp8, gemm.h:20-24).  They need a
 * registered workspace of petit_native_workspace_bytes(m, k) bytes for the quantised activations.
 *
 * Exactness of the class, given the quantised activations (derived from the instruction, not fitted: tools/probes/mfma_scale_align.hip,
 * profiles/r05_mfma_scale_align.txt; the same for v_mfma_scale_f32_32x32x64 and 16x16x128).
 *  (1) every activation format: the partial sums of one 32-element block and the incoming accumulator are aligned to the largest of them and each
 *      is TRUNCATED to a multiple of 2^(E - 24), E = floor(log2(largest)); the sum of the aligned values is exact.  A term in another block of the
 *      same instruction survives beside +-big of any size; with FP6 / FP4 activations a block's own sum is exact.
 *  (2) FP8 (e4m3) activations only: inside a block the products are first summed in groups of 8 consecutive k, aligned to the group's largest
 *      product and truncated 14 bits below it (unit 2^(e_a + e_w - 13)).
 * With P_b / P_g the largest |a w| of block b / group g, T the sum over blocks of |block sum| (no accumulation order or K split has a larger partial
 * sum) and gs the global scale, every output satisfies
 *     |c - exact| <= gs * [ 2^-24 * (33 * sum_b max(P_b, T) + 16 * T)  +  (FP8 activations) 7 * 2^-13 * sum_g P_g ]  +  one 16-bit rounding:
 * a worst case (every truncation a full unit, all in one direction) of ~1e-4 of sum |a w| for FP6 / FP4 activations and ~5e-4 for FP8 at K = 8192;
 * typical errors are one 16-bit rounding of the result.  The tests (tests/test_gpu_parity.py native_exact_bound) and tools/fuzz_parity.py hold every
 * native kernel to it; rounds 3-4 used an empirical 1e-5 ... 4e-5 of sum |a w|, which a longer fuzz run always exceeded somewhere.
 */
int petit_enable_native_fp4(int enable);
uint64_t petit_native_workspace_bytes(unsigned m, unsigned k);
/* A process-wide opt-in for call sites that cannot name a sentinel (an unchanged serving stack calls the MXFP4 entry points with
 * PETIT_SOLUTION_AUTO): activation_format 8 / 6 / 4 makes PETIT_SOLUTION_AUTO on MXFP4 weights run the default pick of THAT native
 * class (MXFP8 / MXFP6 / MXFP4 activations) for m >= $PETIT_AMD_NATIVE_MIN_M (default 64), whenever the call has the scratch the class
 * needs (petit_gemm_workspace_bytes(.., PETIT_SOLUTION_AUTO) then reports it; both Python layers pass it per call) -- without scratch the
 * exact default runs, as before.  0 switches it off (the default).  Initial value: $PETIT_AMD_MXFP4_ACTIVATIONS = mxfp8 | mxfp6 | mxfp4.
 * NVFP4 weights, explicit ids and the sentinels are not affected. */
int petit_set_mxfp4_default_class(int activation_format);
int petit_get_mxfp4_default_class(void);

/*
 * The native class as a PIPELINE (no counterpart in the reference).  petit_gemm_mxfp4_fp16_grid_ws with a native id runs two
 * launches per GEMM (activation quantiser, then the block-scaled-MFMA kernel).  Two hand-over points remove the quantiser:
 *   a_format   8 / 6 / 4: `a` is not the 16-bit matrix but activations ALREADY quantised to MXFP8 / MXFP6 / MXFP4 for (m, k), produced by
 *              petit_quantize_activations() (once, for any number of GEMMs that share the input: q / k / v, gate / up) or by
 *              a producer GEMM's epilogue (next item).  The bytes are opaque ("petit-qact/1": k-tile-major, the 32x32x64
 *              kernels' operand order); petit_quantized_activation_bytes() sizes them.  0: `a` is the 16-bit [m][k] matrix.
 *   out_format 8 / 6 / 4, with epilogue->activation = PETIT_ACTIVATION_SILU_MUL (or _SWIGLU_OAI: its value instead, quantised from f32 by
 *              the same rule): `c` receives silu(y_gate) * y_up QUANTISED for the
 *              next GEMM (m, k' = n / 2) -- petit_quantized_activation_bytes(m, n / 2, out_format) bytes -- instead of the
 *              16-bit [m][n/2] matrix: gate_up -> SiLU-mul -> down of a gated MLP in two launches.  Needs n % 512 == 0 and a
 *              kernel with 128 x 256 workgroup tiles (the sentinels pick one).  Quantised from the f32 result with the
 *              quantiser's own rule (E8M0 scale from the block maximum of 32 columns).
 * solution_id: PETIT_SOLUTION_AUTO_NATIVE_MXFP8 / _MXFP6 / _MXFP4 (must match a_format when given) or an explicit native kernel id;
 * with a_format or out_format set only the 32x32x64 kernels qualify (PETIT_ERROR_KERNEL_SHAPE otherwise).  hints->a_type
 * names the 16-bit type of the matrix input / output and of the bias.  workspace: what petit_gemm_native_workspace_bytes()
 * says for the same arguments (with a_format set: only the slabs of a K split; often 0; a call that runs as bulk + tail,
 * petit_gemm_row_split: the larger part's; 0 also when the call would be refused).
 */
typedef struct petit_native_args {
    uint32_t struct_bytes; /* sizeof(petit_native_args) */
    int32_t a_format;      /* 0, 8 (MXFP8), 6 (MXFP6 e2m3) or 4 (MXFP4) */
    int32_t out_format;    /* 0, 8, 6 or 4 */
    int32_t reserved;      /* 0 */
} petit_native_args;
int petit_gemm_mxfp4_native(void *c, const void *a, const unsigned *b, const unsigned *scales, const float *global_scale, unsigned m,
                            unsigned n, unsigned k, const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue,
                            const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream);
uint64_t petit_gemm_native_workspace_bytes(const petit_solution_hints *hints, unsigned m, unsigned n, unsigned k, uint64_t solution_id,
                                           const petit_epilogue *epilogue, const petit_native_args *native);
/* 16-bit activations [m][k] (a_type PETIT_DTYPE_BF16 / _FP16) -> "petit-qact/1" bytes of `format` (8 / 6 / 4) in qa; k % 256 == 0,
 * both pointers 16-byte aligned. */
uint64_t petit_quantized_activation_bytes(unsigned m, unsigned k, int format);
int petit_quantize_activations(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format, void *stream);

/*
 * RMSNorm into quantised activations (no counterpart in the reference).  Two of the three activation matrices a decoder layer quantises
 * come straight out of an RMSNorm (the inputs of qkv and of gate_up).  ONE launch computes
 *     h = x (+ residual),   y = RMSNorm(h) * (weight + weight_offset),   qa = petit_quantize_activations(y)
 * and can also write the updated residual h and the 16-bit y: no [m][k] 16-bit hand-over between the norm and the quantiser.
 *
 *   x, residual, y16, residual_out   [m][k] in a_type (PETIT_DTYPE_BF16 / _FP16); residual, y16 and residual_out may be NULL
 *   weight                           [k] in a_type
 *   qa                               petit_quantized_activation_bytes(m, k, format) bytes, format 8 / 6 / 4 (MXFP8 / MXFP6 / MXFP4): the layout
 *                                    petit_quantize_activations writes
 *
 * Arithmetic, f32 unless said otherwise; round16 = round to nearest even into a_type:
 *   1. with a residual h = round16(f32(x) + f32(residual)) -- the unfused h = x + r in the 16-bit type; that ROUNDED h is what residual_out
 *      receives and what the norm runs on.  Without: h = x, and residual_out must be NULL.
 *   2. S = the sum of h^2 over the row in ONE order, the same for every format, type and k: the row is cut into 8-element columns c = 0 ..
 *      k / 8 - 1; a column's partial is the ascending chain p = h0 h0, p = fma(h_i, h_i, p), i = 1 .. 7; thread t of 256 starts from +0 and adds the
 *      partials of its columns t, t + 256, ... in ascending order (a thread without a column holds +0); within each group of 64 consecutive
 *      threads s[t] = s[t] + s[t xor d] for d = 1, 2, 4, 8, 16, 32; S = ((s[0] + s[64]) + s[128]) + s[192].  Every product and sum is rounded once;
 *      nothing fuses but the stated fma.
 *   3. inv = 1 / sqrt(S * (1 / k) + eps): 1 / k, the product, the sum, the square root and the division each correctly rounded.
 *   4. y = round16((f32(h) * inv) * (f32(weight) + weight_offset)): three f32 operations, ONE rounding to the 16-bit type.  weight_offset is 0
 *      for Llama-style norms, 1 for Gemma-style.
 *   5. qa = exactly what petit_quantize_activations produces from that 16-bit y: the fused launch is bit for bit the two-step chain on y16, and
 *      the y16 a caller may also ask for is the same matrix (the exact tail of a row-split call or a router needs it).
 * Every consequence is part of the contract and mirrored by the host twin: a zero row gives inv = 1 / sqrt(eps) and zero blocks with scale
 * byte 127; a row whose squares overflow f32 (bf16 only) gives S = inf, inv = 0, y = +-0.
 *
 * y16 may alias x; residual_out may alias residual or x (a row is read completely before any of it is written).  qa must not overlap an input.
 *
 * Errors, all before any launch: PETIT_ERROR_PROBLEM_SHAPE for k % 256 != 0 (and m above 2^20, as everywhere); PETIT_ERROR_KERNEL_SHAPE for
 * k > 16384 (the row is held in registers) and for an a_type that is not bf16 / fp16; PETIT_ERROR_BAD_ARGUMENT for an eps that is not finite or
 * is <= 0, a weight_offset that is not finite, a null (qa, x, weight) or misaligned (16 bytes, any of the six) pointer, a residual_out without
 * a residual, a format other than 8 / 6 / 4.  m == 0 or k == 0 returns PETIT_OK.  No allocation, no host sync, graph-capturable.
 * petit_rmsnorm_quantize_host is the host twin (host pointers): bit-identical outputs, the same refusals.  petit_rmsnorm_inv_host writes the f32
 * `inv` of step 3 for each of the m rows, as the twin (and so the kernel) forms it -- a test aid: y carries inv only through a 16-bit rounding.
 * It refuses what petit_rmsnorm_quantize refuses for the arguments it takes (a_type, m, k > 16384, eps, a null or misaligned x / residual, a null
 * inv), except that k need only be a multiple of 8 (PETIT_ERROR_PROBLEM_SHAPE otherwise): the sum of step 2 is defined for any k / 8, and the
 * 16-bit-only form of petit_moe_combine_rmsnorm norms such rows.
 */
int petit_rmsnorm_quantize(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                           float weight_offset, unsigned m, unsigned k, int a_type, int format, void *stream);
int petit_rmsnorm_quantize_host(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                                float weight_offset, unsigned m, unsigned k, int a_type, int format);
int petit_rmsnorm_inv_host(float *inv, const void *x, const void *residual, float eps, unsigned m, unsigned k, int a_type);

/*
 * NVFP4 weights on the native class (no counterpart in the reference; BASELINE north_star: "a native fp4/fp8 MFMA variant").
 *
 * NVFP4's e4m3 group-16 scales do not fit the block-scaled MFMA (one E8M0 scale per 32 k), and multiplying the e4m3 mantissa into the elements
 * inside the GEMM costs what the exact kernels' unpack costs (petit-kernel_amd/csrc/nvnative.hip has the arithmetic).  So the weights are
 * re-encoded ONCE, at load time, into an MFMA-native image ("petit-cdna4-nv6/1", csrc/layout.h): per 32-k block of a weight row one E8M0 scale
 * 2^E, E = floor(log2(max |fp4 x e4m3|)) - 2, and FP6 e2m3 elements RNE(fp4 x e4m3 / 2^E) -- 6.25 bits per weight next to the 4.5 of the packed
 * tensors, which the exact kernels (every decode call) keep reading.  The instruction then runs at the rate of the ACTIVATION format: MXFP6 / MXFP4
 * activations at the FP4 rate, MXFP8 at the FP8 rate; global_scale stays in the epilogue.
 *
 * Accuracy class: the native class's (quantised activations, see above) PLUS the re-rounding of the weights: fp4 x e4m3 has up to 6 significant
 * bits, e2m3 keeps 4, and the group with the smaller scale of a block loses one more bit per binade of distance.  Per element
 *     |w_image - w_nvfp4| <= 2^-4 |w_nvfp4|  (elements >= 2^E, i.e. within 3 binades of the block maximum),   <= 2^(E-4)  below,
 * hence per output |c_image - c_nvfp4| <= gs * sum_k |a_k| * max(2^-4 |w_k|, 2^(E_k - 4)).  On weights quantised by the checkpoint recipe
 * (tools/quantize_weights.py) 22-38 % of the elements move, by 2.3 % rms of the weight: the weight's total quantisation error goes from 9.51 % to
 * 9.79 % of its rms (profiles/r06_nv6_reencode.md; MLP / stacked budgets: profiles/r06_*accuracy_budget*.json).  Given the image and the
 * quantised activations the kernels are exact in the sense of "Exactness of the class" above (same instruction, same bound).
 *
 *   petit_nvfp4_native_image_bytes(in_chan = K, out_chan = N)    bytes of the image (0 for a shape the class does not take: N % 16, K % 256)
 *   petit_nvfp4_native_image(image, b, scales, K, N, stream)     device: from the PACKED tensors of petit_repack_nvfp4_weights / _scales;
 *                                                                image 256-byte aligned; N * K * 3 / 4 < 2^32
 *   petit_nvfp4_native_image_host                                host twin, bit-identical (offline conversion; packed host tensors from
 *                                                                petit_repack_nvfp4_*_host)
 *   petit_nvfp4_native_image_dequant_host(out, image, K, N)      test / debug aid: out[n][k] f32 = element x 2^(scale - 127), no global scale
 *   petit_nvfp4_native_images(images, b, scales, E, K, N, expert_offsets, m, stream)
 *                                                                the images of E stacked experts back to back in ONE launch: expert e reads byte
 *                                                                e N K / 2 of b and e N K / 16 of scales and writes byte
 *                                                                e * petit_nvfp4_native_image_bytes(K, N) of images -- what petit_gemm_native_moe
 *                                                                reads.  Shapes and alignment per expert as petit_nvfp4_native_image; E in
 *                                                                1 .. PETIT_MOE_MAX_EXPERTS.  expert_offsets NULL: every expert.  Otherwise the
 *                                                                device int32 [E + 1] offsets of a MoE launch over m grouped rows (never read by
 *                                                                the host): an expert to which that launch gives no rows -- each offset clamped
 *                                                                into [its predecessor, m], then a count of 0 -- is skipped, its region left
 *                                                                untouched.  No host sync, no allocation: capturable.
 *   petit_nvfp4_native_images_host                               host twin, bit-identical, the same skip; expert_offsets in HOST memory
 *
 * Running it -- two ways, same kernels:
 *   petit_gemm_nvfp4_native(c, a, image, ...)   names the image per call; solution_id = PETIT_SOLUTION_AUTO_NATIVE_MXFP8 / _MXFP6 / _MXFP4 (the
 *       activation format) or an explicit native id of the NVFP4 family; native / workspace exactly as petit_gemm_mxfp4_native (pre-quantised
 *       activations, the quantising SiLU-mul epilogue, petit_gemm_native_workspace_bytes with hints->b_type = PETIT_DTYPE_FP4_E2M1).
 *   petit_nvfp4_native_attach(b, image)         for call sites that keep calling the reference's entry point: afterwards
 *       petit_gemm_fp4_fp16_grid_ws(c, a, b, scales, ..., PETIT_SOLUTION_AUTO_NATIVE_*, ...) -- mul_nvfp4_a16(..., solution_id = -2 / -3 / -4) --
 *       runs on the image attached to `b`.  The image stays the caller's memory and must outlive the attachment; image = NULL detaches.  A
 *       sentinel (or explicit native id) on weights without an image returns PETIT_ERROR_KERNEL_SHAPE -- never another accuracy class.
 * PETIT_SOLUTION_AUTO on NVFP4 weights is never affected: it stays the exact class.  Both entry points refuse an explicit id of the exact class on an
 * image (PETIT_ERROR_KERNEL_SHAPE).
 *
 * Without a resident image -- petit_gemm_nvfp4_native_transient(c, a, b, scales, ...): b / scales are the PACKED tensors (what
 * petit_gemm_fp4_fp16_grid_ws takes); the call builds the image into its workspace, then runs the native call on it, in stream order on `stream`.
 * Nothing is registered or cached: two calls with different weights may share one workspace one after the other, and a captured call reads b / scales
 * anew at every replay.  The weights then cost 4.5 bits each plus ONE workspace the size of the largest layer's image, shared by all layers.
 *   workspace layout: [0, I) the image, I = petit_nvfp4_native_image_bytes(k, n) rounded up to 256; [I, I + S) exactly the scratch the planned native
 *       call needs.  petit_gemm_nvfp4_native_transient_workspace_bytes returns I + S, read from the launcher's plan (0: the call would be refused).
 *   solution_id: PETIT_SOLUTION_AUTO_NATIVE_MXFP8 / _MXFP6 / _MXFP4 or an explicit native id of the NVFP4 family; PETIT_SOLUTION_AUTO and exact-class
 *       ids: PETIT_ERROR_KERNEL_SHAPE.  N % 16, K % 256 or an element part of 2^32 bytes or more: PETIT_ERROR_PROBLEM_SHAPE.  A workspace that is
 *       missing (the registered one is never used), too small or not 256-byte aligned: the rules of petit_gemm_nvfp4_native.  Every refusal happens
 *       before the first launch: C is untouched and nothing enters a stream capture.
 *   results: bit for bit those of the attached-image call it stands for -- with native NULL or both formats 0, petit_gemm_fp4_fp16_grid_ws(..., the
 *       sentinel) on b with the image attached, its bulk + tail row split at a ragged M included (the image is built once, before the bulk; the exact
 *       tail reads b / scales); with pre-quantised activations or a quantised SiLU-mul output, petit_gemm_nvfp4_native on the same image.
 */
uint64_t petit_nvfp4_native_image_bytes(unsigned in_chan, unsigned out_chan);
int petit_nvfp4_native_image(void *image, const unsigned *b, const unsigned *scales, unsigned in_chan, unsigned out_chan, void *stream);
int petit_nvfp4_native_image_host(void *image, const unsigned *b, const unsigned *scales, unsigned in_chan, unsigned out_chan);
int petit_nvfp4_native_image_dequant_host(float *out, const void *image, unsigned in_chan, unsigned out_chan);
int petit_nvfp4_native_images(void *images, const void *b, const void *scales, unsigned num_experts, unsigned in_chan, unsigned out_chan,
                              const int32_t *expert_offsets, unsigned m, void *stream);
int petit_nvfp4_native_images_host(void *images, const void *b, const void *scales, unsigned num_experts, unsigned in_chan, unsigned out_chan,
                                   const int32_t *expert_offsets /* host */, unsigned m);
int petit_nvfp4_native_attach(const void *b, const void *image);
const void *petit_nvfp4_native_attached(const void *b);
int petit_gemm_nvfp4_native(void *c, const void *a, const void *image, const float *global_scale, unsigned m, unsigned n, unsigned k,
                            const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue,
                            const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream);
int petit_gemm_nvfp4_native_transient(void *c, const void *a, const unsigned *b, const unsigned *scales, const float *global_scale, unsigned m, unsigned n,
                                      unsigned k, const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue,
                                      const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream);
uint64_t petit_gemm_nvfp4_native_transient_workspace_bytes(const petit_solution_hints *hints, unsigned m, unsigned n, unsigned k, uint64_t solution_id,
                                                           const petit_epilogue *epilogue, const petit_native_args *native);

/*
 * Weight quantiser (no counterpart in the reference, whose callers arrive with FP4 checkpoints): 16-bit weights -> the PACKED tensors and the
 * global scales the GEMMs read, in one pass over the weights (NVFP4 without a supplied scale: two), for a stack that loads a bf16 / fp16
 * checkpoint or receives fresh 16-bit weights while it serves.  No row-major FP4 intermediate, no repack launch.
 *
 *   w           [num_experts][n][k], a_type PETIT_DTYPE_BF16 / _FP16, contiguous, 16-byte aligned; num_experts = 1 is a plain linear.
 *               n % 16 == 0, k % 256 == 0 (what the scale repack asks).  Every expert is quantised on its own.
 *   b_type      PETIT_DTYPE_FP4_E2M1 (NVFP4) or PETIT_DTYPE_MXFP4_E2M1
 *   out_b       what petit_repack_nvfp4_weights makes of the row-major FP4 of the stacked [num_experts n, k] matrix (n k / 2 bytes per expert, expert
 *               e at e times that); out_scales what petit_repack_nvfp4_scales (n k / 16 bytes per expert) / petit_repack_mxfp4_scales (n k / 32)
 *               makes of its scales; both 16-byte aligned.  out_gs: float32 [num_experts], the global_scale(s) of the GEMM entry points.
 *   gs_in       NVFP4 only: null, or float32 [num_experts] positive finite global scales of the caller (calibrated, or shared between tensors);
 *               then there is no amax pass.  May be out_gs.  Ignored for MXFP4.
 *   workspace   petit_quantize_weights_workspace_bytes(b_type, num_experts, gs_in != NULL) bytes of device scratch, 4-byte aligned (0: may be
 *               null): the per-expert maxima, zeroed on the stream by the call.
 *
 * The rule.  mid = {0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5}, the midpoints of the e2m1 magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}.
 *   NVFP4 (the recipe of the nvidia FP4 checkpoints, every step named):
 *     global scale  amax_e = max |w_e|;  gs_e = amax_e / 2688.0f, ONE correctly rounded f32 division (2688 = 6 x 448);  gs_e = 1.0f when
 *                   amax_e == 0.  With gs_in: gs_e = gs_in[e].
 *     block scale   per 16 consecutive k of a row: byte = e4m3fn_rne( f32( f32(blk_amax / 6.0f) / gs_e ) ), saturating at 448 (0x7e).
 *     codes         s = the decoded byte; t_i = mid_i * s * gs_e EXACTLY (3 + 4 + 24 significant bits: an f64 product).  The magnitude code is the
 *                   number of t_i < |w|; at |w| == t_i the even one of i, i + 1; the sign bit is set only with a non-zero magnitude code
 *                   (there is no -0).  s == 0 gives code 0 for the whole block.
 *   MXFP4 (OCP MX):
 *     scale         per 32 consecutive k: e = the smallest integer with 6 * 2^e >= blk_amax, clipped to [-126, 127]; byte = e + 127 (a zero
 *                   block: 1).  No element clips.
 *     codes         round to nearest even on the e2m1 grid of w / 2^e (the count above with t_i = mid_i * 2^e), saturating, no -0.
 *     global scale  gs_e = 1.0f.
 *   Non-finite weights give unspecified values, never a fault.
 *
 * petit_quantize_weights_host is the CPU twin on host memory: same arguments without scratch and stream, the same bytes out (offline conversion).
 * Errors, all before any launch: PETIT_ERROR_BAD_ARGUMENT for an a_type / b_type outside the above, null or misaligned pointers, a workspace
 * that is too small; PETIT_ERROR_PROBLEM_SHAPE for n % 16, k % 256 or num_experts * n >= 2^32; PETIT_ERROR_KERNEL_SHAPE for a call that needs
 * scratch and has none.  num_experts, n or k == 0 returns PETIT_OK.  No host sync, no allocation: capturable; a replay quantises what w holds then.
 */
uint64_t petit_quantize_weights_workspace_bytes(int b_type, unsigned num_experts, int gs_supplied);
int petit_quantize_weights(const void *w, int a_type, int b_type, unsigned num_experts, unsigned n, unsigned k, const float *gs_in, void *out_b,
                           void *out_scales, float *out_gs, void *workspace, uint64_t workspace_bytes, void *stream);
int petit_quantize_weights_host(const void *w, int a_type, int b_type, unsigned num_experts, unsigned n, unsigned k, const float *gs_in,
                                void *out_b, void *out_scales, float *out_gs);

/*
 * Grouped launch (no counterpart in the reference): up to PETIT_GROUP_MAX weight matrices that share the activation rows --
 * q / k / v (or their tensor-parallel shards) kept as separate tensors, gate and up, the experts a token routes to -- in ONE
 * kernel launch: c_i[m][n_i] = a[m][k] . dequant(b_i)[n_i][k]^T * (*global_scale_i) (+ bias_i).  At decode batch sizes a
 * TP-8 shard's GEMM takes 3-4 us of which ~1.6 us is the dependent-dispatch gap between launches on MI355X; a group pays it
 * once.  Same numerics, bit for bit, as count separate calls with the same kernel id.
 *   m <= 16 (larger m is not launch-bound: PETIT_ERROR_KERNEL_SHAPE, call per member); every n_i % 16 == 0, k % 256 == 0;
 *   hints->b_type selects NVFP4 or MXFP4 for ALL members; solution_id PETIT_SOLUTION_AUTO (picked for the concatenated
 *   problem) or the id of a decode / staged streaming kernel; no scratch, no SiLU-mul.
 */
#define PETIT_GROUP_MAX 8
typedef struct petit_group_member {
    void *c;                   /* [m][n] output, hints->c_type */
    const void *b;             /* packed weights of this member */
    const void *scales;        /* packed scales */
    const float *global_scale; /* device pointer */
    const void *bias;          /* [n] or NULL */
    uint32_t n;
    uint32_t reserved;         /* 0 */
} petit_group_member;
int petit_gemm_fp4_fp16_grouped(const petit_group_member *members, unsigned count, const unsigned *a, unsigned m, unsigned k,
                                const petit_solution_hints *hints, uint64_t solution_id, void *stream);

/*
 * Routed-expert (MoE) launch (no counterpart in the reference): the E experts of a mixture-of-experts layer in ONE kernel launch,
 * each on its own subset of the token rows:  rows r in [expert_offsets[e], expert_offsets[e+1]) of a belong to expert e, and
 *     c[r][:] = a[r][:] . dequant(b_e)[n][k]^T * global_scales[e] (+ bias[e][:])          (SiLU-mul: silu(gate) * up, c is [m][n/2])
 *   a               [m][k], hints->a_type (16-bit), rows ALREADY GROUPED by expert; c has the same row order, hints->c_type == a_type.
 *   b, scales       the E experts' packed tensors back to back: expert e's block is exactly what repack_nvfp4 / process_nvfp4_scales /
 *                   process_mxfp4_scales make of its [n, k] weight.  The packed layout is n-tile-major, so packing the stacked [E*n, k]
 *                   weight (and its [E*n, k/16] or [E*n, k/32] scales) in ONE call gives the same bytes: callers may repack the stacked tensor.
 *   global_scales   float32 device array [E].
 *   expert_offsets  int32 device array [E + 1]: offsets[0] = 0, non-decreasing, offsets[E] = m.  The host never reads it: the call makes no
 *                   host sync and may be captured in a graph whose replays route differently.
 *   epilogue        optional: bias is read as [E][n] in c's dtype; activation = PETIT_ACTIVATION_SILU_MUL takes each expert's weight as
 *                   [gate; up] along N (vLLM / SGLang's w13) and writes c as [m][n/2]; PETIT_ACTIVATION_SWIGLU_OAI the same with gpt-oss's clamped
 *                   formula (a gpt-oss checkpoint stores gate / up rows interleaved: de-interleave them first, petit_kernel.gptoss does).
 *   solution_id     PETIT_SOLUTION_AUTO, or the id of a kernel that has a MoE form (a decode, staged streaming or tiled kernel of a curated
 *                   subset; no K split): the dense ids, petit_describe_solution names them.  Within an expert the result equals, bit for bit,
 *                   a dense call on that expert's rows with the same id.
 * Shapes: n % 16 == 0 (MXFP4: n % 32 == 0), k % 256 == 0, 1 <= E <= PETIT_MOE_MAX_EXPERTS; PETIT_ERROR_PROBLEM_SHAPE for other shapes and
 * for null pointers, PETIT_ERROR_KERNEL_SHAPE for an id without a MoE form (or when the routing bound ceil(m / rows per workgroup) +
 * min(E, m) exceeds the grid).  No workspace, no K split across workgroups.
 * Robustness: the kernel clamps every offset it reads into [offsets[e-1], m], so malformed offsets can only leave rows of c unwritten;
 * they never make it read or write out of bounds.  An expert without rows is never touched: its weights are not read.
 * petit_gemm_moe_resolve_solution() returns the id the call would run (0: refused) -- the launcher uses the same pick.
 */
#define PETIT_MOE_MAX_EXPERTS 1024
int petit_gemm_fp4_fp16_moe(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                            const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                            const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue, void *stream);
uint64_t petit_gemm_moe_resolve_solution(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                         uint64_t solution_id, const petit_epilogue *epilogue);

/*
 * Indexed MoE launch: petit_gemm_fp4_fp16_moe with a row gather on A and a row scatter on C, so that a layer needs neither a copy of
 * the activations in expert order nor an un-permute of the output.  Grouped row r (r in [expert_offsets[e], expert_offsets[e+1]): expert
 * e, as above) reads row a_row_index[r] of a [a_rows][k] and writes row c_row_index[r] of c [c_rows][n] ([c_rows][n/2] with SiLU-mul).
 *   a_row_index, c_row_index   int32 device arrays [m], or null for the identity (a_rows / c_rows must then be >= m).  Never read by the host.
 *   An A index outside [0, a_rows) reads zeros; a C index outside [0, c_rows) stores nothing (rows of c no index names stay untouched).
 *   expert_offsets[E] may be < m: grouped rows past it belong to no expert and are not computed (petit_moe_align's unrouted entries).
 * Same pick, same ids and, within an expert, the same numbers bit for bit as petit_gemm_fp4_fp16_moe: every kernel with a MoE form has an
 * indexed one.  With both indices null the call IS petit_gemm_fp4_fp16_moe.  PETIT_ERROR_PROBLEM_SHAPE also when an index is given and
 * a_rows * k * 2 > 2^31 (the bytes one 32-bit buffer descriptor of A can bound-check with an out-of-range marker to spare).
 */
int petit_gemm_fp4_fp16_moe_ex(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                               const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                               const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                               const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue, void *stream);

/*
 * Routing on the device (no host sync, graph-capturable, deterministic: no result depends on the order of atomics).
 * petit_moe_align: topk_ids [num_tokens][topk] (int32, or int64 when ids_are_int64) -> the grouped order of the MoE launches:
 *   sorted_pos    int32 [num_tokens * topk]: the flat (token, slot) positions p = token * topk + slot grouped by expert, ascending inside an
 *                 expert (a stable sort by expert id).
 *   token_index   int32 [num_tokens * topk]: sorted_pos[r] / topk (the A row index of gate_up).
 *   expert_offsets int32 [num_experts + 1], as petit_gemm_fp4_fp16_moe reads it.
 *   Ids outside [0, num_experts) (-1: an expert that is not local under expert parallelism) are not routed: they get no row, and
 *   expert_offsets[E] counts the routed entries.  Rows r >= expert_offsets[E] of sorted_pos / token_index are set to -1.
 *   workspace     petit_moe_align_workspace_bytes() bytes of device scratch (0: may be null); one or three launches.
 * petit_moe_combine: the top-k reduce of a layer, out[t][:] = to16(acc) with acc = 0 and, for j = 0 .. topk-1 in order, skipping ids
 *   outside [0, num_experts):  acc = acc + float(slot_out[t * topk + j][:]) * topk_weights[t][j]   (fp32, no FMA contraction, one
 *   round-to-nearest-even at the end).  slot_out [num_tokens * topk][n] and out [num_tokens][n] in dtype (PETIT_DTYPE-style: 4 fp16,
 *   5 bf16), topk_weights float32 [num_tokens][topk], n % 8 == 0.  Slots of unrouted entries are never read.
 * Errors: PETIT_ERROR_PROBLEM_SHAPE for null pointers, topk == 0, num_experts outside 1..PETIT_MOE_MAX_EXPERTS, num_tokens * topk >= 2^31,
 * n % 8 != 0; PETIT_ERROR_BAD_ARGUMENT for another dtype.
 */
uint64_t petit_moe_align_workspace_bytes(unsigned num_tokens, unsigned topk, unsigned num_experts);
int petit_moe_align(const void *topk_ids, int ids_are_int64, unsigned num_tokens, unsigned topk, unsigned num_experts, int32_t *expert_offsets,
                    int32_t *sorted_pos, int32_t *token_index, void *workspace, void *stream);
int petit_moe_combine(void *out, const void *slot_out, const float *topk_weights, const void *topk_ids, int ids_are_int64, unsigned num_tokens,
                      unsigned topk, unsigned n, unsigned num_experts, int dtype, void *stream);

/*
 * Top-k combine into the norm: petit_moe_combine, the residual add, the RMSNorm and (optionally) the activation quantiser in ONE launch -- the
 * end of a routed-expert layer and the head of the next block, without the 16-bit [num_tokens][k] matrix and the launch boundary between them.
 *
 *   slot_out                     [num_tokens * topk][k] in a_type (PETIT_DTYPE_BF16 / _FP16); topk_weights float32 [num_tokens][topk];
 *                                topk_ids int32, or int64 when ids_are_int64, [num_tokens][topk]
 *   residual, residual_out, y16  [num_tokens][k] in a_type; each may be NULL (y16 not with format 0)
 *   weight                       [k] in a_type
 *   format                       8 / 6 / 4 as petit_rmsnorm_quantize (qa: petit_quantized_activation_bytes(num_tokens, k, format) bytes), or
 *                                0 = no quantised output: qa must be NULL and y16 must not be
 *
 * Per token t, in this order (f32 unless said otherwise; round16 = round to nearest even into a_type):
 *   1. c = the row petit_moe_combine writes for t: acc = +0; for j = 0 .. topk-1 in order, skipping ids outside [0, num_experts),
 *      acc = acc + f32(slot_out[t * topk + j][:]) * topk_weights[t][j], the product and the sum each rounded, nothing fused; c = round16(acc).
 *      Slot rows of skipped entries are never read.
 *   2. h = round16(f32(c) + f32(residual)) with a residual, else h = c.  residual_out, when given, receives h IN BOTH CASES: without a
 *      residual it is the combined layer output itself (wider than petit_rmsnorm_quantize's rule, so a caller can still have that matrix).
 *   3. steps 2 - 5 of "RMSNorm into quantised activations" above, word for word, on that h: the same summation order (for any k / 8: a thread
 *      without a column holds +0), the same inv, the same single rounding into y, and qa exactly what petit_quantize_activations makes of y.
 * Whenever the chain accepts the call (k % 256 == 0, a format, a residual when residual_out is wanted) the outputs are bit for bit those of
 * petit_moe_combine -> petit_rmsnorm_quantize(residual = ...) on the same inputs.  With format 0 only y16 and residual_out are written, for any
 * k % 8 == 0 (gpt-oss: 2880).  A token whose slots are all unrouted has c = +0: h = residual, or a zero row with scale bytes 127.
 *
 * residual_out may alias residual: a thread reads from the residual row only the columns it then writes (a lane without a column reads the
 * weight row in its place, never the residual row).  y16, residual_out and qa must not overlap slot_out (other workgroups are still reading
 * it) or weight; qa must not overlap any input.
 *
 * Errors, all before any launch: PETIT_ERROR_PROBLEM_SHAPE for k % 8 != 0, k % 256 != 0 with a format, topk == 0, num_experts outside
 * 1..PETIT_MOE_MAX_EXPERTS, num_tokens * topk >= 2^31, num_tokens above 2^20; PETIT_ERROR_KERNEL_SHAPE for k > 16384 (the row is held in
 * registers) and for an a_type that is not bf16 / fp16; PETIT_ERROR_BAD_ARGUMENT for an eps that is not finite or is <= 0, a weight_offset
 * that is not finite, a null slot_out / topk_weights / topk_ids / weight, a pointer among (qa, y16, residual_out, slot_out, residual, weight)
 * that is not 16-byte aligned, a format outside {0, 8, 6, 4}, format 0 with a qa or without a y16, a format without a qa.  num_tokens == 0 or
 * k == 0 returns PETIT_OK.  No allocation, no host sync, graph-capturable.  petit_moe_combine_rmsnorm_host is the host twin (host pointers):
 * bit-identical outputs on every number (a NaN accumulator gives a NaN, its payload is not pinned), the same refusals.
 * petit_rmsnorm_inv_host takes any k % 8 == 0, so the norm of a format-0 row can be checked through it.
 */
int petit_moe_combine_rmsnorm(void *qa, void *y16, void *residual_out, const void *slot_out, const float *topk_weights, const void *topk_ids,
                              int ids_are_int64, const void *residual, const void *weight, float eps, float weight_offset, unsigned num_tokens,
                              unsigned topk, unsigned k, unsigned num_experts, int a_type, int format, void *stream);
int petit_moe_combine_rmsnorm_host(void *qa, void *y16, void *residual_out, const void *slot_out, const float *topk_weights, const void *topk_ids,
                                   int ids_are_int64, const void *residual, const void *weight, float eps, float weight_offset,
                                   unsigned num_tokens, unsigned topk, unsigned k, unsigned num_experts, int a_type, int format);

/*
 * Routing on the device, from the router's logits: petit_moe_route turns router_logits [num_tokens][num_experts] (contiguous; logits_dtype
 * PETIT_DTYPE_FP32 / _BF16 / _FP16, converted to fp32 exactly) into the top-k ids and weights the calls above read.  One launch, one wave
 * per token; no host sync, graph-capturable, no result depends on the order of atomics (there are none).
 *
 * Definition.  Two scorings (petit_route_desc.scoring):
 *   PETIT_ROUTE_SOFTMAX (Mixtral, Qwen3-MoE, gpt-oss): the selection key of expert e is its logit.  Weights: with renormalize != 0 the
 *     softmax over the k selected logits (this IS "softmax over all, top-k, divide by the sum", and is gpt-oss's "top-k, then softmax over
 *     the k"); with renormalize == 0 the softmax over all E, taken at the selected experts.  Max-subtracted, fp32.
 *   PETIT_ROUTE_SIGMOID (DeepSeek-V3 / R1 and descendants): s_e = sigmoid(logit_e); key = s_e + bias[e] (one fp32 add; bias float32 [E],
 *     null = 0).  With n_group > 1: the experts form n_group contiguous groups of E / n_group; a group's score is the fp32 sum of its two
 *     largest keys (largest first); the topk_group groups with the largest scores are kept and only their experts can be selected.
 *     Weights: the UNBIASED s_e of the selected experts, divided by (their sum + 1e-20) when renormalize, then times routed_scaling_factor.
 *   Selection, both scorings, experts and groups alike: larger key first; among equal keys the LOWER index first (-0 equals +0).  The k ids
 *     of a token are written in selection order (slot 0 = best) and are distinct.  A NaN key ranks below every number (as -inf; among
 *     themselves by index), so ids are always distinct and inside [0, E); the weights of a row that holds a NaN or a +inf (or only -inf)
 *     are unspecified, its ids are not.
 *   Outputs: topk_ids int32 [T][topk], topk_weights float32 [T][topk] (what petit_moe_align / petit_moe_combine read) and, when keys_out is
 *     not null, keys_out float32 [T][E]: the selection keys the kernel ranked (softmax: the logits, bit for bit).
 *
 * Accuracy of the weights, relative to the definition evaluated exactly on the same fp32 logits (u = 2^-24; expf and the fp32 divide are
 * the device library's: expf within 1 ulp = 2 u, the divide correctly rounded = 1 u; D = the largest |logit - row max| among the terms):
 *   the kernel's sequence is  d = x - max (1 rounding of d: a factor exp(+-u D / 2) on the term, <= u D / 2),  t = expf(d) (2 u),  the sum
 *   of positive terms -- the k selected ones in a 6-deep tree over the lanes, or for renormalize == 0 each lane's <= 16 experts in order and
 *   then that tree, <= 21 additions deep (1 u per level) --,  t / sum (1 u),  times the scaling factor (1 u).
 *     softmax, renormalize:      (2 + D/2) + (2 + D/2 + 6) + 1 + 1  = (12 + D) u
 *     softmax, all E:            (2 + D/2) + (2 + D/2 + 21) + 1 + 1 = (27 + D) u
 *     sigmoid: s = 1 / (1 + expf(-x)): expf 2 u (damped by e / (1 + e) <= 1), the add 1 u, the divide 1 u: 4 u on s.  Without renormalize
 *       4 + 1 = 5 u; with: 4 + (4 + 6 + 1 for the 1e-20) + 1 + 1 = 17 u.  A key is s + bias: |key error| <= 4 u s + u |key|.
 *   For logits within 16 of their row's maximum every case is below 48 u < 2^-18, far inside the 2^-16 the 16-bit layers could see.
 *
 * petit_moe_route_align: petit_moe_route followed by petit_moe_align on its ids, same outputs bit for bit.  When num_tokens * topk <= 1024
 * (the align's one-launch case, every decode batch) it is ONE launch: the align's workgroup routes the tokens first.  Above: the route
 * launch, then the align's three.  workspace: petit_moe_route_align_workspace_bytes() = petit_moe_align_workspace_bytes().
 *
 * Errors, all before any launch: PETIT_ERROR_PROBLEM_SHAPE for null pointers, topk == 0, topk > num_experts, topk > PETIT_MOE_MAX_TOPK,
 * num_experts outside 1..PETIT_MOE_MAX_EXPERTS, num_tokens * topk >= 2^31, num_experts % n_group != 0, groups of fewer than 2 experts,
 * topk_group outside 1..n_group, topk > topk_group * (E / n_group), groups or a bias with the softmax scoring, several chunks without a
 * workspace; PETIT_ERROR_BAD_ARGUMENT for a logits_dtype or scoring that does not exist.  num_tokens == 0 is PETIT_OK (petit_moe_route_align
 * then writes the all-zero expert_offsets, as petit_moe_align does).  desc null = a zero-initialised one.
 * An expert map for expert parallelism and shared experts: the _ex entries below.  From the hidden state: "The router's GEMM" below.
 * Not here: auxiliary-loss outputs beyond keys_out.
 */
#define PETIT_ROUTE_SOFTMAX 0
#define PETIT_ROUTE_SIGMOID 1
#define PETIT_MOE_MAX_TOPK 64
typedef struct petit_route_desc { /* zero-initialised = softmax, no renormalise, no groups */
    int scoring;                  /* PETIT_ROUTE_SOFTMAX | PETIT_ROUTE_SIGMOID */
    int renormalize;
    unsigned n_group, topk_group; /* 0 or 1: no groups.  Groups need scoring == PETIT_ROUTE_SIGMOID */
    float routed_scaling_factor;  /* 0 is read as 1 */
    const float *bias;            /* [num_experts] or null; PETIT_ROUTE_SIGMOID only */
} petit_route_desc;
int petit_moe_route(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                    const petit_route_desc *desc, int32_t *topk_ids, float *topk_weights, float *keys_out, void *stream);
uint64_t petit_moe_route_align_workspace_bytes(unsigned num_tokens, unsigned topk, unsigned num_experts);
int petit_moe_route_align(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                          const petit_route_desc *desc, int32_t *topk_ids, float *topk_weights, float *keys_out, int32_t *expert_offsets,
                          int32_t *sorted_pos, int32_t *token_index, void *workspace, void *stream);

/*
 * The complete slot list in the route launch: petit_moe_route_ex / petit_moe_route_align_ex take petit_moe_route's arguments and a
 * petit_route_slots, and write what petit_moe_align and petit_moe_combine read for a layer with an expert map (expert parallelism) and
 * shared experts (DeepSeek-V3 / R1, Llama-4, Qwen2-MoE: "shared-experts fusion", the shared expert as one more expert that every token
 * routes to).  slots null or zero-initialised is petit_moe_route / petit_moe_route_align exactly; those ARE the _ex entries with null slots.
 *
 * Definition.  L = num_local_experts (0 = num_experts), S = num_shared.  topk_ids int32 [T][topk + S], topk_weights float32 [T][topk + S]:
 *   Slots 0 .. topk-1, the routed experts: selection, order and weights are petit_moe_route's, bit for bit.  The weights come from the
 *     GLOBAL selection: a renormalisation runs over all topk selected experts, local or not -- what an all-reduce of the ranks' partial
 *     layer outputs needs.  The id written is expert_map[e] for the selected global expert e (int32 [num_experts]; null = e itself); a
 *     mapped value outside [0, L) is written as -1 (not local: petit_moe_align gives it no row, petit_moe_combine skips it).
 *   Slots topk + s, s < S, the shared experts: id L + s; weight shared_weight (0 is read as 1), or with shared_gate_logits ([T][S],
 *     logits_dtype; Qwen2-MoE's shared_expert_gate)  shared_weight * sigmoid(gate_logit[t][s]): the route's own fp32 sigmoid and one
 *     multiply.  Accuracy, as above: 4 u on the sigmoid plus 1 u for the product, 5 u.  routed_scaling_factor does not touch shared slots.
 *   keys_out stays [T][num_experts]: the keys of the global experts, unchanged.
 *   The expert stacks of the layer hold the L local routed experts followed by the S shared ones (L + S experts: what the MoE launches,
 *   petit_moe_align and petit_moe_combine are given as num_experts, with topk + S as topk).
 * petit_moe_route_align_ex: petit_moe_route_ex followed by petit_moe_align with num_experts = L + S on the T * (topk + S) entries, same
 *   outputs bit for bit (expert_offsets int32 [L + S + 1]).  ONE launch when T * (topk + S) <= 1024; above: the route launch, then the
 *   align's three.  workspace: petit_moe_route_align_ex_workspace_bytes() = petit_moe_align_workspace_bytes(T, topk + S, L + S).
 * Expert parallelism with shared experts.  A REPLICATED shared expert must be added once: give one rank S > 0 and the others S = 0, or
 *   give every rank shared_weight = 1 / ranks.  A shared expert SHARDED along its intermediate dimension takes weight 1 on every rank: down
 *   sums over that dimension, so the ranks' partial outputs add up.  A shared expert k times wider than the routed ones is k shared
 *   experts of the routed width (S = k, column blocks of gate / up and the matching row blocks of down): the gated activation is per
 *   column and down sums over columns.
 * Errors, all before any launch: everything petit_moe_route refuses, and PETIT_ERROR_PROBLEM_SHAPE for topk + S > PETIT_MOE_MAX_TOPK,
 * L + S > PETIT_MOE_MAX_EXPERTS, L > num_experts, L != num_experts without an expert_map, num_tokens * (topk + S) >= 2^31,
 * shared_gate_logits with S == 0.
 */
typedef struct petit_route_slots {      /* null or zero-initialised = petit_moe_route exactly */
    const int32_t *expert_map;          /* [num_experts] or null: global expert -> local expert */
    unsigned num_local_experts;         /* 0 = num_experts; must be num_experts (or 0) when expert_map is null */
    unsigned num_shared;                /* S >= 0 */
    float shared_weight;                /* 0 is read as 1 */
    const void *shared_gate_logits;     /* [num_tokens][S], logits_dtype, or null */
} petit_route_slots;
int petit_moe_route_ex(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                       const petit_route_desc *desc, const petit_route_slots *slots, int32_t *topk_ids, float *topk_weights, float *keys_out,
                       void *stream);
uint64_t petit_moe_route_align_ex_workspace_bytes(unsigned num_tokens, unsigned topk, unsigned num_experts, const petit_route_slots *slots);
int petit_moe_route_align_ex(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                             const petit_route_desc *desc, const petit_route_slots *slots, int32_t *topk_ids, float *topk_weights,
                             float *keys_out, int32_t *expert_offsets, int32_t *sorted_pos, int32_t *token_index, void *workspace, void *stream);

/*
 * The router's GEMM (no counterpart in the reference): router logits from the hidden state, logits [T][E] = hidden [T][K] . weight[E][K]^T
 * (+ router_bias), and the routing above started from the hidden state in two launches.  hidden [T][K] and weight [E][K] are contiguous
 * 16-bit tensors of one type (a_type PETIT_DTYPE_BF16 / _FP16; weight in the checkpoint's layout, no repack), both 16-byte aligned;
 * router_bias is float32 [E] or null; the logits are float32.  Any E in 1..PETIT_MOE_MAX_EXPERTS.  No host sync, graph-capturable.
 *
 * Definition, honoured bit for bit whatever T is:
 *     logit[t][e] = ( ... ((p_0 + p_1) + p_2) ... + p_{S-1} ) + router_bias[e]
 *   fp32 additions in this order, no contraction; without a bias the last add is not made.  p_s is the accumulation of slice s of K,
 *   k in [s L, min(K, (s + 1) L)), by one chain of v_mfma_f32_16x16x32_{bf16,f16} from a zero accumulator, k ascending in steps of 32.
 *   S and L (a multiple of 32) are functions of (E, K, a_type) alone -- petit_moe_router_geometry -- never of T or of a row's position in the
 *   batch: a token's logits, and with the tie rule above its experts, are a pure function of its hidden state.
 *   Accuracy: products of two 16-bit values are exact in fp32, so |logit - exact| <= 2 u (K + S + 1) (sum_k |a_k w_k| + |bias|), u = 2^-24.
 * Two forms produce those bits, chosen by T alone.  Small T (the split form): S x n-blocks x m-tiles workgroups store their partial tiles
 *   to S slabs [T][E] of the workspace with plain stores -- no tickets, no fences, no atomics -- and the NEXT launch adds the slabs.  Large T
 *   (the whole form): a workgroup walks all S slices, adding each slice's accumulation to a running total, and stores one slab.
 *   petit_moe_router_slabs is the slab count of the form T gets: S or 1.
 * Workspace: petit_moe_router_workspace_bytes = slabs * T * E * 4 rounded up to a multiple of 256 (0 for a shape the calls refuse);
 *   petit_moe_route_hidden_workspace_bytes = that, plus T * E * 4 (rounded up likewise) when E > 512, plus
 *   petit_moe_route_align_ex_workspace_bytes(T, topk, E, slots).
 *
 * petit_moe_router_logits writes the logits.  Launches: 1 when there is no bias and one slab (the GEMM writes straight into logits), else 2
 *   (the GEMM, then a finishing launch that makes the definition's additions).
 * petit_moe_route_hidden is petit_moe_route_align_ex (expert_offsets given) or petit_moe_route_ex (expert_offsets null: route only; sorted_pos
 *   and token_index are then not read) on those logits as float32, same outputs bit for bit -- keys_out with the softmax scoring IS the
 *   logit of the definition -- without the logits ever being stored: the route kernels add the slabs themselves.  A shared_gate_logits of the
 *   slot list is float32 here.  Launches: with the align and T * (topk + S_shared) <= 1024, 2 (the GEMM, then route + align in one launch on
 *   the slabs); larger T or route only: the GEMM and the route launch, plus the align's three when there is an align.  E > 512: one more, the
 *   finishing launch in front of the route (the 16-keys-per-lane route kernel has no register left to add slabs), unless one slab without a
 *   bias already is the logits.
 * Errors, all before any launch: PETIT_ERROR_PROBLEM_SHAPE for null required pointers or a hidden / weight that is not 16-byte aligned,
 *   K % 32 != 0 or K outside 32..16384, E outside 1..PETIT_MOE_MAX_EXPERTS, T >= 2^20, a null workspace when the byte query is not zero, and
 *   everything petit_moe_route_align_ex refuses; PETIT_ERROR_BAD_ARGUMENT for an a_type that is not FP16 or BF16.  T == 0 is PETIT_OK (with
 *   an align: the all-zero expert_offsets).
 * Not here: fp32 router weights, a strided hidden, a one-launch form (a last-arriver combine costs what the launch boundary does).
 */
void petit_moe_router_geometry(unsigned num_experts, unsigned k, int a_type, unsigned *slices, unsigned *slice_k); /* S, L */
unsigned petit_moe_router_slabs(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type);
uint64_t petit_moe_router_workspace_bytes(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type);
int petit_moe_router_logits(float *logits, const void *hidden, const void *weight, const float *router_bias, int a_type, unsigned num_tokens,
                            unsigned num_experts, unsigned k, void *workspace, void *stream);
uint64_t petit_moe_route_hidden_workspace_bytes(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type, unsigned topk,
                                                const petit_route_slots *slots);
int petit_moe_route_hidden(const void *hidden, const void *weight, const float *router_bias, int a_type, unsigned num_tokens, unsigned num_experts,
                           unsigned k, unsigned topk, const petit_route_desc *desc, const petit_route_slots *slots, int32_t *topk_ids,
                           float *topk_weights, float *keys_out, int32_t *expert_offsets /* null: route only */, int32_t *sorted_pos,
                           int32_t *token_index, void *workspace, void *stream);

/*
 * Batch-invariant GEMM (no counterpart in the reference): an opt-in dense FP4 GEMM whose every output element is a pure function of its
 * activation row, the weights, the scales and the bias -- not of m, not of the row's position in the batch, not of the launch form.  The
 * default calls above are pinned bit for bit within one call only: across calls the pick (MFMA shape, where the group scale is applied, how K
 * is split, bulk + tail) moves with m, so a token's bits differ alone and inside a batch.  This entry pays speed for the opposite
 * (profiles/gemm_invariant.md has the price).  Arguments as the _ex calls without solution_id, plus `workspace`; a, b, scales, c as there
 * (hints->a_type BF16 or FP16, c_type equal to it, hints->b_type the entry's format; the packed layout the other GEMMs read); global_scale
 * may be NULL.  No host sync, no allocation, graph-capturable.  Nothing here goes through the picks, the arch tables or the tuner.
 *
 * Definition, honoured bit for bit whatever m is:
 *     y[m][n] = ( ... ((p_0 + p_1) + p_2) ... + p_{S-1} ) * (*global_scale) + bias[n]
 *     c[m][n] = round16(y[m][n])                                  (round to nearest even, the one rounding of the exact-class contract)
 *   fp32 additions and one fp32 multiply, each rounded, in this order, no contraction; without a bias the last add is not made, without a
 *   global scale the multiply is not made.  p_s is the accumulation of slice s of K, k in [s L, min(K, (s + 1) L)), by ONE chain of
 *   v_mfma_f32_16x16x32_{bf16,f16} from a zero accumulator: the k-tiles of 128 ascending, inside a tile the four steps of the packed layout in
 *   their own order (step j covers k = 128 kt + 32 g + 8 j + i, g < 4, i < 8; petit-kernel_amd/csrc/layout.h).  The weight operand is the
 *   exactly dequantised value fp4 x group scale in the activation type (what petit_dequant_packed_weights returns with global_scale 1, with
 *   ONE exception: e8m0 scale byte 0 is 2^-127 here, the hardware convert's reading that every exact-class kernel has, where
 *   petit_dequant_packed_weights restates the reference's 0.0; byte 255 is no finite scale in either); the
 *   group scale is applied before the MFMA in every form.
 *   S and L (a multiple of 256: the packed scale layout exists for k % 256 == 0) are functions of (n, k, a_type, b_type) alone --
 *   petit_gemm_invariant_geometry; S * L >= k > (S - 1) * L, S <= 16.
 *   Accuracy: products of an activation and a dequantised weight are exact in fp32, so with u = 2^-24
 *     |y - exact| <= 2 u (K + S + 2) (|gs| sum_k |a_k w_k| + |bias|)      (K accumulation steps, S - 1 slab adds, one multiply, one add).
 *   This y, and the bound, are the PLAIN call's.  A gated call's y (next paragraph) is the fused multiply-add of the same fold: one rounding
 *   fewer, so the same bound holds for it, but with both a global scale and a bias it is not the same fp32 number as the plain call's y.
 *   Gated epilogues (epilogue->activation = PETIT_ACTIVATION_SILU_MUL / _SWIGLU_OAI; c is [m][n/2], n % 32 == 0, as in the _ex calls) are
 *   element-wise on y through the epilogue function every gated kernel of the library calls (silu_mul4, device_common.hpp), which forms
 *   y = fma(fold, gs, bias) -- ONE rounding where the plain call has two; without a bias or without a global scale the two agree.
 * Two forms produce those bits, chosen by m alone for a given shape.  Small m (the split form): S x n-blocks x m-tiles workgroups store their
 *   partial fp32 tiles to S slabs [m][n] of the workspace with plain vector stores -- no tickets, no fences, no atomics -- and a second launch
 *   adds the slabs in ascending order and applies scale, bias and activation.  Large m (the whole form): a workgroup walks all S slices,
 *   accumulates each from zero and adds it to a running total, applies the epilogue itself; one launch, no workspace (the activation tile of a workgroup goes through LDS).
 *   The switch is a constant of the library (m <= 32: split), not a setting.
 *   petit_gemm_invariant_slabs is the slab count of the form m gets: S or 1.
 * Workspace: petit_gemm_invariant_workspace_bytes = slabs * m * n * 4 rounded up to a multiple of 256; 0 for the whole form and for a shape
 *   or type pair the calls refuse.  Caller-owned device memory, 256-byte aligned, untouched until the call's work on `stream` has finished.
 * Errors, all before any launch: PETIT_ERROR_BAD_ARGUMENT for null hints, an a_type that is not BF16 / FP16, a c_type that differs, a b_type
 *   that is not the entry's format, an activation value that does not exist, a non-zero `reserved`; PETIT_ERROR_PROBLEM_SHAPE for n % 16 != 0
 *   (MXFP4: n % 32 != 0, as in the routed-expert launches: its processed scale tensor comes in rows of 32), k % 256 != 0, n or k zero, m >= 2^20, a gated activation with n % 32 != 0, null required pointers (c, a, b, scales), c / a / b / scales
 *   not 16-byte aligned, a bias not 8-byte aligned, a null or misaligned workspace when the byte query is not zero;
 *   PETIT_ERROR_KERNEL_SHAPE for fp16 activations with MXFP4 weights (below).  m == 0 returns PETIT_OK.
 * petit_gemm_fp4_invariant_host is the CPU twin for HOST pointers (activation none; bias may be NULL): it evaluates the definition with a
 *   sequential fp32 sum per slice in place of the MFMA chain -- the same bits whenever the partial sums are exact, a few ulp of y apart
 *   otherwise.  It reads e8m0 byte 0 as the kernels do (2^-127, an fp32 subnormal: its products with a code are exact).  It documents the
 *   format and serves the tests that run without a GPU; it is not a fallback.
 * Not here: grouped launches (the routed-expert launch: "Batch-invariant MoE launch" below); the native class in this entry (it has entries of its own: "Batch-invariant GEMM on the native class" and "Batch-invariant MoE launch on the native class" below); fp16 x MXFP4 (out-of-range scale bytes need the hi / lo fallback body,
 *   a second chain and a definition of its own); a one-launch split form (a last-arriver combine was probed and closed);
 *   any change to what PETIT_SOLUTION_AUTO runs.
 */
void petit_gemm_invariant_geometry(unsigned n, unsigned k, int a_type, int b_type, unsigned *slices, unsigned *slice_k); /* S, L */
unsigned petit_gemm_invariant_slabs(unsigned m, unsigned n, unsigned k, int a_type, int b_type);
uint64_t petit_gemm_invariant_workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int b_type);
int petit_gemm_fp4_fp16_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                  unsigned k, const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream);
int petit_gemm_mxfp4_fp16_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                    unsigned k, const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream);
int petit_gemm_fp4_invariant_host(void *c, const void *a, const void *b, const void *scales, const float *global_scale, const void *bias,
                                  unsigned m, unsigned n, unsigned k, int a_type, int b_type);

/*
 * Batch-invariant MoE launch (no counterpart in the reference): the routed-expert launch of the batch-invariant GEMM above.  Arguments as
 * petit_gemm_fp4_fp16_moe_ex without solution_id, plus `workspace`: grouped row r belongs to expert e under the clamp rule of the routed-expert
 * launch (every offset clamped into [its predecessor, m], a running maximum; rows of no expert are left untouched), reads row a_row_index[r]
 * of a [a_rows][k] and writes row c_row_index[r] of c [c_rows][n_out] (a NULL index is the identity).
 * Definition: the written row equals, bit for bit, row 0 of
 *     petit_gemm_{fp4,mxfp4}_fp16_invariant(m = 1, a = that A row, b / scales = expert e's packed tensors, global_scale = &global_scales[e],
 *                                           bias = bias + e * n, the same activation)
 *   so S and L are petit_gemm_invariant_geometry(n, k, a_type, b_type) -- never functions of m, num_experts or the routing --, the arithmetic
 *   is the dense entry's (one MFMA chain per slice from zero, slices added in ascending order, * gs, + bias, no contraction, one rounding),
 *   and the gated epilogues pair gate tile t with up tile t + ntiles / 2 of the same expert.  With a token's slot rows combined by
 *   petit_moe_combine (slot order, fp32, one rounding), a token's layer output is a pure function of its hidden row and the weights.
 *   An A index outside [0, a_rows) reads a zero row; a C index outside [0, c_rows) stores nothing; malformed offsets can only leave rows
 *   unwritten.  An expert without rows is never read.  The host never reads the offsets: no sync, no allocation, no atomics, tickets or
 *   fences; graph-capturable, and a replay follows new offsets.
 * Two forms produce those bits; petit_gemm_moe_invariant_form(m, num_experts) names the one a call gets (1: split, 0: whole), a function of
 *   these two host-known arguments alone: split iff ceil(m / min(E, m)) <= 8 and m <= 8 (constants of the library, not settings; measured, profiles/moe_invariant.md:
 *   the split form pays for a decode step's few rows only).
 *   split: ceil(m / 16) + min(E, m) slots x S x n-blocks workgroups store fp32 tiles to S slabs [m][n], indexed by grouped row, with plain
 *     vector stores; a second launch over the same slot map adds the slabs in ascending order, applies gs[e], bias[e] and the activation and
 *     scatters C.  Nothing in the workspace needs clearing.
 *   whole: ceil(m / 64) + min(E, m) slots x n-blocks workgroups stage the gathered activation tile through LDS, walk all S slices and
 *     apply the epilogue themselves; no workspace.
 * Workspace: petit_gemm_moe_invariant_workspace_bytes = S * m * n * 4 rounded up to a multiple of 256 in the split form; 0 in the whole form
 *   and for a call that would be refused.  Caller-owned device memory, 256-byte aligned.
 * Errors, all before any launch: the dense entry's codes (above), and PETIT_ERROR_PROBLEM_SHAPE for num_experts outside 1..1024, a NULL index
 *   with fewer than m rows behind it, a_rows * k * 2 > 2^31 (one buffer descriptor bounds every A load), a launch of 2^31 workgroups or
 *   more, a NULL global_scales or expert_offsets, an index or offset pointer that is not 4-byte aligned.  m == 0 returns PETIT_OK.
 * petit_gemm_fp4_moe_invariant_host is the CPU twin on HOST pointers (offsets and indices included; activation none; bias [E][n] or NULL):
 *   petit_gemm_fp4_invariant_host per expert under the clamp rule.
 * Not here: the native class (it has entries of its own below: "Batch-invariant GEMM on the native class" and its routed-expert launch, "Batch-invariant MoE launch on the native class", which also takes fp16 x MXFP4); fp16 x MXFP4; the grouped q / k / v launch; a one-launch split form; a persistent-slot form for dead slots.
 */
int petit_gemm_moe_invariant_form(unsigned m, unsigned num_experts);
uint64_t petit_gemm_moe_invariant_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int b_type);
int petit_gemm_fp4_fp16_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                      const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                      const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                      const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream);
int petit_gemm_mxfp4_fp16_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                        const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                        const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                        const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream);
int petit_gemm_fp4_moe_invariant_host(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const void *bias,
                                      const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                      const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows, int a_type,
                                      int b_type);

/*
 * Batch-invariant GEMM on the native class (no counterpart in the reference): the dense batch-invariant entry for MXFP4 weights on the
 * block-scaled MFMA -- the accuracy class of petit_gemm_mxfp4_native (activations quantised to MXFP8 / MXFP6 / MXFP4), with the guarantee of
 * "Batch-invariant GEMM" above: every output element is a pure function of its activation row, the weights, the scales and the bias -- not of m,
 * not of the row's position in the batch, not of the launch form.  The native default is not: its pick (kernel, wave-level K split, bulk rows in
 * the class plus a tail in the exact class) moves with m.  Opt-in by calling it; nothing here goes through the picks, the arch tables or the tuner.
 *   a               a_is_quantized == 0: the 16-bit [m][k] matrix (hints->a_type BF16 or FP16); the call first runs the library's own quantiser
 *                   (petit_quantize_activations) into the workspace.  Otherwise "petit-qact/1" bytes of act_format for (m, k), as
 *                   petit_quantize_activations / petit_rmsnorm_quantize write them.  Both paths give the same bits: the quantised bytes of a row
 *                   are a function of that row alone (per row and per 32-k block; only their ADDRESS in the k-tile-major image depends on m).
 *   act_format      8 (MXFP8), 6 (MXFP6 e2m3) or 4 (MXFP4).
 *   b, scales       the packed MXFP4 tensors the other GEMMs read; hints->b_type an MXFP4 type, hints->c_type == hints->a_type (FP16 IS accepted:
 *                   the instruction takes any E8M0 byte, so the exact entry's reason for refusing fp16 x MXFP4 does not apply).
 *   global_scale, epilogue (bias, activation), c as in the exact invariant entry; gated calls (c is [m][n/2]) need n % 64 == 0.
 * Definition, honoured bit for bit whatever m is:
 *     y[m][n] = ( ... ((p_0 + p_1) + p_2) ... + p_{S-1} ) * (*global_scale) + bias[n]
 *     c[m][n] = round16(y[m][n])
 *   S and L are petit_gemm_invariant_geometry(n, k, a_type, PETIT_DTYPE_MXFP4): never functions of m or of the activation format.  p_s is the
 *   accumulation of slice s of K by ONE chain of v_mfma_scale_f32_32x32x64_f8f6f4 from a zero accumulator: the k-tiles of 128 ascending, two
 *   instructions per k-tile -- k 0..63 of the tile (P1), then k 64..127 (P2).  The weight operand is the pair of neighbouring n-tiles (32 rows)
 *   as stored -- raw E2M1 nibbles, 32 consecutive k per lane -- with the E8M0 byte of the lane's block as its scale; the activation operand is the
 *   row's "petit-qact/1" bytes of that k-tile and their four E8M0 bytes.  (The 16x16x128 shape aligns and truncates a different number of block
 *   sums per instruction and does not give the same bits: both forms use 32x32x64.)  Fold and epilogue are the exact invariant entry's: fp32
 *   additions in ascending order, no contraction; the plain call then multiplies and adds with a rounding each, the gated call
 *   (PETIT_ACTIVATION_SILU_MUL / _SWIGLU_OAI) forms fma(fold, gs, bias) -- one rounding -- in the epilogue function every gated kernel calls.
 *   Pinned for weight scale bytes 1..254; bytes 0 and 255 are whatever the instruction does, as for the rest of the class.
 *   Accuracy, given the quantised activations: the bound of "Native-FP4 kernels" above.  It holds for any K split, and its 16 * T term is sixteen
 *   fp32 additions of at most 2^-24 * T each: the S - 1 <= 15 slab additions here are covered by it as they stand, and the global-scale multiply
 *   is the sixteenth; a bias adds one more rounding, 2^-24 * (gs * T + |bias|).  Nothing is fitted.
 * Two forms produce those bits, chosen by m alone.  m <= 64 (the split form): pairs of n-tiles x S x m-tiles of 32 waves store their fp32 tiles to
 *   S slabs [m][n] with plain vector stores -- no atomics, tickets or fences --, and a second launch adds the slabs in ascending order and applies
 *   scale, bias and activation.  Above (the whole form): a workgroup stages its activation tile of every k-tile through LDS, a wave walks all S
 *   slices, accumulates each from zero and adds it to a running total, and applies the epilogue itself; no slab workspace.  The switch is a
 *   constant of the library, not a setting (profiles/native_invariant.md).  petit_gemm_native_invariant_slabs: S or 1, the form m gets.
 * Workspace: petit_gemm_native_invariant_workspace_bytes = the quantised bytes (petit_quantized_activation_bytes; 16-bit input only) + the slabs
 *   (slabs * m * n * 4; split form only), each part rounded up to a multiple of 256, in this order; 0 for a call that would be refused and for
 *   m == 0.  Caller-owned device memory, 256-byte aligned.  No host sync, no allocation, graph-capturable.
 * Errors, all before any launch: PETIT_ERROR_BAD_ARGUMENT for null hints, an a_type that is not BF16 / FP16, a c_type that differs, a b_type that
 *   is not MXFP4, an act_format outside {8, 6, 4}, an activation value that does not exist, a non-zero `reserved`; PETIT_ERROR_PROBLEM_SHAPE for
 *   n % 32 != 0, k % 256 != 0, n or k zero, m >= 2^20, a gated activation with n % 64 != 0, null required pointers, c / a / b / scales not
 *   16-byte aligned, a bias not 8-byte aligned, a null or misaligned workspace when the byte query is not zero; PETIT_ERROR_KERNEL_SHAPE for a
 *   16-bit input of more than 65535 rows (the quantiser's limit: pass quantised bytes).  m == 0 returns PETIT_OK.
 * petit_quantize_activations_host is petit_quantize_activations on HOST pointers, bit for bit (the quantiser of petit_rmsnorm_quantize_host).
 * petit_gemm_native_invariant_host is the CPU twin on HOST "petit-qact/1" bytes (activation none; global_scale and bias may be NULL): per slice a
 *   sequential fp32 sum of a_q * w, k ascending, then the stated fold and epilogue -- the device's bits whenever every partial sum is exact.  The
 *   activation bytes are decoded with the formats' own tables, E8M0 as the exact twin reads it.  It documents the format and serves the tests
 *   that run without a GPU; it is not a fallback.
 * Not here: NVFP4 images on this entry (they have entries of their own: "Batch-invariant native-class GEMM and MoE launch on NVFP4 images"
 *   below); grouped launches (the routed-expert launch: "Batch-invariant MoE launch on the native class" below, which
 *   fp4_moe_native(..., invariant=True) runs); a quantising (out_format) epilogue; any change to what the sentinels run.
 */
unsigned petit_gemm_native_invariant_slabs(unsigned m, unsigned n, unsigned k, int a_type);
uint64_t petit_gemm_native_invariant_workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int act_format, int a_is_quantized);
int petit_gemm_mxfp4_native_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                      unsigned k, const petit_solution_hints *hints, int act_format /* 8 | 6 | 4 */, int a_is_quantized,
                                      const petit_epilogue *epilogue, void *workspace, void *stream);
int petit_quantize_activations_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format);
int petit_gemm_native_invariant_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scale, const void *bias,
                                     unsigned m, unsigned n, unsigned k, int a_type, int act_format);

/*
 * Batch-invariant MoE launch on the native class (no counterpart in the reference): the routed-expert launch of "Batch-invariant GEMM on the
 * native class" above -- MXFP4 experts on the block-scaled MFMA, activations quantised to MXFP8 / MXFP6 / MXFP4.  Arguments as
 * petit_gemm_mxfp4_fp16_moe_invariant plus act_format and a_is_quantized: grouped row r belongs to expert e under the clamp rule of the
 * routed-expert launch (every offset clamped into [its predecessor, m], a running maximum; rows of no expert are left untouched) and is written
 * to row c_row_index[r] of c [c_rows][n_out] (a NULL index is the identity).
 *   a               a_is_quantized == 0: the 16-bit [a_rows][k] matrix (hints->a_type BF16 or FP16); grouped row r is its row a_row_index[r] (NULL:
 *                   r).  The call first runs the gathering quantiser (petit_quantize_activations_rows' launch) into the workspace; an index
 *                   outside [0, a_rows) quantises a zero row.  Otherwise "petit-qact/1" bytes of (m, k, act_format) for the m GROUPED rows, as
 *                   petit_quantize_activations_rows writes them; a_row_index must be NULL and a_rows is not read.  Both give the same bits.
 *   b, scales       the experts' packed MXFP4 tensors back to back, as the other MoE launches read them; hints->b_type an MXFP4 type,
 *                   hints->c_type == hints->a_type; FP16 and BF16 are both accepted.
 *   global_scales [E], epilogue (bias [E][n], activation), c as in the exact MoE invariant entry; gated calls (c is [c_rows][n/2]) need n % 64 == 0.
 * Definition: the row written for grouped row r of expert e equals, bit for bit, row 0 of
 *     petit_gemm_mxfp4_native_invariant(m = 1, a = that row, b / scales = expert e's packed tensors, global_scale = &global_scales[e],
 *                                       bias = bias + e * n, the same activation, the same act_format)
 *   so S and L are petit_gemm_invariant_geometry(n, k, a_type, PETIT_DTYPE_MXFP4) -- never functions of m, num_experts or the routing --, the
 *   arithmetic is the dense native entry's (one chain of v_mfma_scale_f32_32x32x64_f8f6f4 per slice from zero, k-tiles of 128 ascending, P1 then
 *   P2, slices added ascending in fp32, no contraction, the same epilogue functions), and the gated epilogues pair gate pair t with up pair
 *   t + ntiles / 4 of the same expert.  With a token's slot rows combined by petit_moe_combine (slot order, fp32, one rounding), a token's
 *   layer output is a pure function of its hidden row and the weights.  A C index outside [0, c_rows) stores nothing; malformed offsets can only
 *   leave rows unwritten.  An expert without rows is never read.  The host never reads the offsets: no sync, no allocation, no atomics, tickets
 *   or fences; graph-capturable, and a replay follows new offsets.
 * Two forms produce those bits; petit_gemm_native_moe_invariant_form(m, num_experts) names the one a call gets (1: split, 0: whole), a function
 *   of these two host-known arguments alone: split iff ceil(m / min(E, m)) <= 8 and m <= 8 (constants of the library, not settings;
 *   profiles/native_moe_invariant.md).  The quantised activations are the k-tile-major image of the m grouped rows, so a tile's rows are one
 *   contiguous run; its descriptor ends with the tile's last valid row of its expert, and rows of the next expert or past m read zeros.
 *   split: ceil(m / 32) + min(E, m) slots x S x blocks of 4 pairs of n-tiles; a wave stores its 32 x 32 fp32 tile of one slice to slab s of
 *     [S][m][n], indexed by grouped row, with plain vector stores; the second launch is the exact MoE entry's fold over its own 16-row slot map
 *     of the same offsets (gs[e], bias[e], the activation, the scatter into C).  Nothing in the workspace needs clearing.
 *   whole: ceil(m / 64) + min(E, m) slots x blocks of 4 x 2 pairs of n-tiles; the workgroup stages its expert's 64-row activation tile of every
 *     k-tile through LDS, a wave walks all S slices with one join per slice, applies the epilogue itself and scatters C; no slab workspace.
 * Workspace: petit_gemm_native_moe_invariant_workspace_bytes = the quantised bytes (petit_quantized_activation_bytes(m, k, act_format); 16-bit
 *   input only) + the slabs (S * m * n * 4; split form only), each part rounded up to a multiple of 256, in this order; 0 for a call that would
 *   be refused and for m == 0.  Caller-owned device memory, 256-byte aligned.
 * Errors, all before any launch: the dense native-invariant entry's codes (above) without its 65535-row limit on 16-bit input -- the gathering
 *   quantiser takes any row count; m < 2^20 stays --; the MoE invariant entry's codes (PETIT_ERROR_PROBLEM_SHAPE for num_experts outside
 *   1..1024, a NULL global_scales or expert_offsets, an index or offset pointer that is not 4-byte aligned, a NULL index with fewer than m rows
 *   behind it, a launch of 2^31 workgroups or more); PETIT_ERROR_BAD_ARGUMENT for a_is_quantized with an a_row_index;
 *   PETIT_ERROR_PROBLEM_SHAPE when the quantised rows reach 2^32 bytes.  m == 0 returns PETIT_OK.
 * petit_gemm_native_moe_invariant_host is the CPU twin on HOST pointers: the grouped "petit-qact/1" bytes of (m, k, act_format), offsets and a C
 *   index (activation none; bias [E][n] or NULL).  Per expert under the clamp rule it computes each row as petit_gemm_native_invariant_host
 *   computes it, decoded from the m-row image (the image's addresses depend on m, the values do not).
 * Not here: NVFP4 images on this entry (petit_gemm_nvfp4_native_moe_invariant below takes them); a quantising (out_format) epilogue; a
 *   pipelined whole form; a one-launch split form.
 */
int petit_gemm_native_moe_invariant_form(unsigned m, unsigned num_experts); /* 1: split, 0: whole */
uint64_t petit_gemm_native_moe_invariant_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int act_format,
                                                         int a_is_quantized);
int petit_gemm_mxfp4_native_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                          const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                          const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                          const petit_solution_hints *hints, int act_format /* 8 | 6 | 4 */, int a_is_quantized,
                                          const petit_epilogue *epilogue, void *workspace, void *stream);
int petit_gemm_native_moe_invariant_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scales, const void *bias,
                                         const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                         const int32_t *c_row_index, unsigned c_rows, int a_type, int act_format);

/*
 * Batch-invariant native-class GEMM and MoE launch on NVFP4 images (no counterpart in the reference): the two entries above for NVFP4 weights,
 * read from their MFMA-native image ("petit-cdna4-nv6/1": petit_nvfp4_native_image / _images above) -- the accuracy class of
 * petit_gemm_nvfp4_native on an image, with the guarantee of "Batch-invariant GEMM on the native class".  Arguments as
 * petit_gemm_mxfp4_native_invariant / petit_gemm_mxfp4_native_moe_invariant with `image` / `images` in the place of (b, scales):
 *   image           petit_nvfp4_native_image of the packed (n, k) tensors: petit_nvfp4_native_image_bytes(k, n) bytes of device memory, 256-byte
 *                   aligned.  hints->b_type PETIT_DTYPE_FP4_E2M1, hints->c_type == hints->a_type (BF16 or FP16).
 *   images          the MoE entry: E images back to back, expert e's at byte e * petit_nvfp4_native_image_bytes(k, n) with its scale region
 *                   after its own elements -- the layout petit_gemm_native_moe reads and petit_nvfp4_native_images writes.
 *   global_scale(s) NVFP4's real global scale (one float; the MoE entry: [E]); a, act_format, a_is_quantized, epilogue, c, the row indices and the
 *                   offsets as in the MXFP4 entries.
 * Definition: that of "Batch-invariant GEMM on the native class" with one substitution -- the weight operand is the image's bytes of the block
 *   of 32 weight rows: FP6 e2m3 elements, 32 consecutive k per lane, with the image's E8M0 byte of the lane's block as its scale.  S and L are
 *   petit_gemm_invariant_geometry(n, k, a_type, PETIT_DTYPE_FP4_E2M1); per slice ONE chain of v_mfma_scale_f32_32x32x64_f8f6f4 from a zero
 *   accumulator, k-tiles of 128 ascending, P1 then P2; slices added ascending in fp32 with no contraction; the plain epilogue rounds twice
 *   (multiply, add), the gated ones form fma(fold, gs, bias) once and pair gate block t with up block t + n / 64.  The MoE row of grouped row r
 *   of expert e equals, bit for bit, row 0 of petit_gemm_nvfp4_native_invariant(m = 1, a = that row, image = expert e's image,
 *   global_scale = &global_scales[e], bias = bias + e * n, the same activation and act_format).
 *   Accuracy: given the quantised activations and the image's weights (petit_nvfp4_native_image_dequant_host), the bound of "Native-FP4 kernels"
 *   exactly as the MXFP4 entry states it; against the true NVFP4 weights add the re-encoding bound stated with petit_nvfp4_native_image above.
 *   Nothing is fitted.
 * Forms, queries, workspace: the MXFP4 native entries' as they stand -- the form constants are shared (dense: split iff m <= 64; MoE: split iff
 *   ceil(m / min(E, m)) <= 8 and m <= 8), so petit_gemm_native_invariant_slabs, petit_gemm_native_moe_invariant_form and the two
 *   ..._workspace_bytes queries answer for these entries too (quantised bytes, then slabs, each rounded up to 256).  A wave's unit of columns is
 *   one block of 32 weight rows, where the MXFP4 kernels merge a pair of n-tiles; everything after the instruction is shared with them.
 * Errors, all before any launch and in this order: PETIT_ERROR_BAD_ARGUMENT for null hints, a c_type that differs from a_type, a b_type that is
 *   not PETIT_DTYPE_FP4_E2M1, a non-zero `reserved`, an a_type that is not BF16 / FP16, an act_format outside {8, 6, 4}, an activation value
 *   that does not exist; PETIT_ERROR_PROBLEM_SHAPE for n % 32 != 0 (the image's zero-padded last block never arises), k % 256 != 0, n or k
 *   zero, m >= 2^20, a gated activation with n % 64 != 0, an image of 2^32 element bytes or more (n * k * 3 / 4); PETIT_ERROR_PROBLEM_SHAPE for
 *   an image address that is no multiple of 256; PETIT_ERROR_KERNEL_SHAPE for a dense 16-bit input of more than 65535 rows; then the MXFP4
 *   entries' routing, pointer and workspace codes.  m == 0 returns PETIT_OK.  The MXFP4 entries keep refusing an NVFP4 b_type.
 * petit_gemm_nvfp4_native_invariant_host / petit_gemm_nvfp4_native_moe_invariant_host are the CPU twins on HOST "petit-qact/1" bytes and HOST
 *   images (activation none): every product is formed exactly from (decoded activation element x its E8M0) x (e2m3 element x 2^(byte - 127))
 *   and rounded once to fp32; per slice a sequential fp32 sum, k ascending, then the stated fold and epilogue -- the device's bits whenever every
 *   partial sum is exact.  The image is decoded at the offsets petit_nvfp4_native_image_dequant_host uses.  Not fallbacks.
 * Measured (profiles/nvfp4_native_invariant.md, bf16, the four Llama-3-70B linears, quantiser launch included): against
 *   petit_gemm_fp4_fp16_invariant, the only invariant NVFP4 path before, 1.2-1.7x faster in every cell at m = 512 and 4096, 1.5-4.0x faster
 *   at m = 64 except on 57344 columns (1.6-2.1x slower), and 11-39 % slower at m = 1 on the narrower layers; 1.8-4.2x the time of
 *   petit_gemm_nvfp4_native on the same image from m = 512 on; 1.0-1.4x the time of petit_gemm_mxfp4_native_invariant with MXFP8
 *   activations (up to 2.0x with MXFP6 / MXFP4: the FP6 weight operand).  Both form switches were measured on images and kept.
 * Not here: the transient (image-per-call) form; a quantising epilogue; a pipelined whole form; a one-launch split form; any change to the
 *   sentinels and default picks; fp4_moe_native(kind="nvfp4", invariant=True), which keeps raising (compose the layer from these launches:
 *   examples/nvfp4_native_invariant.py).
 */
int petit_gemm_nvfp4_native_invariant(void *c, const void *a, const void *image, const float *global_scale, unsigned m, unsigned n, unsigned k,
                                      const petit_solution_hints *hints, int act_format /* 8 | 6 | 4 */, int a_is_quantized,
                                      const petit_epilogue *epilogue, void *workspace, void *stream);
int petit_gemm_nvfp4_native_moe_invariant(void *c, const void *a, const void *images, const float *global_scales, const int32_t *expert_offsets,
                                          unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index, unsigned a_rows,
                                          const int32_t *c_row_index, unsigned c_rows, const petit_solution_hints *hints,
                                          int act_format /* 8 | 6 | 4 */, int a_is_quantized, const petit_epilogue *epilogue, void *workspace,
                                          void *stream);
int petit_gemm_nvfp4_native_invariant_host(void *c, const void *qa, const void *image, const float *global_scale, const void *bias, unsigned m,
                                           unsigned n, unsigned k, int a_type, int act_format);
int petit_gemm_nvfp4_native_moe_invariant_host(void *c, const void *qa, const void *images, const float *global_scales, const void *bias,
                                               const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                               const int32_t *c_row_index, unsigned c_rows, int a_type, int act_format);

/*
 * Native-class MoE launch (no counterpart in the reference): the routed-expert launch on the block-scaled MFMA, the accuracy class of
 * petit_gemm_mxfp4_native (activations quantised to MXFP8 / MXFP6 / MXFP4; the per-element bound is the native block's above).  Opt-in
 * like every native call: solution_id is a PETIT_SOLUTION_AUTO_NATIVE_* sentinel or an explicit native id that has a MoE form (the 128 x 256
 * kernels per activation format and span size); PETIT_SOLUTION_AUTO and exact-class ids return PETIT_ERROR_KERNEL_SHAPE -- never another class.
 * A sentinel picks as petit_gemm_moe_resolve_solution does (rows per active expert), among the native kernels with a MoE form.
 *   b, scales       hints->b_type MXFP4: the stacked packed tensors, exactly what petit_gemm_fp4_fp16_moe reads.  NVFP4 (PETIT_DTYPE_FP4_E2M1):
 *                   b is E MFMA-native images back to back, expert e's = petit_nvfp4_native_image of its packed block, at byte
 *                   e * petit_nvfp4_native_image_bytes(k, n) (an image of the stacked [E n, k] tensor is NOT that: its scale region follows
 *                   all the elements); b 256-byte aligned; scales is ignored (NULL).
 *   a               native->a_format 0 (or native null): 16-bit rows, gathered through a_row_index as petit_gemm_fp4_fp16_moe_ex does (an index
 *                   outside [0, a_rows) quantises a zero row) and quantised into `workspace` first: two launches, workspace_bytes >=
 *                   petit_gemm_native_moe_workspace_bytes().  a_format 8 / 6 / 4: a holds the m GROUPED rows already quantised
 *                   (petit_quantize_activations_rows, or a producer's out_format), a_row_index must be null: one launch, no workspace.
 *   c               16-bit [c_rows][n] ([c_rows][n/2] with SiLU-mul), row c_row_index[r] (null: r) for grouped row r; an index outside
 *                   [0, c_rows) stores nothing.  native->out_format 8 / 6 / 4 (SiLU-mul or SwiGLU-OAI only, n % 512 == 0, c_row_index null): c receives
 *                   the m grouped rows of [m][n/2] quantised for the next launch (petit_quantized_activation_bytes(m, n / 2, format)).
 *   Row limit: every epilogue stores rows of its own expert only; rows past expert_offsets[E] are not computed.  Within an expert the
 *   result equals, bit for bit, petit_gemm_mxfp4_native / petit_gemm_nvfp4_native on that expert's rows with the same id.
 * Shapes and errors as petit_gemm_fp4_fp16_moe_ex and petit_gemm_mxfp4_native; also PETIT_ERROR_BAD_ARGUMENT for a_format with an
 * a_row_index, out_format with a c_row_index or without a gated activation, misaligned pointers; PETIT_ERROR_KERNEL_SHAPE for a workspace below the
 * query; PETIT_ERROR_PROBLEM_SHAPE when the quantised rows reach 2^32 bytes (32-bit offsets).  m == 0 returns PETIT_OK.  No host sync:
 * capturable.  The queries return 0 for a call that would be refused; the workspace query also 0 with a_format set.
 * petit_quantize_activations_rows: petit_quantize_activations of the gathered rows (layout row r from row a_row_index[r] of a [a_rows][k];
 * null: the identity, a_rows >= m), one launch; any m (no grid-row limit) below 2^32 bytes of output.
 *
 * Without resident images -- petit_gemm_native_moe_transient(c, a, b, scales, ...), NVFP4 experts only: b / scales are the stacked PACKED tensors,
 * exactly what petit_gemm_fp4_fp16_moe reads.  The call builds the images of the experts that have rows into its workspace
 * (petit_nvfp4_native_images on expert_offsets, one launch), then does what petit_gemm_native_moe does on them, all in stream order on `stream`.
 * Nothing is registered or cached: two layers' calls may share one workspace one after the other, and a captured call reads b, scales and
 * expert_offsets anew at every replay.  The experts then cost 4.5 bits per weight plus ONE workspace the size of the largest layer's images,
 * shared by all layers, where resident images add 6.25 bits per weight to every layer.
 *   workspace layout: [0, E * I) the images, I = petit_nvfp4_native_image_bytes(k, n) -- a multiple of 256 for every accepted shape (6400 bytes per
 *       32 rows x 256 k), so expert e's image is at e * I as petit_gemm_native_moe reads it; [E * I, E * I + S) exactly what
 *       petit_gemm_native_moe_workspace_bytes returns for the same call (0 with pre-quantised a).  The region of an expert without rows is not written.
 *       petit_gemm_native_moe_transient_workspace_bytes returns E * I + S in 64 bits (0: the call would be refused).
 *   refusals, all before the first launch (C and the workspace untouched, nothing enters a stream capture): PETIT_SOLUTION_AUTO and exact-class ids
 *       PETIT_ERROR_KERNEL_SHAPE; hints->b_type MXFP4 PETIT_ERROR_BAD_ARGUMENT (MXFP4 needs no image: petit_gemm_native_moe); scales NULL
 *       PETIT_ERROR_PROBLEM_SHAPE; b / scales not 16-byte aligned PETIT_ERROR_BAD_ARGUMENT; a workspace that is missing or below the query
 *       PETIT_ERROR_KERNEL_SHAPE, misaligned PETIT_ERROR_BAD_ARGUMENT; every shape limit of petit_gemm_native_moe and petit_nvfp4_native_image.
 *       m == 0 returns PETIT_OK and launches nothing.
 *   results: bit for bit petit_gemm_native_moe with the same id on petit_nvfp4_native_images of the same tensors -- every epilogue, pre-quantised
 *       a, out_format, the indexed A / C forms.
 */
uint64_t petit_gemm_native_moe_transient_workspace_bytes(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                                         uint64_t solution_id, const petit_epilogue *epilogue, const petit_native_args *native);
int petit_gemm_native_moe_transient(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                    const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                    const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                    const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue,
                                    const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream);
uint64_t petit_gemm_native_moe_workspace_bytes(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                               uint64_t solution_id, const petit_epilogue *epilogue, const petit_native_args *native);
uint64_t petit_gemm_native_moe_resolve_solution(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                                uint64_t solution_id, const petit_epilogue *epilogue, const petit_native_args *native);
int petit_gemm_native_moe(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const int32_t *expert_offsets,
                          unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index, unsigned a_rows,
                          const int32_t *c_row_index, unsigned c_rows, const petit_solution_hints *hints, uint64_t solution_id,
                          const petit_epilogue *epilogue, const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream);
int petit_quantize_activations_rows(void *qa, const void *a, const int32_t *a_row_index, unsigned a_rows, unsigned m, unsigned k, int a_type,
                                    int format, void *stream);

/*
 * Block-Hadamard rotation ("petit-had/1") in the native class's activation quantisers (no counterpart in the reference).  MXFP4 activations
 * cost the native class most of its accuracy; the standard cure (QuaRot, MR-GPTQ, QuTLASS) multiplies activations and weights along K by
 * the same +-1 Hadamard block, which leaves the product unchanged and spreads a block's outliers over all of its coefficients before the
 * 4-bit rounding.  The rotation runs INSIDE the quantiser launches: no extra launch and no [m][k] 16-bit round trip per GEMM input.
 *
 * Definition.  B (`block`) is 32 or 128; k % 256 == 0, so a row is a whole number of blocks.  For a row x of 16-bit elements widened exactly
 * to f32 and each block of B consecutive k, z[0 .. B-1] is the block; for s = 0 .. log2(B) - 1 IN THIS ORDER, d = 2^s, and every i with
 * (i & d) == 0:
 *         (z[i], z[i + d])  <-  (z[i] + z[i + d],  z[i] - z[i + d])
 * Each sum and each difference is ONE f32 operation, round to nearest even; nothing is fused.  This is z . H_B with the Sylvester Hadamard
 * matrix in natural order, unnormalised: H_B is symmetric and H_B . H_B = B . I.  The stage order is part of the contract (sums of 128
 * bf16 values round in f32: another order gives other bits).  Two consumers of z:
 *   1. rotation to 16 bit (load time, weights): out = round16(z * 2^log2_scale) -- one f32 multiply by a power of two (exact short of
 *      over- or underflow), ONE round to nearest even into the 16-bit type, subnormals included.   petit_hadamard_rows
 *   2. rotation into the quantiser (per call, activations): z takes the place of the widened row in petit_quantize_activations and nothing
 *      else changes -- the block maximum over each 32-k block of z (with B = 128 a rotation block still carries four scales), the same
 *      scale rule, converts, stores and layout; no intermediate 16-bit rounding.   petit_quantize_activations_rot and its kin
 * The identity a caller relies on:  (x . H_B) . (W . H_B . 2^-log2(B))^T = x . W^T.  Activations rotate with scale 1; weights rotate with
 * log2_scale = -log2(B), which is exact.  A checkpoint whose weights were rotated with the orthonormal H / sqrt(B) runs on the same
 * activation entries: the caller folds 1 / sqrt(B) into global_scale.  The GEMMs read "petit-qact/1" bytes and cannot tell that they were
 * rotated; a rotated row is still a pure function of its row, so the batch-invariant entries keep their property unchanged.
 * A block that contains a non-finite element gives unspecified elements and scales for its own 32-k blocks only.  A zero block stays zero
 * with scale byte 127; a gathered row whose index is out of range stays a zero row.
 *
 * block == 0 is the unrotated entry, bit for bit (the call is handed on); a block other than 0 / 32 / 128 is PETIT_ERROR_BAD_ARGUMENT.
 * format is 8 or 4; format == 6 with a rotation is PETIT_ERROR_KERNEL_SHAPE (the MXFP6 quantiser converts 32 elements straight from their
 * 16-bit patterns; an f32 form of it is out of scope).  Every other refusal is that of the unrotated entry.  petit_hadamard_rows refuses
 * k % 256 != 0 (PETIT_ERROR_PROBLEM_SHAPE), an a_type other than bf16 / fp16 (PETIT_ERROR_KERNEL_SHAPE), and a block other than 32 / 128,
 * |log2_scale| > 126, null pointers or pointers not aligned to 16 bytes (PETIT_ERROR_BAD_ARGUMENT); out may be in (a block is read
 * completely before it is written).  All refusals come before any launch; no allocation, no host sync, graph-capturable.  The _host
 * forms are the host twins (host pointers): bit-identical outputs, the same refusals.
 * In the fused norm steps 1 - 4 of "RMSNorm into quantised activations" are untouched: y is rounded to 16 bit and the rotation runs on
 * f32(y16), so qa is bit for bit petit_quantize_activations_rot on the y16 the same call can return; y16 and residual_out stay unrotated.
 * Out of scope: MXFP6 activations; the quantising gated epilogue (out_format of the gate_up kernels cannot rotate -- a rotated `down`
 * takes the 16-bit hand-over plus petit_quantize_activations_rot); petit_moe_combine_rmsnorm; random sign diagonals; every GEMM and MoE
 * kernel, which consume the bytes as they are.
 */
int petit_hadamard_rows(void *out, const void *in, unsigned rows, unsigned k, int a_type, unsigned block, int log2_scale, void *stream);
int petit_hadamard_rows_host(void *out, const void *in, unsigned rows, unsigned k, int a_type, unsigned block, int log2_scale);
int petit_quantize_activations_rot(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format, unsigned block, void *stream);
int petit_quantize_activations_rot_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format, unsigned block);
int petit_quantize_activations_rows_rot(void *qa, const void *a, const int32_t *a_row_index, unsigned a_rows, unsigned m, unsigned k, int a_type,
                                        int format, unsigned block, void *stream);
int petit_rmsnorm_quantize_rot(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                               float weight_offset, unsigned m, unsigned k, int a_type, int format, unsigned block, void *stream);
int petit_rmsnorm_quantize_rot_host(void *qa, void *y16, void *residual_out, const void *x, const void *residual, const void *weight, float eps,
                                    float weight_offset, unsigned m, unsigned k, int a_type, int format, unsigned block);

/*
 * Tune-and-persist (replaces the reference's `bench_matmul -algo tune`, tools/benchmarks/matmul/main.cc:269-325, which
 * enumerates and times every solution on the user's device but leaves the winning id for the user to carry around).
 *
 * petit_gemm_tune() runs every kernel of the class that fits (m, n, k) and `workspace_bytes`, with the K splits its kind
 * supports: first CHECKS the candidate's output against the class's reference kernel (|c - ref| <= tolerance * max(rms(ref), |ref|),
 * every element), then times it with HIP events on `stream` (launches rotate over the weight copies so that the 256 MB
 * Infinity Cache cannot serve them), and returns the fastest id and its microseconds per launch.  With persist != 0 the
 * winner becomes what PETIT_SOLUTION_AUTO (klass 0) or PETIT_SOLUTION_AUTO_NATIVE_* (klass 8 / 4) picks for (dtypes, n, k)
 * and the M bucket of m (or [m_lo, m_hi] when given) from now on, in this process; petit_tune_save() writes all such rows in
 * the $PETIT_AMD_TUNE_FILE format, which a later process loads on its first call.  `c` is scratch output (overwritten).
 * The call synchronises `stream`, allocates device memory (from the pool of petit_tune_reserve when there is one, else with hipMalloc)
 * and must not run inside a graph capture (PETIT_ERROR_BAD_ARGUMENT).  Returns PETIT_ERROR_KERNEL_SHAPE when no candidate passed.
 * $PETIT_AMD_AUTOTUNE=1 does the same implicitly: the first PETIT_SOLUTION_AUTO call of a (dtypes, n, k, M bucket) that no table
 * knows is tuned in place before it runs -- once per key and process, with the scratch of THAT call (so the winner is a kernel this
 * caller can run) and device memory from the pool of petit_tune_reserve (else hipMalloc).  Every tuning run exchanges the calling
 * thread's stream-capture mode to hipStreamCaptureModeRelaxed for its duration: measured on ROCm 7.2 (tools/probes/capture_legal.hip),
 * that is what lets it synchronise its own stream and allocate while a capture is in progress on ANOTHER stream of the process (global
 * capture mode: torch.cuda.graph) without invalidating that capture; a capture on the tuning stream itself is refused as above.  When
 * $PETIT_AMD_TUNE_FILE is set the new row is merged into that file (rows other processes saved meanwhile are kept; the file is
 * replaced by rename(), under an advisory lock on "<file>.lock").
 */
typedef struct petit_tune_params {
    uint32_t struct_bytes;       /* sizeof(petit_tune_params) */
    int32_t klass;               /* 0: the exact kernels; 8 / 4: the native class, MXFP8 / MXFP4 activations (MXFP4 weights only) */
    uint32_t n_copies;           /* >= 1 packed (weights, scales) pairs to rotate over */
    uint32_t launches;           /* launches per timed sample; 0 = sized so that a sample lasts ~0.3 ms */
    const void *const *b;        /* n_copies device pointers: packed weights */
    const void *const *scales;   /* n_copies device pointers: packed scales */
    uint64_t rotate_bytes;       /* n_copies == 1 only: clone the pair on the device until the rotation covers this many bytes
                                    (0 = time on the single copy: cache-resident numbers for small shapes) */
    uint32_t samples;            /* timed samples per candidate, median reported; 0 = 5 */
    float tolerance;             /* 0 = 2e-2 */
    int32_t persist;             /* insert the winner into the run-time arch table */
    uint32_t m_lo, m_hi;         /* M range of the persisted row; 0, 0 = the bucket of m (1, 2, 3-4, 5-8, ..., 129-256, 257+) */
    uint32_t reserved;
} petit_tune_params;
int petit_gemm_tune(unsigned *c, const unsigned *a, const float *global_scale, unsigned m, unsigned n, unsigned k,
                    const petit_solution_hints *hints, const petit_tune_params *params, void *workspace, uint64_t workspace_bytes,
                    void *stream, uint64_t *best_solution, float *best_us);
/* Hand the tuner a block of device memory (256-byte aligned; the caller keeps ownership and must keep it alive until it reserves
 * another block or nullptr) for the current device: the reference output, result words and the clones of the caller's weights that a
 * tuning run rotates over come out of it.  Sized for the largest problem to be tuned: M*N*2 bytes + as many (weights + scales) copies
 * as fit, ideally > 256 MB of them (fewer copies = timings that see the Infinity Cache; the ranking still holds); what does not fit is
 * allocated with hipMalloc for the run.  Optional: it spares a serving process the allocation of a few hundred MB inside a GEMM call, and
 * it is what makes tuning possible when the process's own allocator already holds the whole device. */
int petit_tune_reserve(void *device_ptr, uint64_t bytes);
/* Add one row by hand (e.g. from a sweep done elsewhere): solution must be a kernel id of this build. */
int petit_tune_insert(const petit_solution_hints *hints, unsigned n, unsigned k, unsigned m_lo, unsigned m_hi, uint64_t solution);
/* Write the run-time rows and the rows loaded from $PETIT_AMD_TUNE_FILE to `path` (same format). */
int petit_tune_save(const char *path);
/* Bumped whenever a row is added: callers that memoise petit_gemm_workspace_bytes / default picks key their cache on it. */
uint64_t petit_tune_generation(void);

/* Human-readable text for a return code. */
const char *petit_error_string(int code);
/* Layout tag of the packed tensors ("petit-cdna4/1") and library version. */
const char *petit_layout_tag(void);
const char *petit_version(void);
/* One-line description of a solution id ("stream bf16xnvfp4 mt1 nt1 wn1 wk8 d8 ..."),
 * written into buf (at most len bytes, NUL-terminated). Returns 0 or
 * PETIT_ERROR_KERNEL_SHAPE for an unknown id. */
int petit_describe_solution(uint64_t solution_id, char *buf, unsigned len);

#ifdef __cplusplus
}
#endif
#endif /* PETIT_AMD_H_ */
