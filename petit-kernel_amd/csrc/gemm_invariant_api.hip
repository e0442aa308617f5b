// gemm_invariant_api.hip -- the C ABI of the batch-invariant GEMM family (include/petit_amd.h "Batch-invariant GEMM", "Batch-invariant MoE
// launch" and their two "... on the native class" sections): ONE entry routine behind the eight launch entries, and the queries and CPU twins as
// reads of gemm_invariant_host.h, where everything that needs no GPU is (the call description, the plan, the checks, the twins).  The kernels
// are in gemm_invariant.hpp, gemm_invariant_moe.hpp, gemm_native_invariant.hpp and gemm_native_invariant_moe.hpp, instantiated by the
// gemm_invariant_*.hip / gemm_native_invariant_*.hip next to this file.  Nothing here goes through dispatch.hip, pick.hip, moe_choose, the arch
// tables or the tuner: the kernels a call runs are a function of (m, num_experts, formats, types) alone, and a row's result of (n, k, formats,
// types) alone.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "gemm_invariant_host.h"
#include "gemm_native_invariant_moe.hpp"
#include "petit_internal.h"
#include "solution.h"

namespace petit_amd {

namespace inv = invariant;
static_assert((int)inv::kRcOk == (int)kOk && (int)inv::kRcProblemShape == (int)kErrProblemShape && (int)inv::kRcKernelShape == (int)kErrKernelShape &&
              (int)inv::kRcBadArgument == (int)kErrBadArgument);
static_assert((int)inv::kTypeNv == (int)kDataTypeFp4e2m1 && (int)inv::kTypeFp16 == (int)kDataTypeFp16 && (int)inv::kTypeBf16 == (int)kDataTypeBf16 &&
              (int)inv::kTypeMx == (int)kDataTypeMxFp4e2m1 && (int)inv::kTypeMxF16Range == (int)kDataTypeMxFp4e2m1F16Range);
static_assert(inv::kMoeMaxExperts == kMoeMaxExperts && inv::kMaxRows == kMaxM);

extern template void invariant_launch<Bf16, kFmtNv>(const InvariantArgs &, const inv::Plan &, hipStream_t);
extern template void invariant_launch<Bf16, kFmtMx>(const InvariantArgs &, const inv::Plan &, hipStream_t);
extern template void invariant_launch<Fp16, kFmtNv>(const InvariantArgs &, const inv::Plan &, hipStream_t);
extern template void invariant_moe_launch<Bf16, kFmtNv>(InvariantMoeArgs, const inv::Plan &, hipStream_t);
extern template void invariant_moe_launch<Bf16, kFmtMx>(InvariantMoeArgs, const inv::Plan &, hipStream_t);
extern template void invariant_moe_launch<Fp16, kFmtNv>(InvariantMoeArgs, const inv::Plan &, hipStream_t);
extern template void native_invariant_launch<Bf16>(const NativeInvariantArgs &, int, const inv::Plan &, hipStream_t);
extern template void native_invariant_launch<Fp16>(const NativeInvariantArgs &, int, const inv::Plan &, hipStream_t);
extern template void native_invariant_moe_launch<Bf16>(const NativeInvariantMoeArgs &, int, const inv::Plan &, hipStream_t);
extern template void native_invariant_moe_launch<Fp16>(const NativeInvariantMoeArgs &, int, const inv::Plan &, hipStream_t);
extern template void native_invariant_launch<Bf16, 6>(const NativeInvariantArgs &, int, const inv::Plan &, hipStream_t);
extern template void native_invariant_launch<Fp16, 6>(const NativeInvariantArgs &, int, const inv::Plan &, hipStream_t);
extern template void native_invariant_moe_launch<Bf16, 6>(const NativeInvariantMoeArgs &, int, const inv::Plan &, hipStream_t);
extern template void native_invariant_moe_launch<Fp16, 6>(const NativeInvariantMoeArgs &, int, const inv::Plan &, hipStream_t);

namespace {

// the pointers of a call (the last three of the first line: the MoE entries')
struct Operands {
    void *c;
    const void *a, *b, *scales;
    const float *gs;
    const int32_t *offsets, *a_idx, *c_idx;
    const petit_solution_hints *hints;
    const petit_epilogue *epilogue;
    void *workspace, *stream;
};

// the kernel arguments of a class: the fields every struct has, then what the struct has of the quantised A, the routing and the A gather
template <class Args> Args make_args(const inv::Call &call, const inv::Plan &plan, const Operands &o, const void *a, const void *bias) {
    Args p{};
    p.c = o.c, p.w = o.b, p.s = o.scales, p.gs = o.gs, p.bias = bias, p.slabs = (float *)((char *)o.workspace + plan.quant_bytes);
    p.m = call.m, p.n = call.n, p.k = call.k, p.act = (unsigned)call.activation, p.slices = plan.slices, p.slice_k = plan.slice_k;
    if constexpr (requires { p.qa; })
        p.qa = (const unsigned char *)a;
    else
        p.a = a;
    if constexpr (requires { p.offsets; })
        p.offsets = o.offsets, p.c_idx = o.c_idx, p.experts = call.num_experts, p.c_rows = call.c_rows;
    if constexpr (requires { p.a_idx; })
        p.a_idx = o.a_idx, p.a_rows = call.a_rows;
    return p;
}

// One call of any entry.  `call` names the class, the weight format the entry point stands for, the activation format, the numbers and which
// row indices exist; its a_type and activation are read here, from the hints and the epilogue.
int run(inv::Call call, const Operands &o) {
    const petit_solution_hints *const hints = o.hints;
    const petit_epilogue *const epilogue = o.epilogue;
    // (the entry point names the format; the hints must agree with it)
    if (!hints || hints->c_type != hints->a_type || (is_mx_type(call.b_type) ? !is_mx_type(hints->b_type) : hints->b_type != kDataTypeFp4e2m1))
        return kErrBadArgument;
    if (epilogue && epilogue->reserved != 0)
        return kErrBadArgument;
    call.a_type = hints->a_type, call.activation = epilogue ? epilogue->activation : 0;
    const inv::Plan plan = inv::plan(call);
    if (plan.rc != kOk)
        return plan.rc;
    if (call.moe && !o.offsets)
        return kErrProblemShape;
    if (call.m == 0)
        return kOk;
    const void *bias = epilogue ? epilogue->bias : nullptr;
    const int prc = call.moe ? inv::moe_pointers_rc(o.c, o.a, o.b, o.scales, o.gs, o.offsets, o.a_idx, o.c_idx, bias, o.workspace, plan.workspace_bytes)
                             : inv::pointers_rc(o.c, o.a, o.b, o.scales, bias, o.workspace, plan.workspace_bytes);
    if (prc != kOk)
        return prc;
    const hipStream_t s = (hipStream_t)o.stream;
    const bool bf16 = call.a_type == kDataTypeBf16;
    const void *a = o.a;
    if (call.native && !call.a_is_quantized) { // the library's own quantiser (MoE: the gathering one): the bytes are a function of the row alone
        const unsigned m = call.m, k = call.k;
        const int fmt = call.act_format;
        const int qrc = call.moe ? (bf16 ? quantize32_rows_bf16(a, o.a_idx, call.a_rows, o.workspace, m, k, fmt, s)
                                         : quantize32_rows_f16(a, o.a_idx, call.a_rows, o.workspace, m, k, fmt, s))
                                 : (bf16 ? quantize32_bf16(a, o.workspace, m, k, fmt, s) : quantize32_f16(a, o.workspace, m, k, fmt, s));
        if (qrc != kOk)
            return qrc;
        a = o.workspace;
    }
    const bool image = call.native && call.b_type == kDataTypeFp4e2m1; // the NVFP4 image(s): o.b, the scale region of the first at o.scales
    if (call.native && call.moe) {
        const auto p = make_args<NativeInvariantMoeArgs>(call, plan, o, a, bias);
        if (image)
            bf16 ? native_invariant_moe_launch<Bf16, 6>(p, call.act_format, plan, s) : native_invariant_moe_launch<Fp16, 6>(p, call.act_format, plan, s);
        else
            bf16 ? native_invariant_moe_launch<Bf16>(p, call.act_format, plan, s) : native_invariant_moe_launch<Fp16>(p, call.act_format, plan, s);
    } else if (call.native) {
        const auto p = make_args<NativeInvariantArgs>(call, plan, o, a, bias);
        if (image)
            bf16 ? native_invariant_launch<Bf16, 6>(p, call.act_format, plan, s) : native_invariant_launch<Fp16, 6>(p, call.act_format, plan, s);
        else
            bf16 ? native_invariant_launch<Bf16>(p, call.act_format, plan, s) : native_invariant_launch<Fp16>(p, call.act_format, plan, s);
    } else if (call.moe) {
        const auto p = make_args<InvariantMoeArgs>(call, plan, o, a, bias);
        if (bf16 && is_mx_type(call.b_type))
            invariant_moe_launch<Bf16, kFmtMx>(p, plan, s);
        else if (bf16)
            invariant_moe_launch<Bf16, kFmtNv>(p, plan, s);
        else
            invariant_moe_launch<Fp16, kFmtNv>(p, plan, s);
    } else {
        const auto p = make_args<InvariantArgs>(call, plan, o, a, bias);
        if (bf16 && is_mx_type(call.b_type))
            invariant_launch<Bf16, kFmtMx>(p, plan, s);
        else if (bf16)
            invariant_launch<Bf16, kFmtNv>(p, plan, s);
        else
            invariant_launch<Fp16, kFmtNv>(p, plan, s);
    }
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

// the call a query describes: no activation, no indices, matrices of m rows
inline inv::Call moe_query(inv::Call c, unsigned num_experts) { return inv::moe_call(c, num_experts, false, c.m, false, c.m); }

} // namespace
} // namespace petit_amd

using namespace petit_amd;

extern "C" {

// ---- queries: reads of the plan ------------------------------------------------------------------------------------------------------------

void petit_gemm_invariant_geometry(unsigned n, unsigned k, int a_type, int b_type, unsigned *slices, unsigned *slice_k) {
    const inv::Plan p = inv::plan(inv::dense_call(0, n, k, a_type, b_type, 0));
    if (slices)
        *slices = p.slices;
    if (slice_k)
        *slice_k = p.slice_k;
}

unsigned petit_gemm_invariant_slabs(unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    const inv::Plan p = inv::plan(inv::dense_call(m, n, k, a_type, b_type, 0));
    return p.split ? p.slices : 1u;
}

uint64_t petit_gemm_invariant_workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    return inv::plan(inv::dense_call(m, n, k, a_type, b_type, 0)).workspace_bytes;
}

unsigned petit_gemm_native_invariant_slabs(unsigned m, unsigned n, unsigned k, int a_type) {
    const inv::Plan p = inv::plan(inv::native_call(m, n, k, a_type, 8, 1, 0));
    return p.split ? p.slices : 1u;
}

uint64_t petit_gemm_native_invariant_workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int act_format, int a_is_quantized) {
    return inv::plan(inv::native_call(m, n, k, a_type, act_format, a_is_quantized, 0)).workspace_bytes;
}

int petit_gemm_moe_invariant_form(unsigned m, unsigned num_experts) {
    return inv::plan(moe_query(inv::dense_call(m, 0, 0, 0, 0, 0), num_experts)).split ? 1 : 0;
}

uint64_t petit_gemm_moe_invariant_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    return inv::plan(moe_query(inv::dense_call(m, n, k, a_type, b_type, 0), num_experts)).workspace_bytes;
}

int petit_gemm_native_moe_invariant_form(unsigned m, unsigned num_experts) {
    return inv::plan(moe_query(inv::native_call(m, 0, 0, 0, 8, 1, 0), num_experts)).split ? 1 : 0;
}

uint64_t petit_gemm_native_moe_invariant_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int act_format,
                                                         int a_is_quantized) {
    return inv::plan(moe_query(inv::native_call(m, n, k, a_type, act_format, a_is_quantized, 0), num_experts)).workspace_bytes;
}

// ---- launches: argument forwarding to run() ------------------------------------------------------------------------------------------------

int petit_gemm_fp4_fp16_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                  unsigned k, const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return run(inv::dense_call(m, n, k, 0, kDataTypeFp4e2m1, 0),
               {c, a, b, scales, global_scale, nullptr, nullptr, nullptr, hints, epilogue, workspace, stream});
}

int petit_gemm_mxfp4_fp16_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                    unsigned k, const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return run(inv::dense_call(m, n, k, 0, kDataTypeMxFp4e2m1, 0),
               {c, a, b, scales, global_scale, nullptr, nullptr, nullptr, hints, epilogue, workspace, stream});
}

int petit_gemm_mxfp4_native_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                      unsigned k, const petit_solution_hints *hints, int act_format, int a_is_quantized,
                                      const petit_epilogue *epilogue, void *workspace, void *stream) {
    return run(inv::native_call(m, n, k, 0, act_format, a_is_quantized, 0),
               {c, a, b, scales, global_scale, nullptr, nullptr, nullptr, hints, epilogue, workspace, stream});
}

int petit_gemm_fp4_fp16_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                      const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                      const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                      const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return run(inv::moe_call(inv::dense_call(m, n, k, 0, kDataTypeFp4e2m1, 0), num_experts, a_row_index != nullptr, a_rows,
                             c_row_index != nullptr, c_rows),
               {c, a, b, scales, global_scales, expert_offsets, a_row_index, c_row_index, hints, epilogue, workspace, stream});
}

int petit_gemm_mxfp4_fp16_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                        const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                        const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                        const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return run(inv::moe_call(inv::dense_call(m, n, k, 0, kDataTypeMxFp4e2m1, 0), num_experts, a_row_index != nullptr, a_rows,
                             c_row_index != nullptr, c_rows),
               {c, a, b, scales, global_scales, expert_offsets, a_row_index, c_row_index, hints, epilogue, workspace, stream});
}

int petit_gemm_mxfp4_native_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                          const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                          const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                          const petit_solution_hints *hints, int act_format, int a_is_quantized, const petit_epilogue *epilogue,
                                          void *workspace, void *stream) {
    return run(inv::moe_call(inv::native_call(m, n, k, 0, act_format, a_is_quantized, 0), num_experts, a_row_index != nullptr, a_rows,
                             c_row_index != nullptr, c_rows),
               {c, a, b, scales, global_scales, expert_offsets, a_row_index, c_row_index, hints, epilogue, workspace, stream});
}

// the image entries: `image` takes the place of (b, scales) -- the scale region follows the (first) image's elements
int petit_gemm_nvfp4_native_invariant(void *c, const void *a, const void *image, const float *global_scale, unsigned m, unsigned n, unsigned k,
                                      const petit_solution_hints *hints, int act_format, int a_is_quantized, const petit_epilogue *epilogue,
                                      void *workspace, void *stream) {
    const void *const scales = image ? (const char *)image + nv6_elem_bytes(n, k) : nullptr;
    return run(inv::native_call(m, n, k, 0, act_format, a_is_quantized, 0, kDataTypeFp4e2m1, image),
               {c, a, image, scales, global_scale, nullptr, nullptr, nullptr, hints, epilogue, workspace, stream});
}

int petit_gemm_nvfp4_native_moe_invariant(void *c, const void *a, const void *images, const float *global_scales, const int32_t *expert_offsets,
                                          unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index, unsigned a_rows,
                                          const int32_t *c_row_index, unsigned c_rows, const petit_solution_hints *hints, int act_format,
                                          int a_is_quantized, const petit_epilogue *epilogue, void *workspace, void *stream) {
    const void *const scales = images ? (const char *)images + nv6_elem_bytes(n, k) : nullptr;
    return run(inv::moe_call(inv::native_call(m, n, k, 0, act_format, a_is_quantized, 0, kDataTypeFp4e2m1, images), num_experts,
                             a_row_index != nullptr, a_rows, c_row_index != nullptr, c_rows),
               {c, a, images, scales, global_scales, expert_offsets, a_row_index, c_row_index, hints, epilogue, workspace, stream});
}

// ---- the CPU twins -------------------------------------------------------------------------------------------------------------------------

int petit_gemm_fp4_invariant_host(void *c, const void *a, const void *b, const void *scales, const float *global_scale, const void *bias,
                                  unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    return inv::gemm_host(c, a, b, scales, global_scale, bias, m, n, k, a_type, b_type);
}

int petit_gemm_native_invariant_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scale, const void *bias,
                                     unsigned m, unsigned n, unsigned k, int a_type, int act_format) {
    return inv::native_gemm_host(c, qa, b, scales, global_scale, bias, m, n, k, a_type, act_format);
}

int petit_gemm_fp4_moe_invariant_host(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const void *bias,
                                      const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                      const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows, int a_type,
                                      int b_type) {
    return inv::moe_gemm_host(c, a, b, scales, global_scales, bias, expert_offsets, num_experts, m, n, k, a_row_index, a_rows, c_row_index,
                              c_rows, a_type, b_type);
}

int petit_gemm_native_moe_invariant_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scales, const void *bias,
                                         const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                         const int32_t *c_row_index, unsigned c_rows, int a_type, int act_format) {
    return inv::native_moe_gemm_host(c, qa, b, scales, global_scales, bias, expert_offsets, num_experts, m, n, k, c_row_index, c_rows, a_type,
                                     act_format);
}

int petit_gemm_nvfp4_native_invariant_host(void *c, const void *qa, const void *image, const float *global_scale, const void *bias, unsigned m,
                                           unsigned n, unsigned k, int a_type, int act_format) {
    return inv::nv_native_gemm_host(c, qa, image, global_scale, bias, m, n, k, a_type, act_format);
}

int petit_gemm_nvfp4_native_moe_invariant_host(void *c, const void *qa, const void *images, const float *global_scales, const void *bias,
                                               const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                               const int32_t *c_row_index, unsigned c_rows, int a_type, int act_format) {
    return inv::nv_native_moe_gemm_host(c, qa, images, global_scales, bias, expert_offsets, num_experts, m, n, k, c_row_index, c_rows, a_type,
                                        act_format);
}

int petit_quantize_activations_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format) {
    return quantize_activations_host(qa, a, m, k, a_type, format);
}

} // extern "C"
