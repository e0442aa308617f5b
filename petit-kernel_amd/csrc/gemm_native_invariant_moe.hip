// gemm_native_invariant_moe.hip -- the C ABI of the batch-invariant MoE launch on the native class (include/petit_amd.h "Batch-invariant MoE
// launch on the native class"): queries, argument checks, the gathering quantiser in front of a 16-bit input, the form switch and the launches.
// The kernels are in gemm_native_invariant_moe.hpp, instantiated per activation type by gemm_native_invariant_moe_{bf16,f16}.hip; what needs no
// GPU (checks, workspace arithmetic, the CPU twin) is in gemm_native_invariant_moe_host.h.  Nothing here goes through moe_choose, the arch tables
// or the tuner: the kernels a call runs are a function of (m, num_experts, formats, types) alone, and a row's result of (n, k, formats, types).
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "gemm_native_invariant_moe.hpp"
#include "gemm_native_invariant_moe_host.h"
#include "petit_internal.h"
#include "solution.h"

namespace petit_amd {

namespace ninv = native_invariant;
static_assert(invariant::kMoeMaxExperts == kMoeMaxExperts && invariant::kMaxRows == kMaxM);

extern template void native_invariant_moe_launch<Bf16>(const NativeInvariantMoeArgs &, int, bool, hipStream_t);
extern template void native_invariant_moe_launch<Fp16>(const NativeInvariantMoeArgs &, int, bool, hipStream_t);

} // namespace petit_amd

using namespace petit_amd;

extern "C" {

int petit_gemm_native_moe_invariant_form(unsigned m, unsigned num_experts) { return ninv::moe_split(m, num_experts) ? 1 : 0; }

uint64_t petit_gemm_native_moe_invariant_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int act_format,
                                                         int a_is_quantized) {
    return ninv::moe_workspace_bytes(num_experts, m, n, k, a_type, act_format, a_is_quantized);
}

int petit_gemm_mxfp4_native_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                          const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                          const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                          const petit_solution_hints *hints, int act_format, int a_is_quantized, const petit_epilogue *epilogue,
                                          void *workspace, void *stream) {
    if (!hints || hints->c_type != hints->a_type || !is_mx_type(hints->b_type))
        return kErrBadArgument;
    if (epilogue && epilogue->reserved != 0)
        return kErrBadArgument;
    const int a_type = hints->a_type, act = epilogue ? epilogue->activation : 0;
    const int rc = ninv::moe_shape_rc(num_experts, m, n, k, a_row_index, a_rows, c_row_index, c_rows, a_type, act_format, a_is_quantized, act);
    if (rc != kOk)
        return rc;
    if (!expert_offsets)
        return kErrProblemShape;
    if (m == 0)
        return kOk;
    const void *bias = epilogue ? epilogue->bias : nullptr;
    const uint64_t q_part = ninv::moe_quant_part_bytes(m, k, act_format, a_is_quantized);
    const uint64_t need = q_part + ninv::moe_slab_part_bytes(num_experts, m, n, k, a_type);
    const int prc = invariant::moe_pointers_rc(c, a, b, scales, global_scales, expert_offsets, a_row_index, c_row_index, bias, workspace, need);
    if (prc != kOk)
        return prc;
    const hipStream_t s = (hipStream_t)stream;
    NativeInvariantMoeArgs p{};
    p.c = c, p.qa = (const unsigned char *)a, p.w = b, p.s = scales, p.gs = global_scales, p.bias = bias;
    p.slabs = (float *)((char *)workspace + q_part);
    p.offsets = expert_offsets, p.c_idx = c_row_index;
    p.m = m, p.n = n, p.k = k, p.act = (unsigned)act, p.experts = num_experts, p.c_rows = c_rows;
    invariant::geometry(n, k, a_type, kDataTypeMxFp4e2m1, &p.slices, &p.slice_k);
    if (!a_is_quantized) { // the gathering quantiser (petit_quantize_activations_rows' launch): the bytes are a function of the row alone
        const int qrc = a_type == kDataTypeBf16 ? quantize32_rows_bf16(a, a_row_index, a_rows, workspace, m, k, act_format, s)
                                                : quantize32_rows_f16(a, a_row_index, a_rows, workspace, m, k, act_format, s);
        if (qrc != kOk)
            return qrc;
        p.qa = (const unsigned char *)workspace;
    }
    const bool split = ninv::moe_split(m, num_experts); // either form gives the same bits: a speed choice only
    if (a_type == kDataTypeBf16)
        native_invariant_moe_launch<Bf16>(p, act_format, split, s);
    else
        native_invariant_moe_launch<Fp16>(p, act_format, split, s);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int petit_gemm_native_moe_invariant_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scales, const void *bias,
                                         const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                         const int32_t *c_row_index, unsigned c_rows, int a_type, int act_format) {
    return ninv::moe_gemm_host(c, qa, b, scales, global_scales, bias, expert_offsets, num_experts, m, n, k, c_row_index, c_rows, a_type,
                               act_format);
}

} // extern "C"
