// gemm_invariant_moe.hip -- the C ABI of the batch-invariant routed-expert (MoE) GEMM (include/petit_amd.h "Batch-invariant MoE launch"):
// queries, argument checks, the form switch and the launches.  The kernels are in gemm_invariant_moe.hpp, instantiated per (format, type) pair
// by gemm_invariant_moe_*.hip; what needs no GPU (checks, workspace arithmetic, the CPU twin) is in gemm_invariant_host.h.  Nothing here goes
// through moe_choose, the arch tables or the tuner: the kernels a call runs are a function of (m, num_experts, types) alone, and a row's
// result of (n, k, types) alone.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "gemm_invariant_host.h"
#include "gemm_invariant_moe.hpp"
#include "petit_internal.h"

namespace petit_amd {

namespace inv = invariant;
static_assert(inv::kMoeMaxExperts == kMoeMaxExperts && inv::kMaxRows == kMaxM);

extern template void invariant_moe_launch<Bf16, kFmtNv>(InvariantMoeArgs, bool, hipStream_t);
extern template void invariant_moe_launch<Bf16, kFmtMx>(InvariantMoeArgs, bool, hipStream_t);
extern template void invariant_moe_launch<Fp16, kFmtNv>(InvariantMoeArgs, bool, hipStream_t);

namespace {

int gemm_moe_invariant(int b_type, void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                       const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index,
                       unsigned a_rows, const int32_t *c_row_index, unsigned c_rows, const petit_solution_hints *hints,
                       const petit_epilogue *epilogue, void *workspace, void *stream) {
    if (!hints)
        return kErrBadArgument;
    if (hints->c_type != hints->a_type || (is_mx_type(b_type) ? !is_mx_type(hints->b_type) : hints->b_type != kDataTypeFp4e2m1))
        return kErrBadArgument; // (the entry point names the format; the hints must agree with it)
    const int a_type = hints->a_type, act = epilogue ? epilogue->activation : 0;
    if (epilogue && epilogue->reserved != 0)
        return kErrBadArgument;
    const int rc = inv::moe_shape_rc(num_experts, m, n, k, a_row_index, a_rows, c_row_index, c_rows, a_type, b_type, act);
    if (rc != kOk)
        return rc;
    if (!expert_offsets)
        return kErrProblemShape;
    if (m == 0)
        return kOk;
    const void *bias = epilogue ? epilogue->bias : nullptr;
    const uint64_t need = inv::moe_workspace_bytes(num_experts, m, n, k, a_type, b_type);
    const int prc = inv::moe_pointers_rc(c, a, b, scales, global_scales, expert_offsets, a_row_index, c_row_index, bias, workspace, need);
    if (prc != kOk)
        return prc;
    InvariantMoeArgs p{};
    p.c = c, p.a = a, p.w = b, p.s = scales, p.gs = global_scales, p.bias = bias, p.slabs = (float *)workspace;
    p.offsets = expert_offsets, p.a_idx = a_row_index, p.c_idx = c_row_index;
    p.m = m, p.n = n, p.k = k, p.act = (unsigned)act, p.experts = num_experts, p.a_rows = a_rows, p.c_rows = c_rows;
    inv::geometry(n, k, a_type, b_type, &p.slices, &p.slice_k);
    const bool split = inv::moe_split(m, num_experts);
    const hipStream_t s = (hipStream_t)stream;
    if (a_type == kDataTypeBf16 && is_mx_type(b_type))
        invariant_moe_launch<Bf16, kFmtMx>(p, split, s);
    else if (a_type == kDataTypeBf16)
        invariant_moe_launch<Bf16, kFmtNv>(p, split, s);
    else
        invariant_moe_launch<Fp16, kFmtNv>(p, split, s);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

} // namespace
} // namespace petit_amd

using namespace petit_amd;

extern "C" {

int petit_gemm_moe_invariant_form(unsigned m, unsigned num_experts) { return inv::moe_split(m, num_experts) ? 1 : 0; }

uint64_t petit_gemm_moe_invariant_workspace_bytes(unsigned num_experts, unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    return inv::moe_workspace_bytes(num_experts, m, n, k, a_type, b_type);
}

int petit_gemm_fp4_fp16_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                      const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                      const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                      const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return gemm_moe_invariant(kDataTypeFp4e2m1, c, a, b, scales, global_scales, expert_offsets, num_experts, m, n, k, a_row_index, a_rows,
                              c_row_index, c_rows, hints, epilogue, workspace, stream);
}

int petit_gemm_mxfp4_fp16_moe_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                        const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                        const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                        const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return gemm_moe_invariant(kDataTypeMxFp4e2m1, c, a, b, scales, global_scales, expert_offsets, num_experts, m, n, k, a_row_index, a_rows,
                              c_row_index, c_rows, hints, epilogue, workspace, stream);
}

int petit_gemm_fp4_moe_invariant_host(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const void *bias,
                                      const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                      const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows, int a_type,
                                      int b_type) {
    return inv::moe_gemm_host(c, a, b, scales, global_scales, bias, expert_offsets, num_experts, m, n, k, a_row_index, a_rows, c_row_index,
                              c_rows, a_type, b_type);
}

} // extern "C"
