// gemm_invariant.hip -- the C ABI of the batch-invariant dense GEMM (include/petit_amd.h "Batch-invariant GEMM"): queries, argument checks,
// the form switch and the launches.  The kernels are in gemm_invariant.hpp, instantiated per (format, type) pair by gemm_invariant_*.hip; what
// needs no GPU (geometry, checks, the CPU twin) is in gemm_invariant_host.h.  Nothing here goes through dispatch.hip, pick.hip, the arch tables
// or the tuner: the kernel a call runs is a function of (m, n, k, types) alone, and its result of (n, k, types) alone.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "gemm_invariant.hpp"
#include "gemm_invariant_host.h"
#include "petit_internal.h"

namespace petit_amd {

namespace inv = invariant;
static_assert((int)inv::kRcOk == (int)kOk && (int)inv::kRcProblemShape == (int)kErrProblemShape && (int)inv::kRcKernelShape == (int)kErrKernelShape &&
              (int)inv::kRcBadArgument == (int)kErrBadArgument);
static_assert((int)inv::kTypeNv == (int)kDataTypeFp4e2m1 && (int)inv::kTypeFp16 == (int)kDataTypeFp16 && (int)inv::kTypeBf16 == (int)kDataTypeBf16 &&
              (int)inv::kTypeMx == (int)kDataTypeMxFp4e2m1 && (int)inv::kTypeMxF16Range == (int)kDataTypeMxFp4e2m1F16Range && inv::kMaxRows == kMaxM);

extern template void invariant_launch<Bf16, kFmtNv>(const InvariantArgs &, bool, hipStream_t);
extern template void invariant_launch<Bf16, kFmtMx>(const InvariantArgs &, bool, hipStream_t);
extern template void invariant_launch<Fp16, kFmtNv>(const InvariantArgs &, bool, hipStream_t);

namespace {

// the form switch: a function of m alone.  Either form gives the same bits, so it is a speed choice only.
constexpr unsigned split_max_m() { return inv::kSplitMaxM; }

int gemm_invariant(int b_type, void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                   unsigned k, const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    if (!hints)
        return kErrBadArgument;
    if (hints->c_type != hints->a_type || (is_mx_type(b_type) ? !is_mx_type(hints->b_type) : hints->b_type != kDataTypeFp4e2m1))
        return kErrBadArgument; // (the entry point names the format; the hints must agree with it)
    const int a_type = hints->a_type, act = epilogue ? epilogue->activation : 0;
    if (epilogue && epilogue->reserved != 0)
        return kErrBadArgument;
    const int rc = inv::shape_rc(m, n, k, a_type, b_type, act);
    if (rc != kOk)
        return rc;
    if (m == 0)
        return kOk;
    const void *bias = epilogue ? epilogue->bias : nullptr;
    const uint64_t need = inv::workspace_bytes(m, n, k, a_type, b_type, split_max_m());
    const int prc = inv::pointers_rc(c, a, b, scales, bias, workspace, need);
    if (prc != kOk)
        return prc;
    InvariantArgs p{};
    p.c = c, p.a = a, p.w = b, p.s = scales, p.gs = global_scale, p.bias = bias, p.slabs = (float *)workspace;
    p.m = m, p.n = n, p.k = k, p.act = (unsigned)act;
    inv::geometry(n, k, a_type, b_type, &p.slices, &p.slice_k);
    const bool whole = m > split_max_m();
    const hipStream_t s = (hipStream_t)stream;
    if (a_type == kDataTypeBf16 && is_mx_type(b_type))
        invariant_launch<Bf16, kFmtMx>(p, whole, s);
    else if (a_type == kDataTypeBf16)
        invariant_launch<Bf16, kFmtNv>(p, whole, s);
    else
        invariant_launch<Fp16, kFmtNv>(p, whole, s);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

} // namespace
} // namespace petit_amd

using namespace petit_amd;

extern "C" {

void petit_gemm_invariant_geometry(unsigned n, unsigned k, int a_type, int b_type, unsigned *slices, unsigned *slice_k) {
    unsigned S, L;
    inv::geometry(n, k, a_type, b_type, &S, &L);
    if (slices)
        *slices = S;
    if (slice_k)
        *slice_k = L;
}

unsigned petit_gemm_invariant_slabs(unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    return inv::slabs(m, n, k, a_type, b_type, split_max_m());
}

uint64_t petit_gemm_invariant_workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    return inv::workspace_bytes(m, n, k, a_type, b_type, split_max_m());
}

int petit_gemm_fp4_fp16_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                  unsigned k, const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return gemm_invariant(kDataTypeFp4e2m1, c, a, b, scales, global_scale, m, n, k, hints, epilogue, workspace, stream);
}

int petit_gemm_mxfp4_fp16_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                    unsigned k, const petit_solution_hints *hints, const petit_epilogue *epilogue, void *workspace, void *stream) {
    return gemm_invariant(kDataTypeMxFp4e2m1, c, a, b, scales, global_scale, m, n, k, hints, epilogue, workspace, stream);
}

int petit_gemm_fp4_invariant_host(void *c, const void *a, const void *b, const void *scales, const float *global_scale, const void *bias,
                                  unsigned m, unsigned n, unsigned k, int a_type, int b_type) {
    return inv::gemm_host(c, a, b, scales, global_scale, bias, m, n, k, a_type, b_type);
}

} // extern "C"
