// gemm_native_invariant.hip -- the C ABI of the batch-invariant GEMM on the native class (include/petit_amd.h "Batch-invariant GEMM on the
// native class"): queries, argument checks, the library's own quantiser in front of a 16-bit input, the form switch and the launches.  The
// kernels are in gemm_native_invariant.hpp, instantiated per activation type by gemm_native_invariant_{bf16,f16}.hip; what needs no GPU (checks,
// workspace arithmetic, the CPU twin) is in gemm_native_invariant_host.h.  Nothing here goes through dispatch.hip, pick.hip, the arch tables or
// the tuner: the kernels a call runs are a function of (m, formats, types) alone, and its result of (n, k, formats, types) alone.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "gemm_native_invariant.hpp"
#include "gemm_native_invariant_host.h"
#include "petit_internal.h"
#include "solution.h"

namespace petit_amd {

namespace ninv = native_invariant;
static_assert((int)invariant::kRcKernelShape == (int)kErrKernelShape && (int)invariant::kRcBadArgument == (int)kErrBadArgument);

extern template void native_invariant_launch<Bf16>(const NativeInvariantArgs &, int, bool, hipStream_t);
extern template void native_invariant_launch<Fp16>(const NativeInvariantArgs &, int, bool, hipStream_t);

} // namespace petit_amd

using namespace petit_amd;

extern "C" {

unsigned petit_gemm_native_invariant_slabs(unsigned m, unsigned n, unsigned k, int a_type) { return ninv::slabs(m, n, k, a_type); }

uint64_t petit_gemm_native_invariant_workspace_bytes(unsigned m, unsigned n, unsigned k, int a_type, int act_format, int a_is_quantized) {
    return ninv::workspace_bytes(m, n, k, a_type, act_format, a_is_quantized);
}

int petit_gemm_mxfp4_native_invariant(void *c, const void *a, const void *b, const void *scales, const float *global_scale, unsigned m, unsigned n,
                                      unsigned k, const petit_solution_hints *hints, int act_format, int a_is_quantized,
                                      const petit_epilogue *epilogue, void *workspace, void *stream) {
    if (!hints || hints->c_type != hints->a_type || !is_mx_type(hints->b_type))
        return kErrBadArgument;
    if (epilogue && epilogue->reserved != 0)
        return kErrBadArgument;
    const int a_type = hints->a_type, act = epilogue ? epilogue->activation : 0;
    const int rc = ninv::shape_rc(m, n, k, a_type, act_format, a_is_quantized, act);
    if (rc != kOk)
        return rc;
    if (m == 0)
        return kOk;
    const void *bias = epilogue ? epilogue->bias : nullptr;
    const uint64_t q_part = ninv::quant_part_bytes(m, k, act_format, a_is_quantized), need = q_part + ninv::slab_part_bytes(m, n, k, a_type);
    const int prc = invariant::pointers_rc(c, a, b, scales, bias, workspace, need);
    if (prc != kOk)
        return prc;
    const hipStream_t s = (hipStream_t)stream;
    NativeInvariantArgs p{};
    p.c = c, p.qa = (const unsigned char *)a, p.w = b, p.s = scales, p.gs = global_scale, p.bias = bias;
    p.slabs = (float *)((char *)workspace + q_part);
    p.m = m, p.n = n, p.k = k, p.act = (unsigned)act;
    invariant::geometry(n, k, a_type, kDataTypeMxFp4e2m1, &p.slices, &p.slice_k);
    if (!a_is_quantized) { // the library's own quantiser: the bytes are a function of the row alone
        const int qrc = a_type == kDataTypeBf16 ? quantize32_bf16(a, workspace, m, k, act_format, s) : quantize32_f16(a, workspace, m, k, act_format, s);
        if (qrc != kOk)
            return qrc;
        p.qa = (const unsigned char *)workspace;
    }
    const bool whole = m > ninv::split_max_m(); // the form switch: a function of m alone.  Either form gives the same bits: a speed choice only.
    if (a_type == kDataTypeBf16)
        native_invariant_launch<Bf16>(p, act_format, whole, s);
    else
        native_invariant_launch<Fp16>(p, act_format, whole, s);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int petit_quantize_activations_host(void *qa, const void *a, unsigned m, unsigned k, int a_type, int format) {
    return quantize_activations_host(qa, a, m, k, a_type, format);
}

int petit_gemm_native_invariant_host(void *c, const void *qa, const void *b, const void *scales, const float *global_scale, const void *bias,
                                     unsigned m, unsigned n, unsigned k, int a_type, int act_format) {
    return ninv::gemm_host(c, qa, b, scales, global_scale, bias, m, n, k, a_type, act_format);
}

} // extern "C"
