// gemm_native_moe_decode_api.hip -- the C ABI of the routed-expert decode GEMM on the native images (include/petit_amd.h "MoE decode on the
// native image"): the checks and the launch.  The kernels are in gemm_native_moe_decode.hpp, instantiated by
// gemm_native_moe_decode_{bf16,f16}.hip.  Nothing here goes through dispatch.hip, pick.hip, the arch tables or the tuner, no sentinel or
// solution id reaches these kernels, and there is no workspace to query.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "gemm_native_moe_decode.hpp"
#include "petit_internal.h"

namespace petit_amd {
extern template void native_moe_decode_launch<Bf16>(const NativeMoeDecodeArgs &, int, bool, hipStream_t);
extern template void native_moe_decode_launch<Fp16>(const NativeMoeDecodeArgs &, int, bool, hipStream_t);
} // namespace petit_amd

using namespace petit_amd;

extern "C" int petit_gemm_nvfp4_native_moe_decode(void *c, const void *a, const void *images, const float *global_scales,
                                                  const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                                  const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                                  const petit_solution_hints *hints, int act_format, int a_is_quantized,
                                                  const petit_epilogue *epilogue, void *stream) {
    if (!hints || hints->c_type != hints->a_type || hints->b_type != kDataTypeFp4e2m1 || (epilogue && epilogue->reserved != 0) ||
        (hints->a_type != kDataTypeBf16 && hints->a_type != kDataTypeFp16) || (act_format != 8 && act_format != 6 && act_format != 4) ||
        (a_is_quantized != 0 && a_is_quantized != 1))
        return kErrBadArgument;
    const int activation = epilogue ? epilogue->activation : 0;
    if (!activation_known(activation) || (a_is_quantized && a_row_index))
        return kErrBadArgument;
    // the (n, k) an image exists for and whole blocks of it; the kernels' 32-bit offsets; a grid the launch can have
    if (num_experts == 0 || num_experts > kMoeMaxExperts || n == 0 || k == 0 || n % 32 != 0 || k % 256 != 0 || m >= kMaxM ||
        (uint64_t)k * 128 >= (1ull << 31) || (uint64_t)nv6_elem_bytes(n, k) >= (1ull << 32) || (activation_gated(activation) && (n / 2) % 32 != 0) ||
        moe_decode_slots(m, num_experts) > 65535u)
        return kErrProblemShape;
    // one descriptor bounds every 16-bit A load, and the kernel's out-of-range offset (2^31) must lie past its end; quantised input is one
    // image with 32-bit offsets.  A null index is the identity: the rows it would name must exist.
    if (a_is_quantized ? (uint64_t)qact_bytes(m, k, act_format) >= (1ull << 32)
                       : (uint64_t)a_rows * k * 2 > (1ull << 31) || (!a_row_index && a_rows < m))
        return kErrProblemShape;
    if (!c_row_index && c_rows < m)
        return kErrProblemShape;
    if (m == 0)
        return kOk;
    const void *const bias = epilogue ? epilogue->bias : nullptr;
    if (!c || !a || !images || !expert_offsets || ((uintptr_t)images & 255) || (((uintptr_t)c | (uintptr_t)a) & 15) || ((uintptr_t)bias & 7) ||
        (((uintptr_t)global_scales | (uintptr_t)expert_offsets | (uintptr_t)a_row_index | (uintptr_t)c_row_index) & 3))
        return kErrBadArgument;
    NativeMoeDecodeArgs p{};
    p.c = c, p.a = a, p.w = images, p.gs = global_scales, p.bias = bias, p.offsets = expert_offsets, p.a_idx = a_row_index, p.c_idx = c_row_index;
    p.m = m, p.n = n, p.k = k, p.act = (unsigned)activation, p.experts = num_experts, p.a_rows = a_rows, p.c_rows = c_rows;
    if (hints->a_type == kDataTypeBf16)
        native_moe_decode_launch<Bf16>(p, act_format, a_is_quantized != 0, (hipStream_t)stream);
    else
        native_moe_decode_launch<Fp16>(p, act_format, a_is_quantized != 0, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}
