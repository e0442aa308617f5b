// gemm_native_decode_api.hip -- the C ABI of the decode GEMM on the native image (include/petit_amd.h "Decode on the native image"): the
// choice of P, the checks, the workspace arithmetic and the launch.  The kernels are in gemm_native_decode.hpp, instantiated by
// gemm_native_decode_{bf16,f16}.hip.  Nothing here goes through dispatch.hip, pick.hip, the arch tables or the tuner, and no sentinel or
// solution id reaches these kernels.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "gemm_native_decode.hpp"
#include "hal.h"
#include "petit_internal.h"

namespace petit_amd {

extern template void native_decode_launch<Bf16>(const NativeDecodeArgs &, int, bool, hipStream_t);
extern template void native_decode_launch<Fp16>(const NativeDecodeArgs &, int, bool, hipStream_t);

namespace {

// the (n, k) an image exists for (petit_nvfp4_native_image_bytes) and the kernels' 32-bit offsets hold
bool decode_shape_ok(unsigned n, unsigned k) {
    return n != 0 && k != 0 && n % kTileN == 0 && k % 256 == 0 && (uint64_t)nv6_elem_bytes(n, k) < (1ull << 32) &&
           (uint64_t)kDecodeMaxM * k * 2 < (1ull << 32);
}

// P when the caller leaves it to the library: a function of (n, k, the CU count) alone.  Blocks of 32 weight rows that fill the chip run
// whole (P = 1); fewer are cut along K until the workgroups do, P <= 4 so that W stays 4 (W P <= 16) and every wave keeps >= kDecodeRing
// k-tiles, the depth of its ring (profiles/native_decode.md has the measurement behind the rule).
unsigned decode_auto_parts(unsigned n, unsigned k, unsigned cus) {
    const unsigned blocks = (n + 31u) / 32u, ktiles = k / kTileK;
    if (blocks >= cus)
        return 1;
    const unsigned fill = (cus + blocks - 1u) / blocks;
    const unsigned room = ktiles / (kDecodeMaxWaves * (unsigned)kDecodeRing);
    const unsigned cap = room < 4u ? (room ? room : 1u) : 4u;
    return fill < cap ? fill : cap;
}

unsigned device_cus() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return (unsigned)arch_info(dev).num_cus;
}

// P of a call (0: an explicit k_parts that is not legal)
unsigned decode_parts(unsigned n, unsigned k, unsigned k_parts) {
    const unsigned parts = k_parts ? k_parts : decode_auto_parts(n, k, device_cus());
    return decode_waves(k / kTileK, parts) ? parts : 0u;
}

uint64_t decode_workspace(unsigned m, unsigned n, unsigned parts) { return parts > 1u ? (uint64_t)parts * m * n * 4u : 0u; }

} // namespace
} // namespace petit_amd

using namespace petit_amd;

extern "C" {

unsigned petit_gemm_nvfp4_native_decode_parts(unsigned n, unsigned k) { return decode_shape_ok(n, k) ? decode_parts(n, k, 0) : 0u; }

uint64_t petit_gemm_nvfp4_native_decode_workspace_bytes(unsigned m, unsigned n, unsigned k, unsigned k_parts) {
    if (m == 0 || m > kDecodeMaxM || !decode_shape_ok(n, k))
        return 0;
    return decode_workspace(m, n, decode_parts(n, k, k_parts));
}

int petit_gemm_nvfp4_native_decode(void *c, const void *a, const void *image, const float *global_scale, unsigned m, unsigned n, unsigned k,
                                   const petit_solution_hints *hints, int act_format, int a_is_quantized, const petit_epilogue *epilogue,
                                   unsigned k_parts, void *workspace, uint64_t workspace_bytes, void *stream) {
    if (!hints || hints->c_type != hints->a_type || hints->b_type != kDataTypeFp4e2m1 || (epilogue && epilogue->reserved != 0) ||
        (hints->a_type != kDataTypeBf16 && hints->a_type != kDataTypeFp16) || (act_format != 8 && act_format != 6 && act_format != 4) ||
        (a_is_quantized != 0 && a_is_quantized != 1))
        return kErrBadArgument;
    const int activation = epilogue ? epilogue->activation : 0;
    if (!activation_known(activation))
        return kErrBadArgument;
    if (m == 0 || m > kDecodeMaxM || !decode_shape_ok(n, k) || (activation_gated(activation) && (n / 2) % 32 != 0))
        return kErrProblemShape;
    const unsigned parts = decode_parts(n, k, k_parts);
    if (parts == 0)
        return kErrBadArgument;
    const void *const bias = epilogue ? epilogue->bias : nullptr;
    if (!c || !a || !image || ((uintptr_t)image & 255) || (((uintptr_t)c | (uintptr_t)a) & 15) || ((uintptr_t)bias & 7) ||
        ((uintptr_t)global_scale & 3) || ((uintptr_t)workspace & 255) || (!workspace && workspace_bytes))
        return kErrBadArgument;
    const uint64_t need = decode_workspace(m, n, parts);
    if (need && (!workspace || workspace_bytes < need))
        return kErrKernelShape; // (as the dense native entry points: scratch below the query)
    NativeDecodeArgs p{};
    p.c = c, p.a = a, p.w = image, p.s = (const char *)image + nv6_elem_bytes(n, k), p.gs = global_scale, p.bias = bias;
    p.slabs = (float *)workspace, p.m = m, p.n = n, p.k = k, p.parts = parts, p.act = (unsigned)activation;
    if (hints->a_type == kDataTypeBf16)
        native_decode_launch<Bf16>(p, act_format, a_is_quantized != 0, (hipStream_t)stream);
    else
        native_decode_launch<Fp16>(p, act_format, a_is_quantized != 0, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

} // extern "C"
