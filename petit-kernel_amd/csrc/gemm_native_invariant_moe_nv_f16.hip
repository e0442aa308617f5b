// gemm_native_invariant_moe_nv_f16.hip -- the native-class batch-invariant MoE GEMM's kernels on the NVFP4 image (gemm_native_invariant_moe.hpp, WF = 6) for f16 outputs and biases.
#include "gemm_native_invariant_moe.hpp"

namespace petit_amd {
template void native_invariant_moe_launch<Fp16, 6>(const NativeInvariantMoeArgs &, int, const invariant::Plan &, hipStream_t);
} // namespace petit_amd
