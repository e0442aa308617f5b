// gemm_native_invariant_moe_f16.hip -- the native-class batch-invariant MoE GEMM's kernels (gemm_native_invariant_moe.hpp) for fp16 outputs and biases.
#include "gemm_native_invariant_moe.hpp"

namespace petit_amd {
template void native_invariant_moe_launch<Fp16>(const NativeInvariantMoeArgs &, int, const invariant::Plan &, hipStream_t);
} // namespace petit_amd
