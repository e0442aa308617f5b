// gemm_native_moe_decode_f16.hip -- the routed-expert decode GEMM's kernels on the native images (gemm_native_moe_decode.hpp) for fp16 inputs,
// outputs and biases.
#include "gemm_native_moe_decode.hpp"

namespace petit_amd {
template void native_moe_decode_launch<Fp16>(const NativeMoeDecodeArgs &, int, bool, hipStream_t);
} // namespace petit_amd
