// gemm_native_decode_f16.hip -- the decode GEMM's kernels on the native image (gemm_native_decode.hpp) for fp16 inputs, outputs and biases.
#include "gemm_native_decode.hpp"

namespace petit_amd {
template void native_decode_launch<Fp16>(const NativeDecodeArgs &, int, bool, hipStream_t);
} // namespace petit_amd
