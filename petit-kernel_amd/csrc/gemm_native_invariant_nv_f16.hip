// gemm_native_invariant_nv_f16.hip -- the native-class batch-invariant GEMM's kernels on the NVFP4 image (gemm_native_invariant.hpp, WF = 6) for f16 outputs and biases.
#include "gemm_native_invariant.hpp"

namespace petit_amd {
template void native_invariant_launch<Fp16, 6>(const NativeInvariantArgs &, int, const invariant::Plan &, hipStream_t);
} // namespace petit_amd
