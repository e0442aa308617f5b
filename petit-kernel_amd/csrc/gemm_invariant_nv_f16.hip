// gemm_invariant_nv_f16.hip -- the batch-invariant GEMM's kernels (gemm_invariant.hpp) for one (format, type) pair: kFmtNv weights, Fp16 activations.
#include "gemm_invariant.hpp"

namespace petit_amd {
template void invariant_launch<Fp16, kFmtNv>(const InvariantArgs &, const invariant::Plan &, hipStream_t);
} // namespace petit_amd
