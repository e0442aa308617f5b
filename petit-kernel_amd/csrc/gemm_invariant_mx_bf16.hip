// gemm_invariant_mx_bf16.hip -- the batch-invariant GEMM's kernels (gemm_invariant.hpp) for one (format, type) pair: kFmtMx weights, Bf16 activations.
#include "gemm_invariant.hpp"

namespace petit_amd {
template void invariant_launch<Bf16, kFmtMx>(const InvariantArgs &, const invariant::Plan &, hipStream_t);
} // namespace petit_amd
