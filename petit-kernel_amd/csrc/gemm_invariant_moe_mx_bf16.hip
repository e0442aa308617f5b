// gemm_invariant_moe_mx_bf16.hip -- the batch-invariant MoE GEMM's kernels (gemm_invariant_moe.hpp) for one (format, type) pair: kFmtMx weights, Bf16 activations.
#include "gemm_invariant_moe.hpp"

namespace petit_amd {
template void invariant_moe_launch<Bf16, kFmtMx>(InvariantMoeArgs, const invariant::Plan &, hipStream_t);
} // namespace petit_amd
