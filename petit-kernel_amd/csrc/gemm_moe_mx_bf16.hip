// gemm_moe_mx_bf16.hip -- MoE forms (all experts in one launch: gemm_moe.hpp; moe_tu.inc): bf16 activations x MXFP4 weights.
#define PETIT_TU_AT Bf16
#define PETIT_TU_FMT kFmtMx
#define PETIT_TU_MOE_FORMS moe_forms_mx_bf16
#include "moe_tu.inc"
