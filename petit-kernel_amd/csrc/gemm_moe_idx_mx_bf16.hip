// gemm_moe_idx_mx_bf16.hip -- indexed MoE forms (gathered A rows, scattered C rows: gemm_moe.hpp; moe_tu.inc): bf16 activations x MXFP4 weights.
#define PETIT_TU_AT Bf16
#define PETIT_TU_FMT kFmtMx
#define PETIT_TU_MOE_FORMS moe_idx_forms_mx_bf16
#define PETIT_TU_MOE_INDEXED
#include "moe_tu.inc"
