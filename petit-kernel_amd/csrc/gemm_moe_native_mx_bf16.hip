// gemm_moe_native_mx_bf16.hip -- routed-expert forms of the 32x32x64 native kernels (gemm_moe_native.hpp; moe_native_tu.inc): bf16 activations x MXFP4 weights (raw).
#define PETIT_TU_AT Bf16
#define PETIT_TU_WF 4
#define PETIT_TU_MOE_FORMS moe_native_forms_mx_bf16
#define PETIT_TU_QUANTIZE_ROWS quantize32_rows_bf16
#include "moe_native_tu.inc"
