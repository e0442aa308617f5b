// gemm_moe_native_nv_bf16.hip -- routed-expert forms of the 32x32x64 native kernels (gemm_moe_native.hpp; moe_native_tu.inc): bf16 activations x NVFP4 weights (their NV6 images, back to back).
#define PETIT_TU_AT Bf16
#define PETIT_TU_WF 6
#define PETIT_TU_MOE_FORMS moe_native_forms_nv_bf16
#include "moe_native_tu.inc"
