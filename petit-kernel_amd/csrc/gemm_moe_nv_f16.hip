// gemm_moe_nv_f16.hip -- MoE forms (all experts in one launch: gemm_moe.hpp; moe_tu.inc): fp16 activations x NVFP4 weights.
#define PETIT_TU_AT Fp16
#define PETIT_TU_FMT kFmtNv
#define PETIT_TU_DECODE
#define PETIT_TU_MOE_FORMS moe_forms_nv_f16
#include "moe_tu.inc"
