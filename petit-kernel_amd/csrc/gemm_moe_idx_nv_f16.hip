// gemm_moe_idx_nv_f16.hip -- indexed MoE forms (gathered A rows, scattered C rows: gemm_moe.hpp; moe_tu.inc): fp16 activations x NVFP4 weights.
#define PETIT_TU_AT Fp16
#define PETIT_TU_FMT kFmtNv
#define PETIT_TU_DECODE
#define PETIT_TU_MOE_FORMS moe_idx_forms_nv_f16
#define PETIT_TU_MOE_INDEXED
#include "moe_tu.inc"
