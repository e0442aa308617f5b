// gemm_moe_mx_f16.hip -- MoE forms (all experts in one launch: gemm_moe.hpp; moe_tu.inc): fp16 activations x MXFP4 weights (Fp16Mx: fast body + exact fallback).
#define PETIT_TU_AT Fp16Mx
#define PETIT_TU_FMT kFmtMx
#define PETIT_TU_MOE_FORMS moe_forms_mx_f16
#include "moe_tu.inc"
