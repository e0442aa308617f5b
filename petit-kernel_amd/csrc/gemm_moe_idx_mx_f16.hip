// gemm_moe_idx_mx_f16.hip -- indexed MoE forms (gathered A rows, scattered C rows: gemm_moe.hpp; moe_tu.inc): fp16 activations x MXFP4 weights (Fp16Mx: fast body + exact fallback).
#define PETIT_TU_AT Fp16Mx
#define PETIT_TU_FMT kFmtMx
#define PETIT_TU_MOE_FORMS moe_idx_forms_mx_f16
#define PETIT_TU_MOE_INDEXED
#include "moe_tu.inc"
