// torch_binding.cpp -- the compiled torch operator layer: `torch.ops.petit_kernel.*` over the C ABI of libpetit_amd.so.
//
// The reference ships its operators as a compiled ATen extension (lib/pybind/fp4.cc:38-283, pybind.cc:8-26); this is the
// same thing for the gfx950 build, registered through torch.library (TORCH_LIBRARY) instead of pybind so that the ops
// are visible to the dispatcher (torch.compile / graph capture see them as opaque custom ops).  Same checks, same
// error texts, same output shapes and dtypes as petit_kernel/ops.py (the ctypes layer), which stays as the
// dependency-free binding; both end in the same C entry points, there is no other compute path.
// torch is used for device memory, the current stream and the per-call scratch allocation only.
//
// Built by petit-kernel_amd/build.py with the host compiler (no device code here) into lib/libpetit_torch.so.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h> // (torch-ROCm devices are "cuda" devices: the masquerading forms)
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <algorithm>
#include <string>

#include "../../include/petit_amd.h"

namespace {

constexpr int64_t kLayoutN = 16, kLayoutM = 128, kPack = 8; // fp4.cc:17-19
constexpr int kCxxFp4 = 3, kCxxFp16 = 4, kCxxBf16 = 5, kCxxMxFp4 = 7; // quantization/types.h:4-13

void *stream_of(const at::Tensor &t) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

// --- the rules more than one op states: each once, the same texts as petit_kernel/ops.py ---

void check_a16(const at::Tensor &A) {
    TORCH_CHECK(A.scalar_type() == at::kBFloat16 || A.scalar_type() == at::kHalf, "A must be bfloat16 or float16.");
}
int a_type_of(at::ScalarType t) { return t == at::kBFloat16 ? kCxxBf16 : kCxxFp16; }

// The schema's `int` (a signed int64) -> the C ABI's uint64 id.  -2 / -3 / -4 are the native-class sentinels where the caller has opted into that
// class (native_ok: a native op, or NVFP4 weights with an image attached).  Ids are 64-bit patterns whose top nibble is the K split: a split
// of 8..15 sets bit 63, and such an id arrives as its two's-complement value (petit_kernel/compiled.py maps it), far below -4096, and is
// reinterpreted; a small negative value is "library default", as in the reference (fp4.cc:189-191,240: solution_id < 0).  The native ops
// take no such ids: there every other negative value is the library default.
uint64_t c_solution_id(int64_t solution_id, bool native_ok) {
    if (native_ok && solution_id <= -2 && solution_id >= -4)
        return solution_id == -2 ? PETIT_SOLUTION_AUTO_NATIVE_MXFP8 : solution_id == -3 ? PETIT_SOLUTION_AUTO_NATIVE_MXFP4 : PETIT_SOLUTION_AUTO_NATIVE_MXFP6;
    return solution_id < 0 && (native_ok || solution_id >= -4096) ? PETIT_SOLUTION_AUTO : (uint64_t)solution_id;
}

// a GEMM entry point's refusal as the caller sees it (call it with rc != PETIT_OK: the shape text is built for the message alone)
void check_gemm_rc(int rc, const char *name, int64_t printed_id, const std::string &shape_text) {
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible problem shape (", shape_text, ")");
    TORCH_CHECK(rc != PETIT_ERROR_KERNEL_SHAPE, "No kernel implementation for solution_id=", printed_id, ".");
    TORCH_CHECK(rc == PETIT_OK, name, ": ", petit_error_string(rc));
}

// activation: 0 none, 1 silu_mul, 2 swiglu_oai (PETIT_ACTIVATION_*); halves_of: the size_n whose gate / up halves a gated form splits
void check_activation(int64_t activation, std::optional<int64_t> halves_of = std::nullopt) {
    TORCH_CHECK(activation >= 0 && activation <= 2, "activation must be 0 (none), 1 (silu_mul) or 2 (swiglu_oai)");
    if (activation && halves_of)
        TORCH_CHECK(*halves_of % 32 == 0, "silu_mul / swiglu_oai need size_n % 32 == 0 (gate / up halves of whole tiles), got ", *halves_of);
}

// the epilogue's bias: `numel` contiguous elements of `dtype` on A's device (text: the rule in the caller's words)
void check_bias(const std::optional<at::Tensor> &bias, const at::Tensor &A, at::ScalarType dtype, int64_t numel, const char *text) {
    if (bias.has_value())
        TORCH_CHECK(bias->is_cuda() && bias->device() == A.device() && bias->scalar_type() == dtype && bias->is_contiguous() && bias->numel() == numel,
                    text);
}

// what the routed-expert launches share on everything but the activations' shape: the expert count, the stacked weights (packed B / s, or
// for NVFP4 on the native class the experts' images -- unless the call is transient and brings the packed tensors), one global scale per expert,
// the E + 1 offsets
void check_expert_operands(bool mx, bool native, const at::Tensor &A, const at::Tensor &B, const at::Tensor *s, const at::Tensor &global_scales,
                           const at::Tensor &expert_offsets, int64_t E, int64_t size_n, int64_t size_k, bool transient = false) {
    TORCH_CHECK(E >= 1 && E <= PETIT_MOE_MAX_EXPERTS, "num_experts must be in 1..", PETIT_MOE_MAX_EXPERTS, ", got ", E);
    // (on the native class s is absent with images, and otherwise answers for itself below)
    TORCH_CHECK(A.is_cuda() && B.is_cuda() && global_scales.is_cuda() && expert_offsets.is_cuda() &&
                    (native ? A.is_contiguous() && B.is_contiguous() : s->is_cuda()),
                "all tensors must be on GPU");
    if (native && !mx && !transient) {
        const int64_t per = (int64_t)petit_nvfp4_native_image_bytes((unsigned)size_k, (unsigned)size_n);
        TORCH_CHECK(B.scalar_type() == at::kByte && per > 0 && B.numel() == E * per, "images do not hold num_experts native images (nvfp4_native_images)");
    } else {
        const int64_t group = mx ? 32 : 16;
        TORCH_CHECK(B.is_contiguous() && B.numel() * B.element_size() == E * size_n * size_k / 2,
                    "B does not hold num_experts * size_n * size_k packed 4-bit weights");
        TORCH_CHECK(s && s->is_cuda() && s->is_contiguous() && s->numel() * s->element_size() == E * size_n * size_k / group,
                    "s does not hold num_experts * size_n * size_k / ", group, " scales");
    }
    TORCH_CHECK(global_scales.scalar_type() == at::kFloat && global_scales.is_contiguous() && global_scales.numel() == E,
                "global_scales must be a contiguous float32 [num_experts] tensor");
    TORCH_CHECK(expert_offsets.scalar_type() == at::kInt && expert_offsets.is_contiguous() && expert_offsets.numel() == E + 1,
                "expert_offsets must be a contiguous int32 [num_experts + 1] tensor");
}

void check_row_indices(const std::optional<at::Tensor> &a_row_index, const std::optional<at::Tensor> &c_row_index, const at::Tensor &A,
                       int64_t size_m) {
    for (const auto *idx : {&a_row_index, &c_row_index})
        if (idx->has_value())
            TORCH_CHECK((*idx)->is_cuda() && (*idx)->device() == A.device() && (*idx)->scalar_type() == at::kInt && (*idx)->is_contiguous() &&
                            (*idx)->numel() == size_m,
                        "row indices must be contiguous int32 [size_m] tensors on A's device");
}
const int32_t *row_index_ptr(const std::optional<at::Tensor> &idx) { return idx.has_value() ? (const int32_t *)idx->data_ptr() : nullptr; }

// the output of a native op: 16-bit [rows, n_out], or with out_format the bytes of the quantised [size_m, n_out] rows (the real op and its Meta twin)
at::Tensor native_output(const at::Tensor &A, at::ScalarType dtype, int64_t rows, int64_t size_m, int64_t n_out, int64_t out_format) {
    if (out_format)
        return at::empty({(int64_t)petit_quantized_activation_bytes((unsigned)size_m, (unsigned)n_out, (int)out_format)}, A.options().dtype(at::kByte));
    return at::empty({rows, n_out}, A.options().dtype(dtype));
}

at::Tensor repack_nvfp4(const at::Tensor &b_q_weight, int64_t size_n, int64_t size_k) {
    TORCH_CHECK(size_k % kLayoutM == 0, "size_k = ", size_k, " is not divisible by tile_k_size = ", kLayoutM);
    TORCH_CHECK(size_n % kLayoutN == 0, "size_n = ", size_n, " is not divisible by tile_n_size = ", kLayoutN);
    TORCH_CHECK(b_q_weight.dim() == 2 && size_k / kPack == b_q_weight.size(1), "Shape mismatch: b_q_weight.size(1) = ",
                b_q_weight.size(-1), ", size_k = ", size_k, ", pack_factor = ", kPack);
    TORCH_CHECK(b_q_weight.size(0) == size_n, "b_q_weight.size(0) = ", b_q_weight.size(0), " is not size_n = ", size_n);
    TORCH_CHECK(b_q_weight.is_cuda(), "b_q_weight is not on GPU");
    TORCH_CHECK(b_q_weight.is_contiguous(), "b_q_weight is not contiguous");
    TORCH_CHECK(b_q_weight.scalar_type() == at::kInt, "b_q_weight type is not kInt");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(b_q_weight.device());
    at::Tensor out = at::empty({size_n / kLayoutN, size_k * kLayoutN / kPack}, b_q_weight.options());
    const int rc = petit_repack_nvfp4_weights((unsigned *)out.data_ptr(), (const unsigned *)b_q_weight.data_ptr(), (unsigned)size_k,
                                              (unsigned)size_n, stream_of(out));
    TORCH_CHECK(rc == PETIT_OK, "repack_nvfp4: ", petit_error_string(rc));
    return out;
}

at::Tensor process_scales(const at::Tensor &scales, int64_t size_n, int64_t size_k, bool mx) {
    const int64_t group = mx ? 32 : 16;
    TORCH_CHECK(size_k % (2 * kLayoutM) == 0, "size_k = ", size_k, " is not divisible by tile_k_size = ", 2 * kLayoutM);
    TORCH_CHECK(size_n % kLayoutN == 0, "size_n = ", size_n, " is not divisible by tile_n_size = ", kLayoutN);
    TORCH_CHECK(scales.dim() == 2 && scales.size(1) > 0 && size_k / scales.size(1) == group && size_k % scales.size(1) == 0,
                "Only groupsize = ", group, " is supported.");
    TORCH_CHECK(scales.size(0) == size_n, "scales.size(0) = ", scales.size(0), " is not size_n = ", size_n);
    TORCH_CHECK(scales.is_cuda(), "scales is not on GPU");
    TORCH_CHECK(scales.is_contiguous(), "scales is not contiguous");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(scales.device());
    at::Tensor out;
    int rc;
    if (mx) {
        TORCH_CHECK(scales.scalar_type() == at::kByte, "scales type is not uint8");
        TORCH_CHECK(size_n % 32 == 0, "size_n = ", size_n, " is not divisible by the MX scale tile (32)");
        out = at::empty({size_n / 32, size_k}, scales.options());
        rc = petit_repack_mxfp4_scales((unsigned *)out.data_ptr(), (const unsigned *)scales.data_ptr(), (unsigned)size_k, (unsigned)size_n,
                                       stream_of(out));
    } else {
        TORCH_CHECK(scales.scalar_type() == at::kFloat8_e4m3fn, "scales type is not float8_e4m3fn");
        out = at::empty({scales.size(0), scales.size(1)}, scales.options());
        rc = petit_repack_nvfp4_scales((unsigned *)out.data_ptr(), (const unsigned *)scales.data_ptr(), (unsigned)size_k, (unsigned)size_n,
                                       stream_of(out));
    }
    TORCH_CHECK(rc == PETIT_OK, mx ? "process_mxfp4_scales: " : "process_nvfp4_scales: ", petit_error_string(rc));
    return out;
}
at::Tensor process_nvfp4_scales(const at::Tensor &s, int64_t n, int64_t k) { return process_scales(s, n, k, false); }
at::Tensor process_mxfp4_scales(const at::Tensor &s, int64_t n, int64_t k) { return process_scales(s, n, k, true); }

// weight quantiser (petit_quantize_weights); the same checks and texts as petit_kernel/ops.py _quantize_operands.  b_type: kCxxFp4 / kCxxMxFp4.
// quantize_shapes states the rules once, for the real op and its Meta twin, and makes the three outputs.
struct QuantizeShapes {
    int64_t E, n, k;
    at::Tensor b, s, gs;
};
QuantizeShapes quantize_shapes(const at::Tensor &w, int64_t b_type, const std::optional<at::Tensor> &global_scale, bool real) {
    TORCH_CHECK(b_type == kCxxFp4 || b_type == kCxxMxFp4, "b_type must be 3 (NVFP4) or 7 (MXFP4)");
    const bool mx = b_type == kCxxMxFp4;
    TORCH_CHECK(w.scalar_type() == at::kBFloat16 || w.scalar_type() == at::kHalf, "w must be bfloat16 or float16.");
    TORCH_CHECK(w.dim() == 2 || w.dim() == 3, "w must be [size_n, size_k] or [num_experts, size_n, size_k]");
    if (real) {
        TORCH_CHECK(w.is_cuda(), "w is not on GPU");
        TORCH_CHECK(w.is_contiguous(), "w is not contiguous");
    }
    const int64_t E = w.dim() == 3 ? w.size(0) : 1, n = w.size(-2), k = w.size(-1);
    TORCH_CHECK(k % (2 * kLayoutM) == 0, "size_k = ", k, " is not divisible by tile_k_size = ", 2 * kLayoutM);
    TORCH_CHECK(n % kLayoutN == 0, "size_n = ", n, " is not divisible by tile_n_size = ", kLayoutN);
    TORCH_CHECK(!mx || E * n % 32 == 0, "num_experts * size_n = ", E * n, " is not divisible by the MX scale tile (32)");
    if (global_scale.has_value())
        TORCH_CHECK(global_scale->device() == w.device() && global_scale->scalar_type() == at::kFloat && global_scale->is_contiguous() &&
                        global_scale->dim() == 1 && global_scale->numel() == E,
                    "global_scale must be a contiguous float32 [num_experts] tensor on w's device");
    QuantizeShapes q{E, n, k, {}, {}, {}};
    q.b = at::empty({E * n / kLayoutN, k * kLayoutN / kPack}, w.options().dtype(at::kInt));
    q.s = mx ? at::empty({E * n / 32, k}, w.options().dtype(at::kByte)) : at::empty({E * n, k / 16}, w.options().dtype(at::kFloat8_e4m3fn));
    q.gs = at::empty({E}, w.options().dtype(at::kFloat));
    return q;
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> quantize_weights(const at::Tensor &w, int64_t b_type, const std::optional<at::Tensor> &global_scale) {
    const QuantizeShapes q = quantize_shapes(w, b_type, global_scale, true);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
    const bool supplied = b_type == kCxxFp4 && global_scale.has_value();
    const uint64_t ws_bytes = petit_quantize_weights_workspace_bytes((int)b_type, (unsigned)q.E, supplied);
    at::Tensor ws;
    if (ws_bytes)
        ws = at::empty({(int64_t)ws_bytes}, w.options().dtype(at::kByte));
    const int rc = petit_quantize_weights(w.data_ptr(), a_type_of(w.scalar_type()), (int)b_type, (unsigned)q.E, (unsigned)q.n, (unsigned)q.k,
                                          supplied ? (const float *)global_scale->data_ptr() : nullptr, q.b.data_ptr(), q.s.data_ptr(),
                                          (float *)q.gs.data_ptr(), ws_bytes ? ws.data_ptr() : nullptr, ws_bytes, stream_of(w));
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible problem shape (num_experts=", q.E, ", n=", q.n, ", k=", q.k, ")");
    TORCH_CHECK(rc == PETIT_OK, b_type == kCxxMxFp4 ? "quantize_mxfp4: " : "quantize_nvfp4: ", petit_error_string(rc));
    return {q.b, q.s, q.gs};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> quantize_weights_meta(const at::Tensor &w, int64_t b_type, const std::optional<at::Tensor> &global_scale) {
    const QuantizeShapes q = quantize_shapes(w, b_type, global_scale, false);
    return {q.b, q.s, q.gs};
}

// block-Hadamard rotation to 16 bit (petit_hadamard_rows); the same checks and texts as petit_kernel/ops.py _hadamard_operands
void hadamard_rotate_out(const at::Tensor &x, int64_t block, int64_t log2_scale, at::Tensor out) {
    TORCH_CHECK(block == 32 || block == 128, "block must be 32 or 128");
    TORCH_CHECK(log2_scale >= -126 && log2_scale <= 126, "log2_scale must be an integer in -126 .. 126");
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 1 && (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf),
                "x must be a contiguous bfloat16 / float16 GPU tensor");
    const int64_t k = x.size(-1);
    TORCH_CHECK(k % 256 == 0, "Incompatible problem shape (k=", k, "): the rotated dimension must be a multiple of 256");
    TORCH_CHECK(out.device() == x.device() && out.scalar_type() == x.scalar_type() && out.sizes() == x.sizes() && out.is_contiguous(),
                "out must be a contiguous tensor of x's shape and dtype on x's device");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    const int rc = petit_hadamard_rows(out.data_ptr(), x.data_ptr(), (unsigned)(k ? x.numel() / k : 0), (unsigned)k, a_type_of(x.scalar_type()),
                                       (unsigned)block, (int)log2_scale, stream_of(x));
    TORCH_CHECK(rc == PETIT_OK, "hadamard_rotate: ", petit_error_string(rc));
}
at::Tensor hadamard_rotate(const at::Tensor &x, int64_t block, int64_t log2_scale) {
    at::Tensor out = at::empty_like(x);
    hadamard_rotate_out(x, block, log2_scale, out);
    return out;
}
at::Tensor hadamard_rotate_meta(const at::Tensor &x, int64_t block, int64_t log2_scale) { return at::empty_like(x); }
void hadamard_rotate_out_meta(const at::Tensor &x, int64_t block, int64_t log2_scale, at::Tensor out) {}

at::Tensor mul_a16(bool mx, const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &global_scale, int64_t size_m,
                   int64_t size_n, int64_t size_k, int64_t solution_id, const std::optional<at::Tensor> &bias, int64_t activation) {
    // (check order as in the reference's MulNvFp4A16 / MulMxFp4A16, fp4.cc:163-260: the scale / weight tensor contracts first)
    if (mx) {
        TORCH_CHECK(B.dim() == 2 && B.size(0) == size_n / kLayoutN, "B.size(0) = ", B.size(0), " is not size_n / 16 = ", size_n / kLayoutN);
        TORCH_CHECK(B.size(1) == size_k * kLayoutN / kPack, "B.size(1) = ", B.size(1), " is not packed size = ", size_k * kLayoutN / kPack);
        TORCH_CHECK(s.dim() == 2 && s.size(0) == size_n / 32, "s.size(0) = ", s.size(0), " is not size_n / 32 = ", size_n / 32);
        TORCH_CHECK(s.size(1) == size_k, "s.size(1) = ", s.size(1), " is not size_k = ", size_k);
    } else {
        TORCH_CHECK(s.dim() == 2 && s.size(1) != 0 && size_k / s.size(1) == 16, "Only groupsize = 16 is supported. size_k = ", size_k,
                    ", s.size(1) = ", s.size(-1));
        TORCH_CHECK(s.numel() == size_n * size_k / 16, "s does not hold size_n * size_k / 16 scales");
    }
    check_a16(A);
    TORCH_CHECK(A.is_cuda() && B.is_cuda() && s.is_cuda() && global_scale.is_cuda(), "all tensors must be on GPU");
    TORCH_CHECK(A.is_contiguous() && A.numel() == size_m * size_k, "A must be a contiguous [size_m, size_k] tensor");
    TORCH_CHECK(B.is_contiguous() && B.numel() * B.element_size() == size_n * size_k / 2, "B does not hold size_n * size_k packed 4-bit weights");
    TORCH_CHECK(global_scale.scalar_type() == at::kFloat && global_scale.numel() >= 1, "global_scale must be float32");
    check_activation(activation, size_n);
    check_bias(bias, A, A.scalar_type(), size_n, "bias must be a contiguous [size_n] tensor of A's dtype on A's device");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    at::Tensor c = at::empty({size_m, activation ? size_n / 2 : size_n}, A.options());
    const int a_type = a_type_of(A.scalar_type());
    const petit_solution_hints hints{a_type, mx ? kCxxMxFp4 : kCxxFp4, a_type, 0};
    // -2 / -3 / -4 name the native class only on ITS entry points: these two ops are the reference's, and exact -- unless the NVFP4 weights have
    // an MFMA-native image attached (petit_nvfp4_native_attach): they have opted into the native class then
    const uint64_t sid = c_solution_id(solution_id, !mx && solution_id <= -2 && solution_id >= -4 && petit_nvfp4_native_attached(B.data_ptr()));
    const petit_epilogue epi{bias.has_value() ? bias->data_ptr() : nullptr, (int32_t)activation, 0};
    // per-call scratch from the caching allocator (stream-ordered, capture-safe): K-split slabs / native-FP4 activations
    const uint64_t ws_bytes = petit_gemm_workspace_bytes_ex(&hints, (unsigned)size_m, (unsigned)size_n, (unsigned)size_k, sid,
                                                            (bias.has_value() || activation) ? &epi : nullptr);
    at::Tensor ws;
    if (ws_bytes)
        ws = at::empty({(int64_t)ws_bytes}, A.options().dtype(at::kByte));
    auto fn = mx ? petit_gemm_mxfp4_fp16_grid_ws : petit_gemm_fp4_fp16_grid_ws;
    const int rc = fn((unsigned *)c.data_ptr(), (const unsigned *)A.data_ptr(), (const unsigned *)B.data_ptr(), (const unsigned *)s.data_ptr(),
                      (const float *)global_scale.data_ptr(), (unsigned)size_m, (unsigned)size_n, (unsigned)size_k, &hints, sid,
                      (bias.has_value() || activation) ? &epi : nullptr, ws_bytes ? ws.data_ptr() : nullptr, ws_bytes, stream_of(A));
    if (rc != PETIT_OK) // (the id as the caller spelled it: PETIT_SOLUTION_AUTO reads -1)
        check_gemm_rc(rc, mx ? "mul_mxfp4_a16" : "mul_nvfp4_a16", (int64_t)sid, c10::str("m=", size_m, ", n=", size_n, ", k=", size_k));
    return c;
}
at::Tensor mul_nvfp4_a16(const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &gs, int64_t m, int64_t n, int64_t k,
                         int64_t solution_id, const std::optional<at::Tensor> &bias, int64_t activation) {
    return mul_a16(false, A, B, s, gs, m, n, k, solution_id, bias, activation);
}
at::Tensor mul_mxfp4_a16(const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &gs, int64_t m, int64_t n, int64_t k,
                         int64_t solution_id, const std::optional<at::Tensor> &bias, int64_t activation) {
    return mul_a16(true, A, B, s, gs, m, n, k, solution_id, bias, activation);
}

// The batch-invariant GEMM family (include/petit_amd.h "Batch-invariant GEMM", "Batch-invariant MoE launch" and their two "... on the native
// class" sections).  The argument checks and their texts are stated once, in petit_kernel/ops.py (_check_invariant), which
// petit_kernel/compiled.py runs in front of these ops; what each op checks itself is what keeps a direct torch.ops call inside its tensors.
// Behind the ops is ONE routine: the output (allocated, or `out` checked), hints, epilogue, workspace tensor, the C call of the entry and the
// three checks on its return code.
struct InvariantRouting { // the MoE entries' part of a call
    const at::Tensor &off;
    int64_t e;
    const std::optional<at::Tensor> &a_idx, &c_idx;
    int64_t a_rows, c_rows;
    const at::Tensor *out;
};
// act_format: 8 / 6 / 4 on the native class (then `quantized` says what A is, and st names the 16-bit type of c and the bias), 0 on the exact.
// The native class with !mx: B is the NVFP4 native image (a MoE call: the experts' images) and s is not read (callers pass B).
at::Tensor invariant_call(const char *name, bool mx, int64_t act_format, bool quantized, at::ScalarType st, const at::Tensor &A, const at::Tensor &B,
                          const at::Tensor &s, const float *gs, int64_t m, int64_t n, int64_t k, const std::optional<at::Tensor> &bias,
                          int64_t activation, const InvariantRouting *r) {
    const bool native = act_format != 0;
    const int64_t n_out = activation ? n / 2 : n;
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    at::Tensor c;
    int64_t c_rows = m;
    if (r && r->out) {
        const at::Tensor *out = r->out;
        TORCH_CHECK(out->is_cuda() && out->device() == A.device() && out->scalar_type() == st && out->is_contiguous() && out->dim() == 2 &&
                        out->size(1) == n_out,
                    "out must be a contiguous [c_rows, n_out] tensor of A's dtype on A's device");
        TORCH_CHECK(r->c_rows < 0 || r->c_rows == out->size(0), "c_rows does not match out.size(0)");
        c = *out;
        c_rows = out->size(0);
    } else {
        c_rows = r && r->c_rows >= 0 ? r->c_rows : m;
        c = at::empty({c_rows, n_out}, A.options().dtype(st));
    }
    const int a_type = a_type_of(st), b_type = mx ? kCxxMxFp4 : kCxxFp4, fmt = (int)act_format, q = quantized ? 1 : 0;
    const unsigned um = (unsigned)m, un = (unsigned)n, uk = (unsigned)k, ue = r ? (unsigned)r->e : 0u;
    const petit_solution_hints hints{a_type, b_type, a_type, 0};
    const petit_epilogue epi{bias.has_value() ? bias->data_ptr() : nullptr, (int32_t)activation, 0};
    const petit_epilogue *const pe = (bias.has_value() || activation) ? &epi : nullptr;
    const uint64_t ws_bytes = native ? (r ? petit_gemm_native_moe_invariant_workspace_bytes(ue, um, un, uk, a_type, fmt, q)
                                          : petit_gemm_native_invariant_workspace_bytes(um, un, uk, a_type, fmt, q))
                                     : (r ? petit_gemm_moe_invariant_workspace_bytes(ue, um, un, uk, a_type, b_type)
                                          : petit_gemm_invariant_workspace_bytes(um, un, uk, a_type, b_type));
    at::Tensor ws;
    if (ws_bytes)
        ws = at::empty({(int64_t)ws_bytes}, A.options().dtype(at::kByte));
    void *const w = ws_bytes ? ws.data_ptr() : nullptr, *const stream = stream_of(A);
    int rc;
    if (!r && !native)
        rc = (mx ? petit_gemm_mxfp4_fp16_invariant : petit_gemm_fp4_fp16_invariant)(c.data_ptr(), A.data_ptr(), B.data_ptr(), s.data_ptr(), gs, um, un,
                                                                                   uk, &hints, pe, w, stream);
    else if (!r && !mx)
        rc = petit_gemm_nvfp4_native_invariant(c.data_ptr(), A.data_ptr(), B.data_ptr(), gs, um, un, uk, &hints, fmt, q, pe, w, stream);
    else if (!r)
        rc = petit_gemm_mxfp4_native_invariant(c.data_ptr(), A.data_ptr(), B.data_ptr(), s.data_ptr(), gs, um, un, uk, &hints, fmt, q, pe, w, stream);
    else if (!native)
        rc = (mx ? petit_gemm_mxfp4_fp16_moe_invariant : petit_gemm_fp4_fp16_moe_invariant)(
            c.data_ptr(), A.data_ptr(), B.data_ptr(), s.data_ptr(), gs, (const int32_t *)r->off.data_ptr(), ue, um, un, uk, row_index_ptr(r->a_idx),
            (unsigned)r->a_rows, row_index_ptr(r->c_idx), (unsigned)c_rows, &hints, pe, w, stream);
    else if (!mx)
        rc = petit_gemm_nvfp4_native_moe_invariant(c.data_ptr(), A.data_ptr(), B.data_ptr(), gs, (const int32_t *)r->off.data_ptr(), ue, um, un, uk,
                                                   row_index_ptr(r->a_idx), (unsigned)r->a_rows, row_index_ptr(r->c_idx), (unsigned)c_rows, &hints,
                                                   fmt, q, pe, w, stream);
    else
        rc = petit_gemm_mxfp4_native_moe_invariant(c.data_ptr(), A.data_ptr(), B.data_ptr(), s.data_ptr(), gs, (const int32_t *)r->off.data_ptr(), ue, um,
                                                   un, uk, row_index_ptr(r->a_idx), (unsigned)r->a_rows, row_index_ptr(r->c_idx), (unsigned)c_rows,
                                                   &hints, fmt, q, pe, w, stream);
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible problem shape (m=", m, ", n=", n, ", k=", k,
                r ? c10::str(", num_experts=", r->e, ", a_rows=", r->a_rows, ", c_rows=", c_rows) : std::string(), ")");
    TORCH_CHECK(rc != PETIT_ERROR_KERNEL_SHAPE,
                native ? "No kernel implementation for solution_id=native-invariant." : "No batch-invariant kernel for these types.");
    TORCH_CHECK(rc == PETIT_OK, name, ": ", petit_error_string(rc));
    return c;
}

#define PETIT_INVARIANT_ARGS                                                                                                                   \
    const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const std::optional<at::Tensor> &global_scale, int64_t size_m, int64_t size_n, \
        int64_t size_k, const std::optional<at::Tensor> &bias, int64_t activation
at::Tensor mul_a16_invariant(bool mx, PETIT_INVARIANT_ARGS) {
    check_a16(A);
    TORCH_CHECK(size_m >= 0 && size_n > 0 && size_k > 0 && A.is_cuda() && B.is_cuda() && s.is_cuda() && A.is_contiguous() && B.is_contiguous() &&
                    s.is_contiguous() && B.device() == A.device() && s.device() == A.device() && A.numel() == size_m * size_k &&
                    B.numel() * B.element_size() == size_n * size_k / 2 && s.numel() * s.element_size() == size_n * size_k / (mx ? 32 : 16) &&
                    (!global_scale || (global_scale->is_cuda() && global_scale->device() == A.device() &&
                                       global_scale->scalar_type() == at::kFloat && global_scale->numel() >= 1)),
                "A [size_m, size_k], packed B and s of [size_n, size_k] weights must be contiguous GPU tensors on one device, global_scale a float32 "
                "tensor on it");
    check_activation(activation, size_n);
    check_bias(bias, A, A.scalar_type(), size_n, "bias must be a contiguous [size_n] tensor of A's dtype on A's device");
    return invariant_call(mx ? "mul_mxfp4_a16_invariant" : "mul_nvfp4_a16_invariant", mx, 0, false, A.scalar_type(), A, B, s,
                          global_scale ? (const float *)global_scale->data_ptr() : nullptr, size_m, size_n, size_k, bias, activation, nullptr);
}
at::Tensor mul_nvfp4_a16_invariant(PETIT_INVARIANT_ARGS) { return mul_a16_invariant(false, A, B, s, global_scale, size_m, size_n, size_k, bias, activation); }
at::Tensor mul_mxfp4_a16_invariant(PETIT_INVARIANT_ARGS) { return mul_a16_invariant(true, A, B, s, global_scale, size_m, size_n, size_k, bias, activation); }

// on the native class A is the 16-bit matrix, or (quantized) the "petit-qact/1" bytes of act_format -- then bf16 names the 16-bit type of c
// and the bias
#define PETIT_NATIVE_INVARIANT_ARGS                                                                                                            \
    const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const std::optional<at::Tensor> &global_scale, int64_t size_m, int64_t size_n, \
        int64_t size_k, int64_t act_format, bool quantized, bool bf16, const std::optional<at::Tensor> &bias, int64_t activation
at::Tensor mul_mxfp4_native_invariant(PETIT_NATIVE_INVARIANT_ARGS) {
    const at::ScalarType st = bf16 ? at::kBFloat16 : at::kHalf;
    TORCH_CHECK(act_format == 8 || act_format == 6 || act_format == 4, "act_format must be 8, 6 or 4");
    TORCH_CHECK(size_m >= 0 && size_n > 0 && size_k > 0 && size_k % 256 == 0 && A.is_cuda() && B.is_cuda() && s.is_cuda() && A.is_contiguous() &&
                    B.is_contiguous() && s.is_contiguous() && B.device() == A.device() && s.device() == A.device() &&
                    (quantized ? A.scalar_type() == at::kByte && A.numel() == (int64_t)petit_quantized_activation_bytes((unsigned)size_m, (unsigned)size_k, (int)act_format)
                               : A.scalar_type() == st && A.numel() == size_m * size_k) &&
                    B.numel() * B.element_size() == size_n * size_k / 2 && s.numel() * s.element_size() == size_n * size_k / 32 &&
                    (!global_scale || (global_scale->is_cuda() && global_scale->device() == A.device() &&
                                       global_scale->scalar_type() == at::kFloat && global_scale->numel() >= 1)),
                "A [size_m, size_k] (or its quantised bytes), packed B and s of [size_n, size_k] weights must be contiguous GPU tensors on one "
                "device, global_scale a float32 tensor on it");
    TORCH_CHECK(activation >= 0 && activation <= 2 && (!activation || size_n % 64 == 0), "activation must be 0, 1 or 2; gated forms need size_n % 64 == 0");
    check_bias(bias, A, st, size_n, "bias must be a contiguous [size_n] tensor of A's dtype on A's device");
    return invariant_call("mul_mxfp4_native_invariant", true, act_format, quantized, st, A, B, s,
                          global_scale ? (const float *)global_scale->data_ptr() : nullptr, size_m, size_n, size_k, bias, activation, nullptr);
}

// the same on the NVFP4 native image (petit_gemm_nvfp4_native_invariant)
#define PETIT_NV_NATIVE_INVARIANT_ARGS                                                                                                         \
    const at::Tensor &A, const at::Tensor &image, const std::optional<at::Tensor> &global_scale, int64_t size_m, int64_t size_n, int64_t size_k, \
        int64_t act_format, bool quantized, bool bf16, const std::optional<at::Tensor> &bias, int64_t activation
at::Tensor mul_nvfp4_native_invariant(PETIT_NV_NATIVE_INVARIANT_ARGS) {
    const at::ScalarType st = bf16 ? at::kBFloat16 : at::kHalf;
    TORCH_CHECK(act_format == 8 || act_format == 6 || act_format == 4, "act_format must be 8, 6 or 4");
    TORCH_CHECK(size_m >= 0 && size_n > 0 && size_k > 0 && size_k % 256 == 0 && A.is_cuda() && image.is_cuda() && A.is_contiguous() &&
                    image.is_contiguous() && image.device() == A.device() &&
                    (quantized ? A.scalar_type() == at::kByte && A.numel() == (int64_t)petit_quantized_activation_bytes((unsigned)size_m, (unsigned)size_k, (int)act_format)
                               : A.scalar_type() == st && A.numel() == size_m * size_k) &&
                    image.scalar_type() == at::kByte && image.numel() > 0 &&
                    image.numel() == (int64_t)petit_nvfp4_native_image_bytes((unsigned)size_k, (unsigned)size_n) &&
                    (!global_scale || (global_scale->is_cuda() && global_scale->device() == A.device() &&
                                       global_scale->scalar_type() == at::kFloat && global_scale->numel() >= 1)),
                "A [size_m, size_k] (or its quantised bytes) and the native image of [size_n, size_k] NVFP4 weights must be contiguous GPU tensors "
                "on one device, global_scale a float32 tensor on it");
    TORCH_CHECK(activation >= 0 && activation <= 2 && (!activation || size_n % 64 == 0), "activation must be 0, 1 or 2; gated forms need size_n % 64 == 0");
    check_bias(bias, A, st, size_n, "bias must be a contiguous [size_n] tensor of A's dtype on A's device");
    return invariant_call("mul_nvfp4_native_invariant", false, act_format, quantized, st, A, image, image,
                          global_scale ? (const float *)global_scale->data_ptr() : nullptr, size_m, size_n, size_k, bias, activation, nullptr);
}

// routed-expert (MoE) launch: all experts in one call (include/petit_amd.h); the same checks and texts as petit_kernel/ops.py _mul_moe
at::Tensor mul_a16_moe(bool mx, const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &global_scales,
                       const at::Tensor &expert_offsets, int64_t size_m, int64_t size_n, int64_t size_k, int64_t num_experts, int64_t solution_id,
                       const std::optional<at::Tensor> &bias, int64_t activation) {
    const int64_t E = num_experts;
    check_a16(A);
    check_expert_operands(mx, false, A, B, &s, global_scales, expert_offsets, E, size_n, size_k);
    TORCH_CHECK(A.is_contiguous() && A.numel() == size_m * size_k, "A must be a contiguous [size_m, size_k] tensor");
    check_activation(activation, size_n);
    check_bias(bias, A, A.scalar_type(), E * size_n, "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    at::Tensor c = at::empty({size_m, activation ? size_n / 2 : size_n}, A.options());
    const int a_type = a_type_of(A.scalar_type());
    const petit_solution_hints hints{a_type, mx ? kCxxMxFp4 : kCxxFp4, a_type, 0};
    const uint64_t sid = c_solution_id(solution_id, false);
    const petit_epilogue epi{bias.has_value() ? bias->data_ptr() : nullptr, (int32_t)activation, 0};
    const int rc = petit_gemm_fp4_fp16_moe(c.data_ptr(), A.data_ptr(), B.data_ptr(), s.data_ptr(), (const float *)global_scales.data_ptr(),
                                           (const int32_t *)expert_offsets.data_ptr(), (unsigned)E, (unsigned)size_m, (unsigned)size_n,
                                           (unsigned)size_k, &hints, sid, (bias.has_value() || activation) ? &epi : nullptr, stream_of(A));
    if (rc != PETIT_OK)
        check_gemm_rc(rc, mx ? "mul_mxfp4_a16_moe" : "mul_nvfp4_a16_moe", (int64_t)sid,
                      c10::str("m=", size_m, ", n=", size_n, ", k=", size_k, ", num_experts=", E));
    return c;
}
at::Tensor mul_nvfp4_a16_moe(const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &gs, const at::Tensor &off, int64_t m,
                             int64_t n, int64_t k, int64_t e, int64_t solution_id, const std::optional<at::Tensor> &bias, int64_t activation) {
    return mul_a16_moe(false, A, B, s, gs, off, m, n, k, e, solution_id, bias, activation);
}
at::Tensor mul_mxfp4_a16_moe(const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &gs, const at::Tensor &off, int64_t m,
                             int64_t n, int64_t k, int64_t e, int64_t solution_id, const std::optional<at::Tensor> &bias, int64_t activation) {
    return mul_a16_moe(true, A, B, s, gs, off, m, n, k, e, solution_id, bias, activation);
}

// indexed MoE launch (row gather on A, row scatter on C: petit_gemm_fp4_fp16_moe_ex); the same checks and texts as petit_kernel/ops.py
// _mul_moe_indexed.  out: the _out op's destination (rows no index names stay untouched), else a new [c_rows, n_out] tensor.
at::Tensor mul_a16_moe_indexed_impl(bool mx, const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &global_scales,
                                    const at::Tensor &expert_offsets, int64_t size_m, int64_t size_n, int64_t size_k, int64_t num_experts,
                                    const std::optional<at::Tensor> &a_row_index, const std::optional<at::Tensor> &c_row_index, int64_t c_rows,
                                    int64_t solution_id, const std::optional<at::Tensor> &bias, int64_t activation, const at::Tensor *out) {
    const int64_t E = num_experts;
    check_a16(A);
    check_expert_operands(mx, false, A, B, &s, global_scales, expert_offsets, E, size_n, size_k);
    TORCH_CHECK(A.is_contiguous() && size_k > 0 && A.numel() % size_k == 0, "A must be a contiguous [a_rows, size_k] tensor");
    check_row_indices(a_row_index, c_row_index, A, size_m);
    check_activation(activation, size_n);
    check_bias(bias, A, A.scalar_type(), E * size_n, "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device");
    const int64_t a_rows = A.numel() / size_k, n_out = activation ? size_n / 2 : size_n;
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    at::Tensor c;
    if (out) {
        TORCH_CHECK(out->is_cuda() && out->device() == A.device() && out->scalar_type() == A.scalar_type() && out->is_contiguous() && out->dim() == 2 &&
                        out->size(1) == n_out,
                    "out must be a contiguous [c_rows, n_out] tensor of A's dtype on A's device");
        TORCH_CHECK(c_rows < 0 || c_rows == out->size(0), "c_rows does not match out.size(0)");
        c = *out;
        c_rows = out->size(0);
    } else {
        c_rows = c_rows < 0 ? size_m : c_rows;
        c = at::empty({c_rows, n_out}, A.options());
    }
    const int a_type = a_type_of(A.scalar_type());
    const petit_solution_hints hints{a_type, mx ? kCxxMxFp4 : kCxxFp4, a_type, 0};
    const uint64_t sid = c_solution_id(solution_id, false);
    const petit_epilogue epi{bias.has_value() ? bias->data_ptr() : nullptr, (int32_t)activation, 0};
    const int rc = petit_gemm_fp4_fp16_moe_ex(c.data_ptr(), A.data_ptr(), B.data_ptr(), s.data_ptr(), (const float *)global_scales.data_ptr(),
                                              (const int32_t *)expert_offsets.data_ptr(), (unsigned)E, (unsigned)size_m, (unsigned)size_n,
                                              (unsigned)size_k, row_index_ptr(a_row_index), (unsigned)a_rows, row_index_ptr(c_row_index),
                                              (unsigned)c_rows, &hints, sid, (bias.has_value() || activation) ? &epi : nullptr, stream_of(A));
    if (rc != PETIT_OK)
        check_gemm_rc(rc, mx ? "mul_mxfp4_a16_moe_indexed" : "mul_nvfp4_a16_moe_indexed", (int64_t)sid,
                      c10::str("m=", size_m, ", n=", size_n, ", k=", size_k, ", num_experts=", E, ", a_rows=", a_rows, ", c_rows=", c_rows));
    return c;
}
#define PETIT_MOE_INDEXED_ARGS                                                                                                                   \
    const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &gs, const at::Tensor &off, int64_t m, int64_t n, int64_t k, \
        int64_t e, const std::optional<at::Tensor> &a_idx, const std::optional<at::Tensor> &c_idx, int64_t c_rows, int64_t solution_id,         \
        const std::optional<at::Tensor> &bias, int64_t activation
at::Tensor mul_nvfp4_a16_moe_indexed(PETIT_MOE_INDEXED_ARGS) {
    return mul_a16_moe_indexed_impl(false, A, B, s, gs, off, m, n, k, e, a_idx, c_idx, c_rows, solution_id, bias, activation, nullptr);
}
at::Tensor mul_mxfp4_a16_moe_indexed(PETIT_MOE_INDEXED_ARGS) {
    return mul_a16_moe_indexed_impl(true, A, B, s, gs, off, m, n, k, e, a_idx, c_idx, c_rows, solution_id, bias, activation, nullptr);
}
void mul_nvfp4_a16_moe_indexed_out(const at::Tensor &out, PETIT_MOE_INDEXED_ARGS) {
    mul_a16_moe_indexed_impl(false, A, B, s, gs, off, m, n, k, e, a_idx, c_idx, c_rows, solution_id, bias, activation, &out);
}
void mul_mxfp4_a16_moe_indexed_out(const at::Tensor &out, PETIT_MOE_INDEXED_ARGS) {
    mul_a16_moe_indexed_impl(true, A, B, s, gs, off, m, n, k, e, a_idx, c_idx, c_rows, solution_id, bias, activation, &out);
}

// the batch-invariant MoE launch (petit_gemm_{fp4,mxfp4}_fp16_moe_invariant): the indexed launch's arguments without a solution id
#define PETIT_MOE_INVARIANT_ARGS                                                                                                                 \
    const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &gs, const at::Tensor &off, int64_t m, int64_t n, int64_t k, \
        int64_t e, const std::optional<at::Tensor> &a_idx, const std::optional<at::Tensor> &c_idx, int64_t c_rows,                               \
        const std::optional<at::Tensor> &bias, int64_t activation
at::Tensor mul_a16_moe_invariant_impl(bool mx, PETIT_MOE_INVARIANT_ARGS, const at::Tensor *out) {
    check_a16(A);
    check_expert_operands(mx, false, A, B, &s, gs, off, e, n, k);
    TORCH_CHECK(m >= 0 && A.is_contiguous() && k > 0 && A.numel() % k == 0, "A must be a contiguous [a_rows, size_k] tensor");
    check_row_indices(a_idx, c_idx, A, m);
    check_activation(activation, n);
    check_bias(bias, A, A.scalar_type(), e * n, "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device");
    const InvariantRouting r{off, e, a_idx, c_idx, A.numel() / k, c_rows, out};
    return invariant_call(mx ? "mul_mxfp4_a16_moe_invariant" : "mul_nvfp4_a16_moe_invariant", mx, 0, false, A.scalar_type(), A, B, s,
                          (const float *)gs.data_ptr(), m, n, k, bias, activation, &r);
}
#define PETIT_MOE_INVARIANT_PASS A, B, s, gs, off, m, n, k, e, a_idx, c_idx, c_rows, bias, activation
at::Tensor mul_nvfp4_a16_moe_invariant(PETIT_MOE_INVARIANT_ARGS) { return mul_a16_moe_invariant_impl(false, PETIT_MOE_INVARIANT_PASS, nullptr); }
at::Tensor mul_mxfp4_a16_moe_invariant(PETIT_MOE_INVARIANT_ARGS) { return mul_a16_moe_invariant_impl(true, PETIT_MOE_INVARIANT_PASS, nullptr); }
void mul_nvfp4_a16_moe_invariant_out(const at::Tensor &out, PETIT_MOE_INVARIANT_ARGS) { mul_a16_moe_invariant_impl(false, PETIT_MOE_INVARIANT_PASS, &out); }
void mul_mxfp4_a16_moe_invariant_out(const at::Tensor &out, PETIT_MOE_INVARIANT_ARGS) { mul_a16_moe_invariant_impl(true, PETIT_MOE_INVARIANT_PASS, &out); }

// the batch-invariant MoE launch on the native class (petit_gemm_mxfp4_native_moe_invariant).  A is the 16-bit [a_rows, k] matrix, or
// (quantized) the "petit-qact/1" bytes of the m grouped rows -- then bf16 names the 16-bit type of c and the bias
#define PETIT_NATIVE_MOE_INVARIANT_ARGS                                                                                                          \
    const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &gs, const at::Tensor &off, int64_t m, int64_t n, int64_t k, \
        int64_t e, const std::optional<at::Tensor> &a_idx, const std::optional<at::Tensor> &c_idx, int64_t c_rows, int64_t act_format,           \
        bool quantized, bool bf16, const std::optional<at::Tensor> &bias, int64_t activation
at::Tensor mul_mxfp4_native_moe_invariant(PETIT_NATIVE_MOE_INVARIANT_ARGS) {
    const at::ScalarType st = bf16 ? at::kBFloat16 : at::kHalf;
    TORCH_CHECK(act_format == 8 || act_format == 6 || act_format == 4, "act_format must be 8, 6 or 4");
    check_expert_operands(true, false, A, B, &s, gs, off, e, n, k);
    TORCH_CHECK(m >= 0 && n > 0 && k > 0 && k % 256 == 0 && A.is_contiguous() &&
                    (quantized ? A.scalar_type() == at::kByte && A.numel() == (int64_t)petit_quantized_activation_bytes((unsigned)m, (unsigned)k, (int)act_format) && !a_idx.has_value()
                               : A.scalar_type() == st && A.numel() % k == 0),
                "A must be a contiguous [a_rows, size_k] tensor, or the quantised bytes of the size_m grouped rows without an a_row_index");
    check_row_indices(a_idx, c_idx, A, m);
    TORCH_CHECK(activation >= 0 && activation <= 2 && (!activation || n % 64 == 0), "activation must be 0, 1 or 2; gated forms need size_n % 64 == 0");
    check_bias(bias, A, st, e * n, "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device");
    const InvariantRouting r{off, e, a_idx, c_idx, quantized ? m : A.numel() / k, c_rows, nullptr};
    return invariant_call("mul_mxfp4_native_moe_invariant", true, act_format, quantized, st, A, B, s, (const float *)gs.data_ptr(), m, n, k, bias,
                          activation, &r);
}

// the same on the experts' NVFP4 native images (petit_gemm_nvfp4_native_moe_invariant)
#define PETIT_NV_NATIVE_MOE_INVARIANT_ARGS                                                                                                      \
    const at::Tensor &A, const at::Tensor &images, const at::Tensor &gs, const at::Tensor &off, int64_t m, int64_t n, int64_t k, int64_t e,      \
        const std::optional<at::Tensor> &a_idx, const std::optional<at::Tensor> &c_idx, int64_t c_rows, int64_t act_format, bool quantized,     \
        bool bf16, const std::optional<at::Tensor> &bias, int64_t activation
at::Tensor mul_nvfp4_native_moe_invariant(PETIT_NV_NATIVE_MOE_INVARIANT_ARGS) {
    const at::ScalarType st = bf16 ? at::kBFloat16 : at::kHalf;
    TORCH_CHECK(act_format == 8 || act_format == 6 || act_format == 4, "act_format must be 8, 6 or 4");
    TORCH_CHECK(n > 0 && k > 0 && k % 256 == 0, "size_n and size_k must be positive, size_k % 256 == 0");
    check_expert_operands(false, true, A, images, nullptr, gs, off, e, n, k);
    TORCH_CHECK(m >= 0 && (quantized ? A.scalar_type() == at::kByte && A.numel() == (int64_t)petit_quantized_activation_bytes((unsigned)m, (unsigned)k, (int)act_format) && !a_idx.has_value()
                                     : A.scalar_type() == st && A.numel() % k == 0),
                "A must be a contiguous [a_rows, size_k] tensor, or the quantised bytes of the size_m grouped rows without an a_row_index");
    check_row_indices(a_idx, c_idx, A, m);
    TORCH_CHECK(activation >= 0 && activation <= 2 && (!activation || n % 64 == 0), "activation must be 0, 1 or 2; gated forms need size_n % 64 == 0");
    check_bias(bias, A, st, e * n, "bias must be a contiguous [num_experts, size_n] tensor of A's dtype on A's device");
    const InvariantRouting r{off, e, a_idx, c_idx, quantized ? m : A.numel() / k, c_rows, nullptr};
    return invariant_call("mul_nvfp4_native_moe_invariant", false, act_format, quantized, st, A, images, images, (const float *)gs.data_ptr(), m, n, k,
                          bias, activation, &r);
}

// device routing (petit_moe_align / petit_moe_combine); the same checks and texts as petit_kernel/ops.py
void check_topk_ids(const at::Tensor &ids, int64_t num_experts) {
    TORCH_CHECK(num_experts >= 1 && num_experts <= PETIT_MOE_MAX_EXPERTS, "num_experts must be in 1..", PETIT_MOE_MAX_EXPERTS, ", got ", num_experts);
    TORCH_CHECK(ids.is_cuda() && ids.dim() == 2 && ids.is_contiguous() && (ids.scalar_type() == at::kInt || ids.scalar_type() == at::kLong),
                "topk_ids must be a contiguous int32 / int64 [num_tokens, topk] GPU tensor");
    TORCH_CHECK(ids.size(1) >= 1, "topk must be >= 1");
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_align_device(const at::Tensor &topk_ids, int64_t num_experts) {
    check_topk_ids(topk_ids, num_experts);
    const int64_t T = topk_ids.size(0), topk = topk_ids.size(1);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(topk_ids.device());
    const auto i32 = topk_ids.options().dtype(at::kInt);
    at::Tensor sorted_pos = at::empty({T * topk}, i32), token_index = at::empty({T * topk}, i32), offsets = at::empty({num_experts + 1}, i32);
    const uint64_t ws_bytes = petit_moe_align_workspace_bytes((unsigned)T, (unsigned)topk, (unsigned)num_experts);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, topk_ids.options().dtype(at::kByte));
    const int rc = petit_moe_align(topk_ids.data_ptr(), topk_ids.scalar_type() == at::kLong, (unsigned)T, (unsigned)topk, (unsigned)num_experts,
                                   (int32_t *)offsets.data_ptr(), (int32_t *)sorted_pos.data_ptr(), (int32_t *)token_index.data_ptr(),
                                   ws_bytes ? ws.data_ptr() : nullptr, stream_of(topk_ids));
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible routing shape (num_tokens=", T, ", topk=", topk, ", num_experts=", num_experts, ")");
    TORCH_CHECK(rc == PETIT_OK, "moe_align_device: ", petit_error_string(rc));
    return {sorted_pos, offsets, token_index};
}
at::Tensor moe_combine(const at::Tensor &slot_out, const at::Tensor &topk_weights, const at::Tensor &topk_ids, int64_t num_experts) {
    check_topk_ids(topk_ids, num_experts);
    const int64_t T = topk_ids.size(0), topk = topk_ids.size(1);
    TORCH_CHECK(slot_out.is_cuda() && slot_out.device() == topk_ids.device() &&
                    (slot_out.scalar_type() == at::kBFloat16 || slot_out.scalar_type() == at::kHalf) && slot_out.is_contiguous() &&
                    slot_out.dim() == 2 && slot_out.size(0) == T * topk,
                "slot_out must be a contiguous bfloat16 / float16 [num_tokens * topk, n] tensor on topk_ids' device");
    TORCH_CHECK(topk_weights.is_cuda() && topk_weights.device() == topk_ids.device() && topk_weights.scalar_type() == at::kFloat &&
                    topk_weights.is_contiguous() && topk_weights.sizes() == topk_ids.sizes(),
                "topk_weights must be a contiguous float32 [num_tokens, topk] tensor");
    const int64_t n = slot_out.size(1);
    TORCH_CHECK(n % 8 == 0, "n must be a multiple of 8, got ", n);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(slot_out.device());
    at::Tensor out = at::empty({T, n}, slot_out.options());
    const int rc = petit_moe_combine(out.data_ptr(), slot_out.data_ptr(), (const float *)topk_weights.data_ptr(), topk_ids.data_ptr(),
                                     topk_ids.scalar_type() == at::kLong, (unsigned)T, (unsigned)topk, (unsigned)n, (unsigned)num_experts,
                                     a_type_of(slot_out.scalar_type()), stream_of(slot_out));
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible routing shape (num_tokens=", T, ", topk=", topk, ", n=", n, ", num_experts=", num_experts, ")");
    TORCH_CHECK(rc == PETIT_OK, "moe_combine: ", petit_error_string(rc));
    return out;
}

// petit_moe_combine_rmsnorm: (qa, h, y16), an absent output as an empty tensor; format 0 = no quantised output.  The checks that keep every
// access inside its tensor; petit_kernel/ops.py _combine_norm_operands states the full set, with its texts, for both Python layers
#define PETIT_COMBINE_NORM_ARGS                                                                                                            \
    const at::Tensor &slot_out, const at::Tensor &topk_weights, const at::Tensor &topk_ids, int64_t num_experts, const at::Tensor &weight, \
        double eps, int64_t format, const std::optional<at::Tensor> &residual, double weight_offset, bool return_normed, bool return_hidden, \
        bool inplace_residual
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_combine_rmsnorm(PETIT_COMBINE_NORM_ARGS) {
    check_topk_ids(topk_ids, num_experts);
    const int64_t T = topk_ids.size(0), topk = topk_ids.size(1);
    TORCH_CHECK(slot_out.is_cuda() && slot_out.device() == topk_ids.device() &&
                    (slot_out.scalar_type() == at::kBFloat16 || slot_out.scalar_type() == at::kHalf) && slot_out.is_contiguous() &&
                    slot_out.dim() == 2 && slot_out.size(0) == T * topk,
                "slot_out must be a contiguous bfloat16 / float16 [num_tokens * topk, k] tensor on topk_ids' device");
    TORCH_CHECK(topk_weights.device() == topk_ids.device() && topk_weights.scalar_type() == at::kFloat && topk_weights.is_contiguous() &&
                    topk_weights.sizes() == topk_ids.sizes(),
                "topk_weights must be a contiguous float32 [num_tokens, topk] tensor on topk_ids' device");
    const int64_t k = slot_out.size(1);
    TORCH_CHECK(format == 0 || format == 8 || format == 6 || format == 4, "fmt must be None, 'mxfp8', 'mxfp6' or 'mxfp4'");
    TORCH_CHECK(k % 8 == 0, "k must be a multiple of 8, got ", k);
    TORCH_CHECK(format == 0 || k % 256 == 0, "k must be a multiple of 256 with a fmt, got ", k);
    TORCH_CHECK(weight.device() == slot_out.device() && weight.is_contiguous() && weight.scalar_type() == slot_out.scalar_type() &&
                    weight.dim() == 1 && weight.size(0) == k,
                "weight must be a contiguous [k] tensor of slot_out's dtype on its device (k=", k, ")");
    const bool has_res = residual.has_value() && residual->defined();
    TORCH_CHECK(!has_res || (residual->device() == slot_out.device() && residual->is_contiguous() &&
                             residual->scalar_type() == slot_out.scalar_type() && residual->dim() == 2 && residual->size(0) == T &&
                             residual->size(1) == k),
                "residual must be a contiguous [num_tokens, k] tensor of slot_out's dtype on its device");
    TORCH_CHECK(format != 0 || return_normed, "fmt=None returns the 16-bit y: return_normed cannot be False");
    TORCH_CHECK(!inplace_residual || (has_res && return_hidden), "inplace_residual needs a residual and return_hidden");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(slot_out.device());
    const auto bytes = slot_out.options().dtype(at::kByte);
    at::Tensor qa = at::empty({format ? (int64_t)petit_quantized_activation_bytes((unsigned)T, (unsigned)k, (int)format) : 0}, bytes);
    at::Tensor h = return_hidden && !inplace_residual ? at::empty({T, k}, slot_out.options()) : at::empty({0}, slot_out.options());
    at::Tensor y = return_normed ? at::empty({T, k}, slot_out.options()) : at::empty({0}, slot_out.options());
    void *const h_ptr = !return_hidden ? nullptr : inplace_residual ? residual->data_ptr() : h.data_ptr();
    const int rc = petit_moe_combine_rmsnorm(format ? qa.data_ptr() : nullptr, return_normed ? y.data_ptr() : nullptr, h_ptr, slot_out.data_ptr(),
                                             (const float *)topk_weights.data_ptr(), topk_ids.data_ptr(), topk_ids.scalar_type() == at::kLong,
                                             has_res ? residual->data_ptr() : nullptr, weight.data_ptr(), (float)eps, (float)weight_offset,
                                             (unsigned)T, (unsigned)topk, (unsigned)k, (unsigned)num_experts, a_type_of(slot_out.scalar_type()),
                                             (int)format, stream_of(slot_out));
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible problem shape (num_tokens=", T, ", topk=", topk, ", k=", k, ", num_experts=", num_experts, ")");
    TORCH_CHECK(rc != PETIT_ERROR_KERNEL_SHAPE, "No kernel implementation for k=", k, " (the fused norm holds a row of at most 16384 elements).");
    TORCH_CHECK(rc == PETIT_OK, "moe_combine_rmsnorm: ", petit_error_string(rc));
    return {qa, h, y};
}

// routing from the logits (petit_moe_route / petit_moe_route_align); the same checks and texts as petit_kernel/ops.py _check_route
#define PETIT_ROUTE_ARGS                                                                                                                     \
    const at::Tensor &router_logits, int64_t topk, int64_t scoring, bool renormalize, const std::optional<at::Tensor> &bias, int64_t n_group, \
        int64_t topk_group, double routed_scaling_factor, bool return_keys
int route_logits_dtype(const at::Tensor &t) {
    return t.scalar_type() == at::kFloat ? PETIT_DTYPE_FP32 : a_type_of(t.scalar_type());
}
petit_route_desc check_route(PETIT_ROUTE_ARGS) {
    TORCH_CHECK(scoring == PETIT_ROUTE_SOFTMAX || scoring == PETIT_ROUTE_SIGMOID, "scoring must be 'softmax' or 'sigmoid'");
    TORCH_CHECK(router_logits.is_cuda() && router_logits.dim() == 2 && router_logits.is_contiguous() &&
                    (router_logits.scalar_type() == at::kFloat || router_logits.scalar_type() == at::kBFloat16 ||
                     router_logits.scalar_type() == at::kHalf),
                "router_logits must be a contiguous float32 / bfloat16 / float16 [num_tokens, num_experts] GPU tensor");
    const int64_t E = router_logits.size(1);
    TORCH_CHECK(E >= 1 && E <= PETIT_MOE_MAX_EXPERTS, "num_experts must be in 1..", PETIT_MOE_MAX_EXPERTS, ", got ", E);
    TORCH_CHECK(topk >= 1 && topk <= std::min<int64_t>(E, PETIT_MOE_MAX_TOPK), "topk must be in 1..min(num_experts, ", PETIT_MOE_MAX_TOPK, "), got ",
                topk);
    TORCH_CHECK(n_group >= 1 && topk_group >= 1, "n_group and topk_group must be >= 1");
    if (bias) {
        TORCH_CHECK(scoring == PETIT_ROUTE_SIGMOID, "bias needs scoring='sigmoid'");
        TORCH_CHECK(bias->is_cuda() && bias->device() == router_logits.device() && bias->scalar_type() == at::kFloat && bias->is_contiguous() &&
                        bias->dim() == 1 && bias->size(0) == E,
                    "bias must be a contiguous float32 [num_experts] tensor on router_logits' device");
    }
    petit_route_desc d{};
    d.scoring = (int)scoring, d.renormalize = renormalize, d.n_group = (unsigned)n_group, d.topk_group = (unsigned)topk_group;
    d.routed_scaling_factor = (float)routed_scaling_factor, d.bias = bias ? (const float *)bias->data_ptr() : nullptr;
    return d;
}
void route_rc(int rc, const char *what, int64_t T, int64_t E, int64_t topk, int64_t n_group, int64_t topk_group) {
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible routing shape (num_tokens=", T, ", num_experts=", E, ", topk=", topk, ", n_group=", n_group,
                ", topk_group=", topk_group, ")");
    TORCH_CHECK(rc == PETIT_OK, what, ": ", petit_error_string(rc));
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_route(PETIT_ROUTE_ARGS) {
    const petit_route_desc d = check_route(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys);
    const int64_t T = router_logits.size(0), E = router_logits.size(1);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(router_logits.device());
    at::Tensor ids = at::empty({T, topk}, router_logits.options().dtype(at::kInt)), w = at::empty({T, topk}, router_logits.options().dtype(at::kFloat));
    at::Tensor keys = return_keys ? at::empty({T, E}, w.options()) : at::empty({0}, w.options());
    const int rc = petit_moe_route(router_logits.data_ptr(), route_logits_dtype(router_logits), (unsigned)T, (unsigned)E, (unsigned)topk, &d,
                                   (int32_t *)ids.data_ptr(), (float *)w.data_ptr(), return_keys ? (float *)keys.data_ptr() : nullptr,
                                   stream_of(router_logits));
    route_rc(rc, "moe_route", T, E, topk, n_group, topk_group);
    return {w, ids, keys};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> moe_route_align(PETIT_ROUTE_ARGS) {
    const petit_route_desc d = check_route(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys);
    const int64_t T = router_logits.size(0), E = router_logits.size(1);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(router_logits.device());
    const auto i32 = router_logits.options().dtype(at::kInt);
    at::Tensor ids = at::empty({T, topk}, i32), w = at::empty({T, topk}, router_logits.options().dtype(at::kFloat));
    at::Tensor keys = return_keys ? at::empty({T, E}, w.options()) : at::empty({0}, w.options());
    at::Tensor sorted_pos = at::empty({T * topk}, i32), token_index = at::empty({T * topk}, i32), offsets = at::empty({E + 1}, i32);
    const uint64_t ws_bytes = petit_moe_route_align_workspace_bytes((unsigned)T, (unsigned)topk, (unsigned)E);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, router_logits.options().dtype(at::kByte));
    const int rc = petit_moe_route_align(router_logits.data_ptr(), route_logits_dtype(router_logits), (unsigned)T, (unsigned)E, (unsigned)topk, &d,
                                         (int32_t *)ids.data_ptr(), (float *)w.data_ptr(), return_keys ? (float *)keys.data_ptr() : nullptr,
                                         (int32_t *)offsets.data_ptr(), (int32_t *)sorted_pos.data_ptr(), (int32_t *)token_index.data_ptr(),
                                         ws_bytes ? ws.data_ptr() : nullptr, stream_of(router_logits));
    route_rc(rc, "moe_route_align", T, E, topk, n_group, topk_group);
    return {w, ids, sorted_pos, offsets, token_index, keys};
}

// the complete slot list (petit_moe_route_ex / petit_moe_route_align_ex); the same checks and texts as petit_kernel/ops.py _check_route_slots
#define PETIT_ROUTE_SLOTS_ARGS                                                                                                          \
    const std::optional<at::Tensor> &expert_map, int64_t num_local_experts, int64_t num_shared, double shared_weight,                    \
        const std::optional<at::Tensor> &shared_gate_logits
struct RouteSlots {
    petit_route_slots s;
    int64_t L, S;
};
RouteSlots check_route_slots(const at::Tensor &router_logits, int64_t topk, PETIT_ROUTE_SLOTS_ARGS) {
    const int64_t T = router_logits.size(0), E = router_logits.size(1), S = num_shared;
    const int64_t L = num_local_experts <= 0 ? E : num_local_experts; // (-1 or 0: num_experts, as the C ABI's 0)
    TORCH_CHECK(S >= 0 && topk + S <= PETIT_MOE_MAX_TOPK, "topk + num_shared must be in 1..", PETIT_MOE_MAX_TOPK, ", got ", topk + S);
    TORCH_CHECK(L >= 1 && L <= E && L + S <= PETIT_MOE_MAX_EXPERTS, "num_local_experts must be in 1..num_experts with num_local_experts + num_shared <= ",
                PETIT_MOE_MAX_EXPERTS, ", got ", L);
    if (!expert_map) {
        TORCH_CHECK(L == E, "num_local_experts needs an expert_map");
    } else {
        TORCH_CHECK(expert_map->is_cuda() && expert_map->device() == router_logits.device() && expert_map->scalar_type() == at::kInt &&
                        expert_map->is_contiguous() && expert_map->dim() == 1 && expert_map->size(0) == E,
                    "expert_map must be a contiguous int32 [num_experts] tensor on router_logits' device");
    }
    if (shared_gate_logits) {
        TORCH_CHECK(S >= 1, "shared_gate_logits needs num_shared >= 1");
        TORCH_CHECK(shared_gate_logits->is_cuda() && shared_gate_logits->device() == router_logits.device() &&
                        shared_gate_logits->scalar_type() == router_logits.scalar_type() && shared_gate_logits->is_contiguous() &&
                        shared_gate_logits->dim() == 2 && shared_gate_logits->size(0) == T && shared_gate_logits->size(1) == S,
                    "shared_gate_logits must be a contiguous [num_tokens, num_shared] tensor of router_logits' dtype on its device");
    }
    petit_route_slots s{};
    s.expert_map = expert_map ? (const int32_t *)expert_map->data_ptr() : nullptr;
    s.num_local_experts = (unsigned)L, s.num_shared = (unsigned)S, s.shared_weight = (float)shared_weight;
    s.shared_gate_logits = shared_gate_logits ? shared_gate_logits->data_ptr() : nullptr;
    return {s, L, S};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_route_ex(PETIT_ROUTE_ARGS, PETIT_ROUTE_SLOTS_ARGS) {
    const petit_route_desc d = check_route(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys);
    const RouteSlots sl = check_route_slots(router_logits, topk, expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits);
    const int64_t T = router_logits.size(0), E = router_logits.size(1), n_slots = topk + sl.S;
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(router_logits.device());
    at::Tensor ids = at::empty({T, n_slots}, router_logits.options().dtype(at::kInt)), w = at::empty({T, n_slots}, router_logits.options().dtype(at::kFloat));
    at::Tensor keys = return_keys ? at::empty({T, E}, w.options()) : at::empty({0}, w.options());
    const int rc = petit_moe_route_ex(router_logits.data_ptr(), route_logits_dtype(router_logits), (unsigned)T, (unsigned)E, (unsigned)topk, &d, &sl.s,
                                      (int32_t *)ids.data_ptr(), (float *)w.data_ptr(), return_keys ? (float *)keys.data_ptr() : nullptr,
                                      stream_of(router_logits));
    route_rc(rc, "moe_route_ex", T, E, topk, n_group, topk_group);
    return {w, ids, keys};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> moe_route_align_ex(PETIT_ROUTE_ARGS, PETIT_ROUTE_SLOTS_ARGS) {
    const petit_route_desc d = check_route(router_logits, topk, scoring, renormalize, bias, n_group, topk_group, routed_scaling_factor, return_keys);
    const RouteSlots sl = check_route_slots(router_logits, topk, expert_map, num_local_experts, num_shared, shared_weight, shared_gate_logits);
    const int64_t T = router_logits.size(0), E = router_logits.size(1), n_slots = topk + sl.S;
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(router_logits.device());
    const auto i32 = router_logits.options().dtype(at::kInt);
    at::Tensor ids = at::empty({T, n_slots}, i32), w = at::empty({T, n_slots}, router_logits.options().dtype(at::kFloat));
    at::Tensor keys = return_keys ? at::empty({T, E}, w.options()) : at::empty({0}, w.options());
    at::Tensor sorted_pos = at::empty({T * n_slots}, i32), token_index = at::empty({T * n_slots}, i32), offsets = at::empty({sl.L + sl.S + 1}, i32);
    const uint64_t ws_bytes = petit_moe_route_align_ex_workspace_bytes((unsigned)T, (unsigned)topk, (unsigned)E, &sl.s);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, router_logits.options().dtype(at::kByte));
    const int rc = petit_moe_route_align_ex(router_logits.data_ptr(), route_logits_dtype(router_logits), (unsigned)T, (unsigned)E, (unsigned)topk, &d, &sl.s,
                                            (int32_t *)ids.data_ptr(), (float *)w.data_ptr(), return_keys ? (float *)keys.data_ptr() : nullptr,
                                            (int32_t *)offsets.data_ptr(), (int32_t *)sorted_pos.data_ptr(), (int32_t *)token_index.data_ptr(),
                                            ws_bytes ? ws.data_ptr() : nullptr, stream_of(router_logits));
    route_rc(rc, "moe_route_align_ex", T, E, topk, n_group, topk_group);
    return {w, ids, sorted_pos, offsets, token_index, keys};
}

// the router's GEMM (petit_moe_router_logits / petit_moe_route_hidden).  The argument checks and their texts are stated once, in
// petit_kernel/ops.py (_check_router, _check_route_hidden), which petit_kernel/compiled.py runs in front of these ops; what is checked here is
// what keeps a direct torch.ops call inside its tensors.
#define PETIT_ROUTER_ARGS const at::Tensor &hidden, const at::Tensor &router_weight, const std::optional<at::Tensor> &router_bias
void check_router(PETIT_ROUTER_ARGS) {
    TORCH_CHECK(hidden.is_cuda() && hidden.dim() == 2 && hidden.is_contiguous() &&
                    (hidden.scalar_type() == at::kBFloat16 || hidden.scalar_type() == at::kHalf) && router_weight.is_cuda() &&
                    router_weight.device() == hidden.device() && router_weight.dim() == 2 && router_weight.is_contiguous() &&
                    router_weight.scalar_type() == hidden.scalar_type() && router_weight.size(1) == hidden.size(1) &&
                    (!router_bias || (router_bias->is_cuda() && router_bias->device() == hidden.device() && router_bias->is_contiguous() &&
                                      router_bias->scalar_type() == at::kFloat && router_bias->dim() == 1 &&
                                      router_bias->size(0) == router_weight.size(0))),
                "hidden [num_tokens, k] and router_weight [num_experts, k] must be contiguous bfloat16 / float16 GPU tensors of one dtype, "
                "router_bias a contiguous float32 [num_experts] tensor on their device");
}
at::Tensor moe_router_logits(PETIT_ROUTER_ARGS) {
    check_router(hidden, router_weight, router_bias);
    const int64_t T = hidden.size(0), K = hidden.size(1), E = router_weight.size(0);
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(hidden.device());
    const int a_type = a_type_of(hidden.scalar_type());
    at::Tensor logits = at::empty({T, E}, hidden.options().dtype(at::kFloat));
    const uint64_t ws_bytes = petit_moe_router_workspace_bytes((unsigned)T, (unsigned)E, (unsigned)K, a_type);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, hidden.options().dtype(at::kByte));
    const int rc = petit_moe_router_logits((float *)logits.data_ptr(), hidden.data_ptr(), router_weight.data_ptr(),
                                           router_bias ? (const float *)router_bias->data_ptr() : nullptr, a_type, (unsigned)T, (unsigned)E,
                                           (unsigned)K, ws_bytes ? ws.data_ptr() : nullptr, stream_of(hidden));
    TORCH_CHECK(rc != PETIT_ERROR_PROBLEM_SHAPE, "Incompatible router shape (num_tokens=", T, ", num_experts=", E, ", k=", K, ")");
    TORCH_CHECK(rc == PETIT_OK, "moe_router_logits: ", petit_error_string(rc));
    return logits;
}
// (the routing's arguments are PETIT_ROUTE_ARGS without the logits)
#define PETIT_ROUTE_HIDDEN_ARGS                                                                                                             \
    PETIT_ROUTER_ARGS, int64_t topk, bool align, int64_t scoring, bool renormalize, const std::optional<at::Tensor> &bias, int64_t n_group, \
        int64_t topk_group, double routed_scaling_factor, bool return_keys, PETIT_ROUTE_SLOTS_ARGS
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> moe_route_hidden(PETIT_ROUTE_HIDDEN_ARGS) {
    check_router(hidden, router_weight, router_bias);
    const int64_t T = hidden.size(0), K = hidden.size(1), E = router_weight.size(0);
    const auto f32 = hidden.options().dtype(at::kFloat);
    const auto i32 = hidden.options().dtype(at::kInt);
    TORCH_CHECK(scoring == PETIT_ROUTE_SOFTMAX || scoring == PETIT_ROUTE_SIGMOID, "scoring must be 'softmax' or 'sigmoid'");
    TORCH_CHECK(E >= 1 && E <= PETIT_MOE_MAX_EXPERTS && topk >= 1 && topk <= std::min<int64_t>(E, PETIT_MOE_MAX_TOPK) && n_group >= 1 &&
                    topk_group >= 1 && num_shared >= 0 && topk + num_shared <= PETIT_MOE_MAX_TOPK,
                "moe_route_hidden: num_experts, topk, n_group, topk_group or num_shared out of range");
    const int64_t S = num_shared, L = num_local_experts <= 0 ? E : num_local_experts, n_slots = topk + S;
    TORCH_CHECK(L <= E && L + S <= PETIT_MOE_MAX_EXPERTS && (expert_map || L == E), "moe_route_hidden: num_local_experts out of range");
    auto on_dev = [&](const at::Tensor &t, at::ScalarType st, int64_t n) {
        return t.is_cuda() && t.device() == hidden.device() && t.scalar_type() == st && t.is_contiguous() && t.numel() == n;
    };
    TORCH_CHECK((!bias || (scoring == PETIT_ROUTE_SIGMOID && on_dev(*bias, at::kFloat, E))) && (!expert_map || on_dev(*expert_map, at::kInt, E)) &&
                    (!shared_gate_logits || (S >= 1 && on_dev(*shared_gate_logits, at::kFloat, T * S))),
                "moe_route_hidden: bias float32 [num_experts] (sigmoid scoring), expert_map int32 [num_experts] and shared_gate_logits float32 "
                "[num_tokens, num_shared] must be contiguous tensors on hidden's device");
    petit_route_desc d{};
    d.scoring = (int)scoring, d.renormalize = renormalize, d.n_group = (unsigned)n_group, d.topk_group = (unsigned)topk_group;
    d.routed_scaling_factor = (float)routed_scaling_factor, d.bias = bias ? (const float *)bias->data_ptr() : nullptr;
    petit_route_slots sl{};
    sl.expert_map = expert_map ? (const int32_t *)expert_map->data_ptr() : nullptr;
    sl.num_local_experts = (unsigned)L, sl.num_shared = (unsigned)S, sl.shared_weight = (float)shared_weight;
    sl.shared_gate_logits = shared_gate_logits ? shared_gate_logits->data_ptr() : nullptr;
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(hidden.device());
    const int a_type = a_type_of(hidden.scalar_type());
    at::Tensor ids = at::empty({T, n_slots}, i32), w = at::empty({T, n_slots}, f32);
    at::Tensor keys = return_keys ? at::empty({T, E}, f32) : at::empty({0}, f32);
    const int64_t entries = align ? T * n_slots : 0;
    at::Tensor sorted_pos = at::empty({entries}, i32), token_index = at::empty({entries}, i32), offsets = at::empty({align ? L + S + 1 : 0}, i32);
    const uint64_t ws_bytes = petit_moe_route_hidden_workspace_bytes((unsigned)T, (unsigned)E, (unsigned)K, a_type, (unsigned)topk, &sl);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, hidden.options().dtype(at::kByte));
    const int rc = petit_moe_route_hidden(hidden.data_ptr(), router_weight.data_ptr(), router_bias ? (const float *)router_bias->data_ptr() : nullptr,
                                          a_type, (unsigned)T, (unsigned)E, (unsigned)K, (unsigned)topk, &d, &sl, (int32_t *)ids.data_ptr(),
                                          (float *)w.data_ptr(), return_keys ? (float *)keys.data_ptr() : nullptr,
                                          align ? (int32_t *)offsets.data_ptr() : nullptr, align ? (int32_t *)sorted_pos.data_ptr() : nullptr,
                                          align ? (int32_t *)token_index.data_ptr() : nullptr, ws_bytes ? ws.data_ptr() : nullptr, stream_of(hidden));
    route_rc(rc, "moe_route_hidden", T, E, topk, n_group, topk_group);
    return {w, ids, sorted_pos, offsets, token_index, keys};
}

// native-class MoE launch (petit_gemm_native_moe); the same checks and texts as petit_kernel/ops.py _mul_native_moe.  A: 16-bit [a_rows,
// size_k] (a_format 0), or the bytes of the size_m quantised grouped rows (a_format 8 / 6 / 4; a_type names their 16-bit dtype).  Returns
// 16-bit [c_rows, n_out], or with out_format the bytes of the quantised grouped [size_m, size_n / 2] rows.
#define PETIT_NATIVE_MOE_ARGS                                                                                                                    \
    const at::Tensor &A, const at::Tensor &B, const std::optional<at::Tensor> &s, const at::Tensor &global_scales,                                \
        const at::Tensor &expert_offsets, int64_t size_m, int64_t size_n, int64_t size_k, int64_t num_experts,                                    \
        const std::optional<at::Tensor> &a_row_index, const std::optional<at::Tensor> &c_row_index, int64_t c_rows, int64_t solution_id,         \
        const std::optional<at::Tensor> &bias, int64_t activation, int64_t a_format, int64_t a_type, int64_t out_format
at::ScalarType native_moe_dtype(const at::Tensor &A, int64_t a_format, int64_t a_type) {
    if (!a_format) {
        check_a16(A);
        return A.scalar_type();
    }
    TORCH_CHECK(A.scalar_type() == at::kByte && (a_type == kCxxBf16 || a_type == kCxxFp16), "quantised activations are uint8 bytes of a bf16 / fp16 matrix");
    return a_type == kCxxBf16 ? at::kBFloat16 : at::kHalf;
}
// transient (NVFP4): B / s are the stacked packed tensors, the images are built per call into the call's workspace (petit_gemm_native_moe_transient)
// workspace (transient only): the caller's scratch instead of one from the allocator
at::Tensor mul_native_moe_impl(bool mx, bool transient, PETIT_NATIVE_MOE_ARGS, const std::optional<at::Tensor> &workspace = std::nullopt) {
    const int64_t E = num_experts;
    const at::ScalarType dtype = native_moe_dtype(A, a_format, a_type);
    check_expert_operands(mx, true, A, B, s.has_value() ? &*s : nullptr, global_scales, expert_offsets, E, size_n, size_k, transient);
    TORCH_CHECK(size_k > 0 && (a_format || A.numel() % size_k == 0), "A must be a contiguous [a_rows, size_k] bfloat16 / float16 GPU tensor");
    if (a_format)
        TORCH_CHECK(A.numel() == (int64_t)petit_quantized_activation_bytes((unsigned)size_m, (unsigned)size_k, (int)a_format) && !a_row_index.has_value(),
                    "quantised activations are grouped rows already: a_row_index must be None");
    check_row_indices(a_row_index, c_row_index, A, size_m);
    check_activation(activation);
    TORCH_CHECK(!out_format || (activation && !c_row_index.has_value()), "out_quantized needs activation='silu_mul' or 'swiglu_oai' and no c_row_index");
    check_bias(bias, A, dtype, E * size_n, "bias must be a contiguous [num_experts, size_n] tensor of the activation dtype on the same device");
    const int64_t a_rows = a_format ? size_m : A.numel() / size_k, n_out = activation ? size_n / 2 : size_n;
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    c_rows = out_format || c_rows < 0 ? size_m : c_rows;
    at::Tensor c = native_output(A, dtype, c_rows, size_m, n_out, out_format);
    const int at_code = a_type_of(dtype);
    const petit_solution_hints hints{at_code, mx ? kCxxMxFp4 : kCxxFp4, at_code, 0};
    const uint64_t sid = c_solution_id(solution_id, true);
    const petit_epilogue epi{bias.has_value() ? bias->data_ptr() : nullptr, (int32_t)activation, 0};
    const petit_epilogue *epi_p = (bias.has_value() || activation) ? &epi : nullptr;
    const petit_native_args na{sizeof(petit_native_args), (int32_t)a_format, (int32_t)out_format, 0};
    const auto query = transient ? petit_gemm_native_moe_transient_workspace_bytes : petit_gemm_native_moe_workspace_bytes;
    const auto launch = transient ? petit_gemm_native_moe_transient : petit_gemm_native_moe;
    const uint64_t ws_bytes = query(&hints, (unsigned)E, (unsigned)size_m, (unsigned)size_n, (unsigned)size_k, sid, epi_p, &na);
    if (workspace.has_value())
        TORCH_CHECK(workspace->is_cuda() && workspace->device() == A.device() && workspace->scalar_type() == at::kByte && workspace->is_contiguous() &&
                        workspace->numel() >= (int64_t)ws_bytes,
                    "workspace must be a contiguous uint8 tensor on A's device of at least the queried bytes");
    at::Tensor ws = workspace.has_value() && ws_bytes ? *workspace : at::empty({(int64_t)ws_bytes}, A.options().dtype(at::kByte));
    const int rc = launch(c.data_ptr(), A.data_ptr(), B.data_ptr(), mx || transient ? s->data_ptr() : nullptr, (const float *)global_scales.data_ptr(),
                          (const int32_t *)expert_offsets.data_ptr(), (unsigned)E, (unsigned)size_m, (unsigned)size_n, (unsigned)size_k,
                          row_index_ptr(a_row_index), (unsigned)a_rows, row_index_ptr(c_row_index), (unsigned)c_rows, &hints, sid, epi_p, &na,
                          ws_bytes ? ws.data_ptr() : nullptr, ws_bytes, stream_of(A));
    if (rc != PETIT_OK)
        check_gemm_rc(rc, mx ? "mul_mxfp4_native_moe" : transient ? "mul_nvfp4_native_moe_transient" : "mul_nvfp4_native_moe", solution_id,
                      c10::str("m=", size_m, ", n=", size_n, ", k=", size_k, ", num_experts=", E, ", a_rows=", a_rows, ", c_rows=", c_rows));
    return c;
}
at::Tensor mul_mxfp4_native_moe(PETIT_NATIVE_MOE_ARGS) {
    return mul_native_moe_impl(true, false, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                               solution_id, bias, activation, a_format, a_type, out_format);
}
at::Tensor mul_nvfp4_native_moe(PETIT_NATIVE_MOE_ARGS) {
    return mul_native_moe_impl(false, false, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                               solution_id, bias, activation, a_format, a_type, out_format);
}
at::Tensor mul_nvfp4_native_moe_transient(PETIT_NATIVE_MOE_ARGS, const std::optional<at::Tensor> &workspace) {
    return mul_native_moe_impl(false, true, A, B, s, global_scales, expert_offsets, size_m, size_n, size_k, num_experts, a_row_index, c_row_index, c_rows,
                               solution_id, bias, activation, a_format, a_type, out_format, workspace);
}

// NVFP4 weights on the native class without a resident image (petit_gemm_nvfp4_native_transient): the same checks and texts as petit_kernel/ops.py
// mul_nvfp4_native_transient.  A: 16-bit [size_m, size_k] (a_format 0) or the bytes of quantised activations (a_format 8 / 6 / 4; a_type names their
// 16-bit dtype).  The workspace (image + the native call's scratch) comes from torch's caching allocator per call.
#define PETIT_NV_TRANSIENT_ARGS                                                                                                              \
    const at::Tensor &A, const at::Tensor &B, const at::Tensor &s, const at::Tensor &global_scale, int64_t size_m, int64_t size_n,         \
        int64_t size_k, int64_t solution_id, const std::optional<at::Tensor> &bias, int64_t activation, int64_t a_format, int64_t a_type,    \
        int64_t out_format
at::Tensor mul_nvfp4_native_transient(PETIT_NV_TRANSIENT_ARGS) {
    const at::ScalarType dtype = native_moe_dtype(A, a_format, a_type);
    TORCH_CHECK(A.is_cuda() && A.is_contiguous() && (a_format ? A.numel() == (int64_t)petit_quantized_activation_bytes((unsigned)size_m, (unsigned)size_k, (int)a_format)
                                                               : A.numel() == size_m * size_k),
                "A must be a contiguous [size_m, size_k] bfloat16 / float16 GPU tensor");
    TORCH_CHECK(B.is_cuda() && s.is_cuda() && global_scale.is_cuda(), "all tensors must be on GPU");
    TORCH_CHECK(B.is_contiguous() && B.numel() * B.element_size() == size_n * size_k / 2, "B does not hold size_n * size_k packed 4-bit weights");
    TORCH_CHECK(s.is_contiguous() && s.numel() * s.element_size() == size_n * size_k / 16, "s does not hold size_n * size_k / 16 scales");
    check_activation(activation);
    TORCH_CHECK(!out_format || activation, "out_quantized needs activation='silu_mul' or 'swiglu_oai'");
    check_bias(bias, A, dtype, size_n, "bias must be a contiguous [size_n] tensor of the activation dtype on the same device");
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    at::Tensor c = native_output(A, dtype, size_m, size_m, activation ? size_n / 2 : size_n, out_format);
    const int at_code = a_type_of(dtype);
    const petit_solution_hints hints{at_code, kCxxFp4, at_code, 0};
    const uint64_t sid = c_solution_id(solution_id, true);
    const petit_epilogue epi{bias.has_value() ? bias->data_ptr() : nullptr, (int32_t)activation, 0};
    const petit_epilogue *epi_p = (bias.has_value() || activation) ? &epi : nullptr;
    const petit_native_args na{sizeof(petit_native_args), (int32_t)a_format, (int32_t)out_format, 0};
    const uint64_t ws_bytes = petit_gemm_nvfp4_native_transient_workspace_bytes(&hints, (unsigned)size_m, (unsigned)size_n, (unsigned)size_k, sid, epi_p, &na);
    at::Tensor ws = at::empty({(int64_t)ws_bytes}, A.options().dtype(at::kByte));
    const int rc = petit_gemm_nvfp4_native_transient(c.data_ptr(), A.data_ptr(), (const unsigned *)B.data_ptr(), (const unsigned *)s.data_ptr(),
                                                     (const float *)global_scale.data_ptr(), (unsigned)size_m, (unsigned)size_n, (unsigned)size_k, &hints,
                                                     sid, epi_p, &na, ws_bytes ? ws.data_ptr() : nullptr, ws_bytes, stream_of(A));
    if (rc != PETIT_OK)
        check_gemm_rc(rc, "mul_nvfp4_native_transient", solution_id, c10::str("m=", size_m, ", n=", size_n, ", k=", size_k));
    return c;
}

// Shape functions for the Meta key (FakeTensor / torch.compile tracing, torch.export): outputs of the right shape, dtype and
// device, nothing launched -- the ops trace as opaque calls instead of breaking the graph.
at::Tensor repack_nvfp4_meta(const at::Tensor &q, int64_t n, int64_t k) { return at::empty({n / kLayoutN, k * kLayoutN / kPack}, q.options()); }
at::Tensor process_nvfp4_scales_meta(const at::Tensor &s, int64_t n, int64_t k) { return at::empty({n, k / 16}, s.options()); }
at::Tensor process_mxfp4_scales_meta(const at::Tensor &s, int64_t n, int64_t k) { return at::empty({n / 32, k}, s.options()); }
at::Tensor mul_a16_meta(const at::Tensor &A, const at::Tensor &, const at::Tensor &, const at::Tensor &, int64_t m, int64_t n, int64_t, int64_t,
                        const std::optional<at::Tensor> &, int64_t activation) {
    check_a16(A);
    return at::empty({m, activation ? n / 2 : n}, A.options());
}
at::Tensor mul_a16_invariant_meta(PETIT_INVARIANT_ARGS) {
    check_a16(A);
    return at::empty({size_m, activation ? size_n / 2 : size_n}, A.options());
}
at::Tensor mul_mxfp4_native_invariant_meta(PETIT_NATIVE_INVARIANT_ARGS) {
    return at::empty({size_m, activation ? size_n / 2 : size_n}, A.options().dtype(bf16 ? at::kBFloat16 : at::kHalf));
}
at::Tensor mul_a16_moe_meta(const at::Tensor &A, const at::Tensor &, const at::Tensor &, const at::Tensor &, const at::Tensor &, int64_t m, int64_t n,
                            int64_t, int64_t, int64_t, const std::optional<at::Tensor> &, int64_t activation) {
    check_a16(A);
    return at::empty({m, activation ? n / 2 : n}, A.options());
}

at::Tensor mul_a16_moe_indexed_meta(PETIT_MOE_INDEXED_ARGS) {
    check_a16(A);
    return at::empty({c_rows < 0 ? m : c_rows, activation ? n / 2 : n}, A.options());
}
void mul_a16_moe_indexed_out_meta(const at::Tensor &, PETIT_MOE_INDEXED_ARGS) {}
at::Tensor mul_a16_moe_invariant_meta(PETIT_MOE_INVARIANT_ARGS) {
    check_a16(A);
    return at::empty({c_rows < 0 ? m : c_rows, activation ? n / 2 : n}, A.options());
}
void mul_a16_moe_invariant_out_meta(const at::Tensor &, PETIT_MOE_INVARIANT_ARGS) {}
at::Tensor mul_mxfp4_native_moe_invariant_meta(PETIT_NATIVE_MOE_INVARIANT_ARGS) {
    return at::empty({c_rows < 0 ? m : c_rows, activation ? n / 2 : n}, A.options().dtype(bf16 ? at::kBFloat16 : at::kHalf));
}
at::Tensor mul_nvfp4_native_invariant_meta(PETIT_NV_NATIVE_INVARIANT_ARGS) {
    return at::empty({size_m, activation ? size_n / 2 : size_n}, A.options().dtype(bf16 ? at::kBFloat16 : at::kHalf));
}
at::Tensor mul_nvfp4_native_moe_invariant_meta(PETIT_NV_NATIVE_MOE_INVARIANT_ARGS) {
    return at::empty({c_rows < 0 ? m : c_rows, activation ? n / 2 : n}, A.options().dtype(bf16 ? at::kBFloat16 : at::kHalf));
}
at::Tensor mul_nvfp4_native_transient_meta(PETIT_NV_TRANSIENT_ARGS) {
    return native_output(A, native_moe_dtype(A, a_format, a_type), size_m, size_m, activation ? size_n / 2 : size_n, out_format);
}
at::Tensor mul_native_moe_meta(PETIT_NATIVE_MOE_ARGS) {
    return native_output(A, native_moe_dtype(A, a_format, a_type), c_rows < 0 ? size_m : c_rows, size_m, activation ? size_n / 2 : size_n, out_format);
}
at::Tensor mul_native_moe_transient_meta(PETIT_NATIVE_MOE_ARGS, const std::optional<at::Tensor> &) {
    return native_output(A, native_moe_dtype(A, a_format, a_type), c_rows < 0 ? size_m : c_rows, size_m, activation ? size_n / 2 : size_n, out_format);
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_align_device_meta(const at::Tensor &topk_ids, int64_t num_experts) {
    const auto i32 = topk_ids.options().dtype(at::kInt);
    const int64_t entries = topk_ids.size(0) * topk_ids.size(1);
    return {at::empty({entries}, i32), at::empty({num_experts + 1}, i32), at::empty({entries}, i32)};
}
at::Tensor moe_combine_meta(const at::Tensor &slot_out, const at::Tensor &, const at::Tensor &topk_ids, int64_t) {
    return at::empty({topk_ids.size(0), slot_out.size(1)}, slot_out.options());
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_combine_rmsnorm_meta(PETIT_COMBINE_NORM_ARGS) {
    const int64_t T = topk_ids.size(0), k = slot_out.size(1);
    const auto none = at::empty({0}, slot_out.options());
    return {at::empty({format ? (int64_t)petit_quantized_activation_bytes((unsigned)T, (unsigned)k, (int)format) : 0}, slot_out.options().dtype(at::kByte)),
            return_hidden && !inplace_residual ? at::empty({T, k}, slot_out.options()) : none, return_normed ? at::empty({T, k}, slot_out.options()) : none};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_route_meta(PETIT_ROUTE_ARGS) {
    const int64_t T = router_logits.size(0), E = router_logits.size(1);
    const auto f32 = router_logits.options().dtype(at::kFloat);
    return {at::empty({T, topk}, f32), at::empty({T, topk}, router_logits.options().dtype(at::kInt)), (return_keys ? at::empty({T, E}, f32) : at::empty({0}, f32))};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> moe_route_align_meta(PETIT_ROUTE_ARGS) {
    const int64_t T = router_logits.size(0), E = router_logits.size(1);
    const auto f32 = router_logits.options().dtype(at::kFloat);
    const auto i32 = router_logits.options().dtype(at::kInt);
    return {at::empty({T, topk}, f32), at::empty({T, topk}, i32),     at::empty({T * topk}, i32),
            at::empty({E + 1}, i32),   at::empty({T * topk}, i32), (return_keys ? at::empty({T, E}, f32) : at::empty({0}, f32))};
}
// (the slot list: topk + num_shared slots, num_local_experts + num_shared experts; num_local_experts <= 0 = num_experts)
std::tuple<at::Tensor, at::Tensor, at::Tensor> moe_route_ex_meta(PETIT_ROUTE_ARGS, PETIT_ROUTE_SLOTS_ARGS) {
    const int64_t T = router_logits.size(0), E = router_logits.size(1), n_slots = topk + num_shared;
    const auto f32 = router_logits.options().dtype(at::kFloat);
    return {at::empty({T, n_slots}, f32), at::empty({T, n_slots}, router_logits.options().dtype(at::kInt)),
            (return_keys ? at::empty({T, E}, f32) : at::empty({0}, f32))};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> moe_route_align_ex_meta(PETIT_ROUTE_ARGS, PETIT_ROUTE_SLOTS_ARGS) {
    const int64_t T = router_logits.size(0), E = router_logits.size(1), n_slots = topk + num_shared;
    const int64_t L = num_local_experts <= 0 ? E : num_local_experts;
    const auto f32 = router_logits.options().dtype(at::kFloat);
    const auto i32 = router_logits.options().dtype(at::kInt);
    return {at::empty({T, n_slots}, f32),         at::empty({T, n_slots}, i32),     at::empty({T * n_slots}, i32),
            at::empty({L + num_shared + 1}, i32), at::empty({T * n_slots}, i32), (return_keys ? at::empty({T, E}, f32) : at::empty({0}, f32))};
}
at::Tensor moe_router_logits_meta(PETIT_ROUTER_ARGS) {
    return at::empty({hidden.size(0), router_weight.size(0)}, hidden.options().dtype(at::kFloat));
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> moe_route_hidden_meta(PETIT_ROUTE_HIDDEN_ARGS) {
    const int64_t T = hidden.size(0), E = router_weight.size(0), n_slots = topk + num_shared;
    const int64_t L = num_local_experts <= 0 ? E : num_local_experts, entries = align ? T * n_slots : 0;
    const auto f32 = hidden.options().dtype(at::kFloat);
    const auto i32 = hidden.options().dtype(at::kInt);
    return {at::empty({T, n_slots}, f32),        at::empty({T, n_slots}, i32), at::empty({entries}, i32), at::empty({align ? L + num_shared + 1 : 0}, i32),
            at::empty({entries}, i32), (return_keys ? at::empty({T, E}, f32) : at::empty({0}, f32))};
}

} // namespace

// Schemas first, then one implementation per backend key.  The CPU key gets the SAME functions as the GPU key: a CPU
// tensor then reaches the checks above and gets the reference's own error text ("... is not on GPU", fp4.cc:50-52)
// instead of a dispatcher message.  (torch-ROCm devices dispatch on the CUDA key.)
TORCH_LIBRARY(petit_kernel, m) {
    m.def("repack_nvfp4(Tensor b_q_weight, int size_n, int size_k) -> Tensor");
    m.def("process_nvfp4_scales(Tensor scales, int size_n, int size_k) -> Tensor");
    m.def("process_mxfp4_scales(Tensor scales, int size_n, int size_k) -> Tensor");
    m.def("quantize_weights(Tensor w, int b_type, Tensor? global_scale=None) -> (Tensor, Tensor, Tensor)");
    m.def("hadamard_rotate(Tensor x, int block, int log2_scale=0) -> Tensor");
    m.def("hadamard_rotate_out(Tensor x, int block, int log2_scale, Tensor(a!) out) -> ()");
    m.def("mul_nvfp4_a16(Tensor A, Tensor B, Tensor s, Tensor global_scale, int size_m, int size_n, int size_k, int solution_id, "
          "Tensor? bias=None, int activation=0) -> Tensor");
    m.def("mul_mxfp4_a16(Tensor A, Tensor B, Tensor s, Tensor global_scale, int size_m, int size_n, int size_k, int solution_id, "
          "Tensor? bias=None, int activation=0) -> Tensor");
    m.def("mul_nvfp4_a16_moe(Tensor A, Tensor B, Tensor s, Tensor global_scales, Tensor expert_offsets, int size_m, int size_n, int size_k, "
          "int num_experts, int solution_id=-1, Tensor? bias=None, int activation=0) -> Tensor");
    m.def("mul_mxfp4_a16_moe(Tensor A, Tensor B, Tensor s, Tensor global_scales, Tensor expert_offsets, int size_m, int size_n, int size_k, "
          "int num_experts, int solution_id=-1, Tensor? bias=None, int activation=0) -> Tensor");
#define PETIT_MOE_INDEXED_SCHEMA                                                                                                          \
    "Tensor A, Tensor B, Tensor s, Tensor global_scales, Tensor expert_offsets, int size_m, int size_n, int size_k, int num_experts, " \
    "Tensor? a_row_index=None, Tensor? c_row_index=None, int c_rows=-1, int solution_id=-1, Tensor? bias=None, int activation=0"
    m.def("mul_nvfp4_a16_moe_indexed(" PETIT_MOE_INDEXED_SCHEMA ") -> Tensor");
    m.def("mul_mxfp4_a16_moe_indexed(" PETIT_MOE_INDEXED_SCHEMA ") -> Tensor");
    m.def("mul_nvfp4_a16_moe_indexed_out(Tensor(a!) out, " PETIT_MOE_INDEXED_SCHEMA ") -> ()");
    m.def("mul_mxfp4_a16_moe_indexed_out(Tensor(a!) out, " PETIT_MOE_INDEXED_SCHEMA ") -> ()");
#define PETIT_NATIVE_MOE_SCHEMA                                                                                                           \
    "Tensor A, Tensor B, Tensor? s, Tensor global_scales, Tensor expert_offsets, int size_m, int size_n, int size_k, int num_experts, "    \
    "Tensor? a_row_index=None, Tensor? c_row_index=None, int c_rows=-1, int solution_id=-2, Tensor? bias=None, int activation=0, "        \
    "int a_format=0, int a_type=5, int out_format=0"
    m.def("mul_mxfp4_native_moe(" PETIT_NATIVE_MOE_SCHEMA ") -> Tensor");
    m.def("mul_nvfp4_native_moe(" PETIT_NATIVE_MOE_SCHEMA ") -> Tensor");
    m.def("mul_nvfp4_native_moe_transient(" PETIT_NATIVE_MOE_SCHEMA ", Tensor? workspace=None) -> Tensor");
    m.def("mul_nvfp4_native_transient(Tensor A, Tensor B, Tensor s, Tensor global_scale, int size_m, int size_n, int size_k, int solution_id=-2, "
          "Tensor? bias=None, int activation=0, int a_format=0, int a_type=5, int out_format=0) -> Tensor");
    m.def("moe_align_device(Tensor topk_ids, int num_experts) -> (Tensor, Tensor, Tensor)");
    m.def("moe_combine(Tensor slot_out, Tensor topk_weights, Tensor topk_ids, int num_experts) -> Tensor");
    m.def("moe_combine_rmsnorm(Tensor slot_out, Tensor topk_weights, Tensor topk_ids, int num_experts, Tensor weight, float eps=1e-6, "
          "int format=0, Tensor(a!)? residual=None, float weight_offset=0.0, bool return_normed=True, bool return_hidden=False, "
          "bool inplace_residual=False) -> (Tensor, Tensor, Tensor)");
#define PETIT_ROUTE_SCHEMA                                                                                                            \
    "Tensor router_logits, int topk, int scoring=0, bool renormalize=True, Tensor? bias=None, int n_group=1, int topk_group=1, " \
    "float routed_scaling_factor=1.0, bool return_keys=False"
    m.def("moe_route(" PETIT_ROUTE_SCHEMA ") -> (Tensor, Tensor, Tensor)");
    m.def("moe_route_align(" PETIT_ROUTE_SCHEMA ") -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
#define PETIT_ROUTE_SLOTS_SCHEMA \
    ", Tensor? expert_map=None, int num_local_experts=-1, int num_shared=0, float shared_weight=1.0, Tensor? shared_gate_logits=None"
    m.def("moe_route_ex(" PETIT_ROUTE_SCHEMA PETIT_ROUTE_SLOTS_SCHEMA ") -> (Tensor, Tensor, Tensor)");
    m.def("moe_route_align_ex(" PETIT_ROUTE_SCHEMA PETIT_ROUTE_SLOTS_SCHEMA ") -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("moe_router_logits(Tensor hidden, Tensor router_weight, Tensor? router_bias=None) -> Tensor");
    m.def("moe_route_hidden(Tensor hidden, Tensor router_weight, Tensor? router_bias, int topk, bool align=True, int scoring=0, "
          "bool renormalize=True, Tensor? bias=None, int n_group=1, int topk_group=1, float routed_scaling_factor=1.0, bool return_keys=False"
          PETIT_ROUTE_SLOTS_SCHEMA ") -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("mul_nvfp4_a16_invariant(Tensor A, Tensor B, Tensor s, Tensor? global_scale, int size_m, int size_n, int size_k, Tensor? bias=None, "
          "int activation=0) -> Tensor");
    m.def("mul_mxfp4_a16_invariant(Tensor A, Tensor B, Tensor s, Tensor? global_scale, int size_m, int size_n, int size_k, Tensor? bias=None, "
          "int activation=0) -> Tensor");
#define PETIT_MOE_INVARIANT_SCHEMA                                                                                                        \
    "Tensor A, Tensor B, Tensor s, Tensor global_scales, Tensor expert_offsets, int size_m, int size_n, int size_k, int num_experts, " \
    "Tensor? a_row_index=None, Tensor? c_row_index=None, int c_rows=-1, Tensor? bias=None, int activation=0"
    m.def("mul_mxfp4_native_invariant(Tensor A, Tensor B, Tensor s, Tensor? global_scale, int size_m, int size_n, int size_k, int act_format, "
          "bool quantized, bool bf16, Tensor? bias=None, int activation=0) -> Tensor");
    m.def("mul_mxfp4_native_moe_invariant(Tensor A, Tensor B, Tensor s, Tensor global_scales, Tensor expert_offsets, int size_m, int size_n, "
          "int size_k, int num_experts, Tensor? a_row_index, Tensor? c_row_index, int c_rows, int act_format, bool quantized, bool bf16, "
          "Tensor? bias=None, int activation=0) -> Tensor");
    m.def("mul_nvfp4_native_invariant(Tensor A, Tensor image, Tensor? global_scale, int size_m, int size_n, int size_k, int act_format, "
          "bool quantized, bool bf16, Tensor? bias=None, int activation=0) -> Tensor");
    m.def("mul_nvfp4_native_moe_invariant(Tensor A, Tensor images, Tensor global_scales, Tensor expert_offsets, int size_m, int size_n, "
          "int size_k, int num_experts, Tensor? a_row_index, Tensor? c_row_index, int c_rows, int act_format, bool quantized, bool bf16, "
          "Tensor? bias=None, int activation=0) -> Tensor");
    m.def("mul_nvfp4_a16_moe_invariant(" PETIT_MOE_INVARIANT_SCHEMA ") -> Tensor");
    m.def("mul_mxfp4_a16_moe_invariant(" PETIT_MOE_INVARIANT_SCHEMA ") -> Tensor");
    m.def("mul_nvfp4_a16_moe_invariant_out(Tensor(a!) out, " PETIT_MOE_INVARIANT_SCHEMA ") -> ()");
    m.def("mul_mxfp4_a16_moe_invariant_out(Tensor(a!) out, " PETIT_MOE_INVARIANT_SCHEMA ") -> ()");
    // round 3's op name (scales promised inside fp16's range): an alias of mul_mxfp4_a16 for one more round -- the kernels test the range themselves
    m.def("mul_mxfp4_a16_f16range(Tensor A, Tensor B, Tensor s, Tensor global_scale, int size_m, int size_n, int size_k, int solution_id, "
          "Tensor? bias=None, int activation=0) -> Tensor");
}
#define PETIT_IMPL_REAL(m)                                      \
    m.impl("repack_nvfp4", &repack_nvfp4);                      \
    m.impl("process_nvfp4_scales", &process_nvfp4_scales);      \
    m.impl("process_mxfp4_scales", &process_mxfp4_scales);      \
    m.impl("quantize_weights", &quantize_weights);              \
    m.impl("hadamard_rotate", &hadamard_rotate);                \
    m.impl("hadamard_rotate_out", &hadamard_rotate_out);        \
    m.impl("mul_nvfp4_a16", &mul_nvfp4_a16);                    \
    m.impl("mul_mxfp4_a16", &mul_mxfp4_a16);                    \
    m.impl("mul_mxfp4_a16_f16range", &mul_mxfp4_a16);          \
    m.impl("mul_nvfp4_a16_invariant", &mul_nvfp4_a16_invariant); \
    m.impl("mul_mxfp4_a16_invariant", &mul_mxfp4_a16_invariant); \
    m.impl("mul_mxfp4_native_invariant", &mul_mxfp4_native_invariant); \
    m.impl("mul_nvfp4_a16_moe", &mul_nvfp4_a16_moe);            \
    m.impl("mul_mxfp4_a16_moe", &mul_mxfp4_a16_moe);            \
    m.impl("mul_nvfp4_a16_moe_indexed", &mul_nvfp4_a16_moe_indexed); \
    m.impl("mul_mxfp4_a16_moe_indexed", &mul_mxfp4_a16_moe_indexed); \
    m.impl("mul_nvfp4_a16_moe_indexed_out", &mul_nvfp4_a16_moe_indexed_out); \
    m.impl("mul_mxfp4_a16_moe_indexed_out", &mul_mxfp4_a16_moe_indexed_out); \
    m.impl("mul_mxfp4_native_moe_invariant", &mul_mxfp4_native_moe_invariant); \
    m.impl("mul_nvfp4_native_invariant", &mul_nvfp4_native_invariant); \
    m.impl("mul_nvfp4_native_moe_invariant", &mul_nvfp4_native_moe_invariant); \
    m.impl("mul_nvfp4_a16_moe_invariant", &mul_nvfp4_a16_moe_invariant); \
    m.impl("mul_mxfp4_a16_moe_invariant", &mul_mxfp4_a16_moe_invariant); \
    m.impl("mul_nvfp4_a16_moe_invariant_out", &mul_nvfp4_a16_moe_invariant_out); \
    m.impl("mul_mxfp4_a16_moe_invariant_out", &mul_mxfp4_a16_moe_invariant_out); \
    m.impl("mul_mxfp4_native_moe", &mul_mxfp4_native_moe);      \
    m.impl("mul_nvfp4_native_moe", &mul_nvfp4_native_moe);      \
    m.impl("mul_nvfp4_native_moe_transient", &mul_nvfp4_native_moe_transient); \
    m.impl("mul_nvfp4_native_transient", &mul_nvfp4_native_transient); \
    m.impl("moe_align_device", &moe_align_device);              \
    m.impl("moe_combine", &moe_combine);                        \
    m.impl("moe_combine_rmsnorm", &moe_combine_rmsnorm);        \
    m.impl("moe_route", &moe_route);                            \
    m.impl("moe_route_align", &moe_route_align);                \
    m.impl("moe_route_ex", &moe_route_ex);                      \
    m.impl("moe_route_align_ex", &moe_route_align_ex);          \
    m.impl("moe_router_logits", &moe_router_logits);            \
    m.impl("moe_route_hidden", &moe_route_hidden);
TORCH_LIBRARY_IMPL(petit_kernel, CUDA, m) { PETIT_IMPL_REAL(m) }
TORCH_LIBRARY_IMPL(petit_kernel, CPU, m) { PETIT_IMPL_REAL(m) }
TORCH_LIBRARY_IMPL(petit_kernel, Meta, m) {
    m.impl("repack_nvfp4", &repack_nvfp4_meta);
    m.impl("process_nvfp4_scales", &process_nvfp4_scales_meta);
    m.impl("process_mxfp4_scales", &process_mxfp4_scales_meta);
    m.impl("quantize_weights", &quantize_weights_meta);
    m.impl("hadamard_rotate", &hadamard_rotate_meta);
    m.impl("hadamard_rotate_out", &hadamard_rotate_out_meta);
    m.impl("mul_nvfp4_a16", &mul_a16_meta);
    m.impl("mul_mxfp4_a16", &mul_a16_meta);
    m.impl("mul_mxfp4_a16_f16range", &mul_a16_meta);
    m.impl("mul_nvfp4_a16_invariant", &mul_a16_invariant_meta);
    m.impl("mul_mxfp4_a16_invariant", &mul_a16_invariant_meta);
    m.impl("mul_mxfp4_native_invariant", &mul_mxfp4_native_invariant_meta);
    m.impl("mul_nvfp4_a16_moe", &mul_a16_moe_meta);
    m.impl("mul_mxfp4_a16_moe", &mul_a16_moe_meta);
    m.impl("mul_nvfp4_a16_moe_indexed", &mul_a16_moe_indexed_meta);
    m.impl("mul_mxfp4_a16_moe_indexed", &mul_a16_moe_indexed_meta);
    m.impl("mul_nvfp4_a16_moe_indexed_out", &mul_a16_moe_indexed_out_meta);
    m.impl("mul_mxfp4_a16_moe_indexed_out", &mul_a16_moe_indexed_out_meta);
    m.impl("mul_mxfp4_native_moe_invariant", &mul_mxfp4_native_moe_invariant_meta);
    m.impl("mul_nvfp4_native_invariant", &mul_nvfp4_native_invariant_meta);
    m.impl("mul_nvfp4_native_moe_invariant", &mul_nvfp4_native_moe_invariant_meta);
    m.impl("mul_nvfp4_a16_moe_invariant", &mul_a16_moe_invariant_meta);
    m.impl("mul_mxfp4_a16_moe_invariant", &mul_a16_moe_invariant_meta);
    m.impl("mul_nvfp4_a16_moe_invariant_out", &mul_a16_moe_invariant_out_meta);
    m.impl("mul_mxfp4_a16_moe_invariant_out", &mul_a16_moe_invariant_out_meta);
    m.impl("mul_mxfp4_native_moe", &mul_native_moe_meta);
    m.impl("mul_nvfp4_native_moe", &mul_native_moe_meta);
    m.impl("mul_nvfp4_native_moe_transient", &mul_native_moe_transient_meta);
    m.impl("mul_nvfp4_native_transient", &mul_nvfp4_native_transient_meta);
    m.impl("moe_align_device", &moe_align_device_meta);
    m.impl("moe_combine", &moe_combine_meta);
    m.impl("moe_combine_rmsnorm", &moe_combine_rmsnorm_meta);
    m.impl("moe_route", &moe_route_meta);
    m.impl("moe_route_align", &moe_route_align_meta);
    m.impl("moe_route_ex", &moe_route_ex_meta);
    m.impl("moe_route_align_ex", &moe_route_align_ex_meta);
    m.impl("moe_router_logits", &moe_router_logits_meta);
    m.impl("moe_route_hidden", &moe_route_hidden_meta);
}
