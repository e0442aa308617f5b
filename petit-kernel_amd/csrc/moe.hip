// moe.hip -- the routed-expert (MoE) entry points of include/petit_amd.h: argument checks, the pick, the launch (the kernels: gemm_moe.hpp,
// instantiated by moe_tu.inc; the native class's: gemm_moe_native.hpp, instantiated by moe_native_tu.inc).  One pick (moe_choose) serves the launcher, its indexed form (petit_gemm_fp4_fp16_moe_ex) and
// petit_gemm_moe_resolve_solution.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "dispatch.h"

using namespace petit_amd;

namespace {

// rows one workgroup of a MoE form covers (gemm_moe.hpp: the staged / decode kernels' AM / R, the tiled and native kernels' tile rows)
unsigned moe_rows(const SolutionEntry &e) { return workgroup_tile(e.shape).moe_rows(); }
// what the MoE launchers are handed: the kernel's unsplit geometry on the whole problem
LaunchGeometry moe_geometry(const SolutionEntry &e, unsigned m, unsigned n, unsigned k) { return launch_geometry(e.shape, 1, m, n, k); }

bool moe_runs(const SolutionEntry &e, bool act, unsigned num_experts, unsigned m, unsigned k) {
    return e.launch_moe && e.shape.ks == span_tiles_for_k(k) && (!act || act_ok(e)) && moe_slots(m, moe_rows(e), num_experts) != 0;
}

// PETIT_SOLUTION_AUTO: rows per active expert r = ceil(m / min(E, m)); the dense pick for (r, n, k) when it has a MoE form and no K split,
// else the heuristic among the MoE forms (decode / staged kernels for r <= 16, on the columns of all active experts: that is the grid which
// fills the chip; tiled kernels above).  An explicit id: its entry, when that has a MoE form and split-K 1.
const SolutionEntry *moe_choose(const Family &fam, int a_type, int b_type, bool act, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                uint64_t solution_id) {
    if (solution_id != PETIT_SOLUTION_AUTO) {
        if (is_auto_id(solution_id) || solution_splitk(solution_id) != 1)
            return nullptr;
        const SolutionEntry *e = find_explicit(fam, solution_id);
        return e && moe_runs(*e, act, num_experts, m, k) ? e : nullptr;
    }
    const unsigned active = num_experts < m ? num_experts : m;
    const unsigned r = (m + active - 1) / active;
    const AutoChoice ch = choose_auto(fam, current_device(), a_type, b_type, act, r, n, k);
    if (ch.entry && ch.splitk == 1 && moe_runs(*ch.entry, act, num_experts, m, k))
        return ch.entry;
    const SolutionEntry *e = nullptr;
    if (r <= 16) {
        const uint64_t n_all = (uint64_t)n * active;
        e = heuristic(fam, r, (unsigned)(n_all < (1u << 30) ? n_all : (1u << 30)), k, act, nullptr, false, true);
    } else {
        e = heuristic(fam, m, n, k, act, nullptr, false, true);
    }
    if (e && moe_runs(*e, act, num_experts, m, k))
        return e;
    const SolutionEntry *best = nullptr; // (any MoE form that runs the problem: the most rows per workgroup fits the grid best)
    for (int i = 0; i < fam.count; ++i)
        if (moe_runs(fam.entries[i], act, num_experts, m, k) && (!best || moe_rows(fam.entries[i]) > moe_rows(*best)))
            best = &fam.entries[i];
    return best;
}

// the checks both entry points share; *fam and *act are set on success
int moe_check(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k, const petit_epilogue *epilogue,
              Family *fam, bool *act) {
    if (!hints)
        return kErrProblemShape;
    if (epilogue && (!activation_known(epilogue->activation) || epilogue->reserved != 0))
        return kErrBadArgument;
    *act = epilogue && activation_gated(epilogue->activation);
    if (hints->c_type != hints->a_type || !family_for(hints->a_type, canonical_b_type(hints->b_type), fam))
        return kErrKernelShape;
    if (num_experts == 0 || num_experts > kMoeMaxExperts)
        return kErrProblemShape;
    const bool mx = is_mx_type(hints->b_type);
    if (!shape_ok(n, k) || (mx && n % 32 != 0) || (*act && n % 32 != 0))
        return kErrProblemShape;
    if (m != 0 && !problem_in_range(m, n, k))
        return kErrProblemShape;
    return kOk;
}

// --- the native class (petit_gemm_native_moe): the routed-expert forms of the 32x32x64 native kernels (gemm_moe_native.hpp) ---------------

bool native_moe_runs(const SolutionEntry &e, bool act, unsigned num_experts, unsigned m, unsigned k) {
    return e.launch_moe_native && e.shape.ks == span_tiles_for_k(k) && (!act || act_ok(e)) && moe_slots(m, moe_rows(e), num_experts) != 0;
}

// A native sentinel: rows per active expert r = ceil(m / min(E, m)); the class's pick for (r, n, k) when it has a MoE form and no K split, else
// the class's MoE form of the span size k needs (one per class and span size: moe_native_tu.inc).  An explicit id: its entry, when that is a
// native kernel with a MoE form, split-K 1, of the class a_format names (if set).  PETIT_SOLUTION_AUTO and exact-class ids: nothing -- this
// entry point never serves another accuracy class.
const SolutionEntry *native_moe_choose(const Family &fam, int a_type, int b_type, bool act, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                       uint64_t solution_id, unsigned a_format, unsigned out_format) {
    if (solution_id == PETIT_SOLUTION_AUTO)
        return nullptr;
    const int klass = auto_class(solution_id);
    if (klass == kClassExact) {
        if (solution_splitk(solution_id) != 1)
            return nullptr;
        const SolutionEntry *e = find_explicit(fam, solution_id);
        if (!e || entry_class(*e) == kClassExact || (a_format && (unsigned)entry_class(*e) != a_format))
            return nullptr;
        return native_moe_runs(*e, act, num_experts, m, k) ? e : nullptr;
    }
    if (a_format && (unsigned)klass != a_format)
        return nullptr; // activations quantised to one format, class of another
    const unsigned active = num_experts < m ? num_experts : m;
    const unsigned r = (m + active - 1) / active;
    const unsigned restrict_ = kNeedK32 | (out_format ? kNeedQuantOut : 0u);
    const AutoChoice ch = choose_auto(fam, current_device(), a_type, b_type, act, r, n, k, klass, restrict_);
    if (ch.entry && ch.splitk == 1 && entry_class(*ch.entry) == klass && native_moe_runs(*ch.entry, act, num_experts, m, k))
        return ch.entry;
    for (int i = 0; i < fam.count; ++i)
        if (entry_class(fam.entries[i]) == klass && native_moe_runs(fam.entries[i], act, num_experts, m, k))
            return &fam.entries[i];
    return nullptr;
}

// the checks every native MoE entry point shares (and the pick): *e, *fam, *act, *a_format, *out_format set on success; m == 0 passes with *e null
int native_moe_plan(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index,
                    const int32_t *c_row_index, uint64_t solution_id, const petit_epilogue *epilogue, const petit_native_args *native,
                    const SolutionEntry **e, Family *fam, bool *act, unsigned *a_format, unsigned *out_format) {
    *e = nullptr;
    if (!native_args_ok(native))
        return kErrBadArgument;
    if (const int rc = moe_check(hints, num_experts, m, n, k, epilogue, fam, act))
        return rc;
    *a_format = native ? (unsigned)native->a_format : 0u, *out_format = native ? (unsigned)native->out_format : 0u;
    if (*a_format && a_row_index)
        return kErrBadArgument; // quantised activations are grouped rows already: nothing to gather
    if (*out_format && (!*act || c_row_index))
        return kErrBadArgument; // the quantised output is the SiLU-mul epilogue's, in the grouped order the next launch reads
    if (*out_format && n % 512 != 0)
        return kErrProblemShape; // the consumer's K = n / 2 must be a whole number of 256-column producer tiles
    if (solution_id == PETIT_SOLUTION_AUTO)
        return kErrKernelShape; // the native class's entry point: name a native sentinel or a native kernel id
    if (m == 0)
        return kOk;
    *e = native_moe_choose(*fam, hints->a_type, canonical_b_type(hints->b_type), *act, num_experts, m, n, k, solution_id, *a_format, *out_format);
    if (!*e)
        return kErrKernelShape;
    // the kernels read the quantised rows (and the quantising epilogue writes its output) through 32-bit buffer offsets; one descriptor per NV6 image
    if (petit_quantized_activation_bytes(m, k, entry_class(**e)) >= (1ull << 32) || (*out_format && petit_quantized_activation_bytes(m, n / 2, (int)*out_format) >= (1ull << 32)) ||
        (!is_mx_type(hints->b_type) && nv6_elem_bytes(n, k) >= (1ull << 32)))
        return kErrProblemShape;
    return kOk;
}

// The launch behind petit_gemm_native_moe and petit_gemm_native_moe_transient.  transient (NVFP4 only): b / scales are the stacked PACKED tensors;
// the images of the experts with rows are built into [0, E x nv6_image_bytes) of the workspace first (nv6_images on expert_offsets), the call's own
// scratch follows them, and the launch reads the workspace as its images.  Every refusal comes before the first launch.
int native_moe_run(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const int32_t *expert_offsets,
                   unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index,
                   unsigned c_rows, const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue,
                   const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream, bool transient) {
    const SolutionEntry *e;
    Family fam;
    bool act = false;
    unsigned a_format = 0, out_format = 0;
    const bool mx = hints && is_mx_type(hints->b_type);
    if (transient && mx)
        return kErrBadArgument; // MXFP4 experts need no image: petit_gemm_native_moe reads the packed tensors
    if (!c || !a || !b || ((mx || transient) && !scales) || !global_scales || !expert_offsets)
        return kErrProblemShape;
    if (const int rc = native_moe_plan(hints, num_experts, m, n, k, a_row_index, c_row_index, solution_id, epilogue, native, &e, &fam, &act, &a_format,
                                       &out_format))
        return rc;
    // a null index is the identity: the rows it would name must exist
    if ((!a_format && !a_row_index && a_rows < m) || (!out_format && !c_row_index && c_rows < m))
        return kErrProblemShape;
    // 16-byte loads and stores of A / C (and of the packed tensors a transient call converts), 256-byte aligned scratch and NV6 images (as the
    // dense native entry points)
    if (((uintptr_t)a & 15) || ((uintptr_t)c & 15) || ((uintptr_t)workspace & 255) || (!workspace && workspace_bytes) ||
        (!mx && !transient && ((uintptr_t)b & 255)) || (transient && (((uintptr_t)b & 15) || ((uintptr_t)scales & 15))))
        return kErrBadArgument;
    if (m == 0)
        return kOk;
    const int klass = entry_class(*e);
    // (the image of every accepted shape is a multiple of 256 bytes -- 6400 per 32 rows x 256 k --, so images and scratch stay aligned)
    const uint64_t images_bytes = transient ? (uint64_t)num_experts * nv6_image_bytes(n, k) : 0;
    const uint64_t need = images_bytes + (a_format ? 0 : petit_quantized_activation_bytes(m, k, klass));
    if (need && (!workspace || workspace_bytes < need))
        return kErrKernelShape; // (as the dense native entry points: scratch below the query)
    void *const scratch = (char *)workspace + images_bytes;
    if (transient) {
        if (const int rc = nv6_images(workspace, b, scales, num_experts, n, k, expert_offsets, m, (hipStream_t)stream))
            return rc;
        b = workspace;
    }
    const void *qa = a;
    if (!a_format) {
        const int rc = hints->a_type == kDataTypeBf16 ? quantize32_rows_bf16(a, a_row_index, a_rows, scratch, m, k, klass, (hipStream_t)stream)
                                                      : quantize32_rows_f16(a, a_row_index, a_rows, scratch, m, k, klass, (hipStream_t)stream);
        if (rc)
            return rc;
        qa = scratch;
    }
    MoeArgs g{};
    g.c = c, g.a = qa, g.w = b, g.s = mx ? scales : nullptr, g.gs = global_scales, g.bias = epilogue ? epilogue->bias : nullptr, g.act = act ? (unsigned)epilogue->activation : 0u;
    g.offsets = expert_offsets, g.num_experts = num_experts, g.m = m, g.n = n, g.k = k;
    g.c_idx = c_row_index, g.c_rows = c_row_index ? c_rows : m, g.out_format = out_format;
    return e->launch_moe_native(g, moe_geometry(*e, m, n, k), (hipStream_t)stream);
}

} // namespace

extern "C" {

uint64_t petit_gemm_native_moe_workspace_bytes(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                               uint64_t solution_id, const petit_epilogue *epilogue, const petit_native_args *native) {
    const SolutionEntry *e;
    Family fam;
    bool act = false;
    unsigned a_format = 0, out_format = 0;
    if (native_moe_plan(hints, num_experts, m, n, k, nullptr, nullptr, solution_id, epilogue, native, &e, &fam, &act, &a_format, &out_format) != kOk || !e)
        return 0;
    return a_format ? 0 : petit_quantized_activation_bytes(m, k, entry_class(*e));
}

uint64_t petit_gemm_native_moe_resolve_solution(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                                uint64_t solution_id, const petit_epilogue *epilogue, const petit_native_args *native) {
    const SolutionEntry *e;
    Family fam;
    bool act = false;
    unsigned a_format = 0, out_format = 0;
    if (native_moe_plan(hints, num_experts, m, n, k, nullptr, nullptr, solution_id, epilogue, native, &e, &fam, &act, &a_format, &out_format) != kOk || !e)
        return 0;
    return entry_id(fam, *e);
}

int petit_gemm_native_moe(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const int32_t *expert_offsets,
                          unsigned num_experts, unsigned m, unsigned n, unsigned k, const int32_t *a_row_index, unsigned a_rows,
                          const int32_t *c_row_index, unsigned c_rows, const petit_solution_hints *hints, uint64_t solution_id,
                          const petit_epilogue *epilogue, const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream) {
    return native_moe_run(c, a, b, scales, global_scales, expert_offsets, num_experts, m, n, k, a_row_index, a_rows, c_row_index, c_rows, hints,
                          solution_id, epilogue, native, workspace, workspace_bytes, stream, false);
}

uint64_t petit_gemm_native_moe_transient_workspace_bytes(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                                         uint64_t solution_id, const petit_epilogue *epilogue, const petit_native_args *native) {
    const SolutionEntry *e;
    Family fam;
    bool act = false;
    unsigned a_format = 0, out_format = 0;
    if (!hints || is_mx_type(hints->b_type))
        return 0;
    if (native_moe_plan(hints, num_experts, m, n, k, nullptr, nullptr, solution_id, epilogue, native, &e, &fam, &act, &a_format, &out_format) != kOk || !e)
        return 0;
    return (uint64_t)num_experts * nv6_image_bytes(n, k) + (a_format ? 0 : petit_quantized_activation_bytes(m, k, entry_class(*e)));
}

int petit_gemm_native_moe_transient(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                                    const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                    const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                                    const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue,
                                    const petit_native_args *native, void *workspace, uint64_t workspace_bytes, void *stream) {
    return native_moe_run(c, a, b, scales, global_scales, expert_offsets, num_experts, m, n, k, a_row_index, a_rows, c_row_index, c_rows, hints,
                          solution_id, epilogue, native, workspace, workspace_bytes, stream, true);
}

int petit_quantize_activations_rows(void *qa, const void *a, const int32_t *a_row_index, unsigned a_rows, unsigned m, unsigned k, int a_type,
                                    int format, void *stream) {
    if (m == 0 || k == 0)
        return kOk;
    if (!qa || !a || ((uintptr_t)qa & 15) || ((uintptr_t)a & 15))
        return kErrBadArgument;
    if (k % 256 != 0 || (!a_row_index && a_rows < m) || petit_quantized_activation_bytes(m, k, format) >= (1ull << 32))
        return kErrProblemShape;
    if (a_type == kDataTypeBf16)
        return quantize32_rows_bf16(a, a_row_index, a_rows, qa, m, k, format, (hipStream_t)stream);
    if (a_type == kDataTypeFp16)
        return quantize32_rows_f16(a, a_row_index, a_rows, qa, m, k, format, (hipStream_t)stream);
    return kErrKernelShape;
}

int petit_gemm_fp4_fp16_moe(void *c, const void *a, const void *b, const void *scales, const float *global_scales, const int32_t *expert_offsets,
                            unsigned num_experts, unsigned m, unsigned n, unsigned k, const petit_solution_hints *hints, uint64_t solution_id,
                            const petit_epilogue *epilogue, void *stream) {
    Family fam;
    bool act = false;
    if (const int rc = moe_check(hints, num_experts, m, n, k, epilogue, &fam, &act))
        return rc;
    if (!c || !a || !b || !scales || !global_scales || !expert_offsets)
        return kErrProblemShape;
    if (m == 0)
        return kOk;
    const SolutionEntry *e = moe_choose(fam, hints->a_type, canonical_b_type(hints->b_type), act, num_experts, m, n, k, solution_id);
    if (!e)
        return kErrKernelShape;
    MoeArgs g{};
    g.c = c, g.a = a, g.w = b, g.s = scales, g.gs = global_scales, g.bias = epilogue ? epilogue->bias : nullptr, g.act = act ? (unsigned)epilogue->activation : 0u;
    g.offsets = expert_offsets, g.num_experts = num_experts, g.m = m, g.n = n, g.k = k;
    return e->launch_moe(g, moe_geometry(*e, m, n, k), (hipStream_t)stream);
}

int petit_gemm_fp4_fp16_moe_ex(void *c, const void *a, const void *b, const void *scales, const float *global_scales,
                               const int32_t *expert_offsets, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                               const int32_t *a_row_index, unsigned a_rows, const int32_t *c_row_index, unsigned c_rows,
                               const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue, void *stream) {
    // a null index is the identity: the rows it would name must exist
    if ((!a_row_index && a_rows < m) || (!c_row_index && c_rows < m))
        return kErrProblemShape;
    if (!a_row_index && !c_row_index)
        return petit_gemm_fp4_fp16_moe(c, a, b, scales, global_scales, expert_offsets, num_experts, m, n, k, hints, solution_id, epilogue, stream);
    Family fam;
    bool act = false;
    if (const int rc = moe_check(hints, num_experts, m, n, k, epilogue, &fam, &act))
        return rc;
    if (!c || !a || !b || !scales || !global_scales || !expert_offsets)
        return kErrProblemShape;
    // one descriptor bounds every A load, and the kernels' out-of-range voffset (2^31) must lie past its end (device_common.hpp RowIndex)
    if ((uint64_t)a_rows * k * 2 > (1ull << 31))
        return kErrProblemShape;
    if (m == 0)
        return kOk;
    const SolutionEntry *e = moe_choose(fam, hints->a_type, canonical_b_type(hints->b_type), act, num_experts, m, n, k, solution_id);
    if (!e || !e->launch_moe_idx)
        return kErrKernelShape;
    MoeArgs g{};
    g.c = c, g.a = a, g.w = b, g.s = scales, g.gs = global_scales, g.bias = epilogue ? epilogue->bias : nullptr, g.act = act ? (unsigned)epilogue->activation : 0u;
    g.offsets = expert_offsets, g.num_experts = num_experts, g.m = m, g.n = n, g.k = k;
    g.a_idx = a_row_index, g.c_idx = c_row_index, g.a_rows = a_rows, g.c_rows = c_rows;
    return e->launch_moe_idx(g, moe_geometry(*e, m, n, k), (hipStream_t)stream);
}

uint64_t petit_gemm_moe_resolve_solution(const petit_solution_hints *hints, unsigned num_experts, unsigned m, unsigned n, unsigned k,
                                         uint64_t solution_id, const petit_epilogue *epilogue) {
    Family fam;
    bool act = false;
    if (m == 0 || moe_check(hints, num_experts, m, n, k, epilogue, &fam, &act) != kOk)
        return 0;
    const SolutionEntry *e = moe_choose(fam, hints->a_type, canonical_b_type(hints->b_type), act, num_experts, m, n, k, solution_id);
    return e ? entry_id(fam, *e) : 0;
}

} // extern "C"
