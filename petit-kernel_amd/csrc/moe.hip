// moe.hip -- the routed-expert (MoE) entry points of include/petit_amd.h: argument checks, the pick, the launch (the kernels: gemm_moe.hpp,
// instantiated by moe_tu.inc).  One pick (moe_choose) serves the launcher, its indexed form (petit_gemm_fp4_fp16_moe_ex) and
// petit_gemm_moe_resolve_solution.
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "dispatch.h"

using namespace petit_amd;

namespace {

// rows one workgroup of a MoE form covers (gemm_moe.hpp: the staged / decode kernels' AM / R, the tiled kernel's 16 MT)
unsigned moe_rows(const SolutionEntry &e) { return e.shape.am == kTiledAm ? 16u * (unsigned)e.shape.mt : (unsigned)am_rows(e.shape.am); }

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
    if (epilogue && ((epilogue->activation != PETIT_ACTIVATION_NONE && epilogue->activation != PETIT_ACTIVATION_SILU_MUL) || epilogue->reserved != 0))
        return kErrBadArgument;
    *act = epilogue && epilogue->activation == PETIT_ACTIVATION_SILU_MUL;
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

} // namespace

extern "C" {

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
    g.c = c, g.a = a, g.w = b, g.s = scales, g.gs = global_scales, g.bias = epilogue ? epilogue->bias : nullptr, g.act = act ? 1u : 0u;
    g.offsets = expert_offsets, g.num_experts = num_experts, g.m = m, g.n = n, g.k = k;
    return e->launch_moe(g, (hipStream_t)stream);
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
    g.c = c, g.a = a, g.w = b, g.s = scales, g.gs = global_scales, g.bias = epilogue ? epilogue->bias : nullptr, g.act = act ? 1u : 0u;
    g.offsets = expert_offsets, g.num_experts = num_experts, g.m = m, g.n = n, g.k = k;
    g.a_idx = a_row_index, g.c_idx = c_row_index, g.a_rows = a_rows, g.c_rows = c_rows;
    return e->launch_moe_idx(g, (hipStream_t)stream);
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
