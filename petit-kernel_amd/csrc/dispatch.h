// dispatch.h -- declarations shared by the host-side translation units of libpetit_amd.so (round 6: csrc/api.hip, 1 650 lines, became five):
//   solutions.hip  the family tables, ids <-> table entries, what an entry can run (its launch geometry -- tile, grid, K parts and slices -- is
//                  launch_geometry in solution.h: one function for plan_gemm, the launchers, the cost model, the picks and the tuner's candidates)
//   cost.hip       the cost model and the formula heuristic behind the arch tables
//   pick.hip       what PETIT_SOLUTION_AUTO (and the native-class sentinels) resolve to: arch table, neighbours, row split
//   dispatch.hip   scratch memory, the tuner's candidate list, plan_gemm (what a dense call runs: kernel, K split and the K slices the launch really
//                  gets, so also where SiLU-mul is applied when a named split collapses) and gemm_impl (which launches the plan)
//   api.hip        the C ABI of include/petit_amd.h;  describe.hip: petit_describe_solution / error strings
// Not installed; the public surface is include/petit_amd.h.
#pragma once

#include <atomic>
#include <cstdint>

#include "../../include/petit_amd.h"
#include "gemm_native32.hpp"
#include "gemm_stream.hpp"
#include "hal.h"
#include "layout.h"
#include "petit_internal.h"
#include "solution.h"

namespace petit_amd {

// --- solutions.hip
struct Family {
    const SolutionEntry *entries;
    int count;
    unsigned elem_b, mfma;
};
bool family_for(int a_type, int b_type, Family *out);
bool shape_ok(unsigned n, unsigned k);
bool problem_in_range(unsigned m, unsigned n, unsigned k);
bool entry_fits(const SolutionEntry &e, unsigned m, unsigned k);
unsigned entry_mfma(const Family &fam, const SolutionEntry &e);
uint64_t entry_id(const Family &fam, const SolutionEntry &e);
const SolutionEntry *find_entry(const Family &fam, uint64_t id);
const SolutionEntry *find_explicit(const Family &fam, uint64_t id);
petit_solution_hints effective_hints(const petit_solution_hints *hints);
extern std::atomic<int> g_native_enabled; // -1: $PETIT_AMD_NATIVE_FP4 not read yet
bool native_enabled();
// the accuracy classes: exact, or the native block-scaled MFMA with activations quantised to MXFP8 / MXFP6 / MXFP4
enum : int { kClassExact = 0, kClassNativeFp8 = 8, kClassNativeFp6 = 6, kClassNativeFp4 = 4 };
int entry_class(const SolutionEntry &e);
enum : unsigned { kNeedK32 = 1u, kNeedQuantOut = 2u }; // restrictions of the native pipeline (entry_allows)
bool entry_allows(const SolutionEntry &e, unsigned restrict_);
inline bool is_shared(const SolutionEntry &e) { return shape_is_shared(e.shape); } // gemm_shared.hpp (plain / bias epilogue only)
inline bool is_batch(const SolutionEntry &e) { return shape_is_batch(e.shape); }   // gemm_batch.hpp (17 <= M <= 128; reaches the default path through the arch table)
// SiLU-mul epilogue: a wave must hold the gate and the up tile of an output tile -> even n-tiles per wave
inline bool act_ok(const SolutionEntry &e) { return e.shape.nt % 2 == 0 && !is_shared(e); }
bool act_runs(const SolutionEntry &e, unsigned splitk, unsigned restrict_ = 0);
// petit_native_args as the native entry points take it (null: 16-bit in and out)
inline bool native_args_ok(const petit_native_args *na) {
    return !na || (na->struct_bytes == sizeof(petit_native_args) && na->reserved == 0 &&
                   (na->a_format == 0 || na->a_format == 8 || na->a_format == 6 || na->a_format == 4) &&
                   (na->out_format == 0 || na->out_format == 8 || na->out_format == 6 || na->out_format == 4));
}
uint64_t operand_bytes(const SolutionEntry &e, unsigned m, unsigned n, unsigned k);

// --- cost.hip
struct StepCost {
    int a_type, fmt, kind, tile_m, nt, d, pf, kg;
    float t1, resident, err;
};
const StepCost *step_cost(const SolutionEntry &e);
unsigned guarded_splitk(const SolutionEntry &e, unsigned splitk, unsigned m, unsigned n, unsigned k, int num_cus);
double stream_cost_us(const SolutionEntry &e, unsigned m, unsigned n, unsigned k, int num_cus);
double tiled_cost_us(const SolutionEntry &e, unsigned m, unsigned n, unsigned k, int num_cus, unsigned splitk = 1);
const SolutionEntry *heuristic(const Family &fam, unsigned m, unsigned n, unsigned k, bool need_pairs = false, unsigned *splitk_out = nullptr,
                               bool need_grouped = false, bool need_moe = false);

// --- pick.hip
const SolutionEntry *heuristic_native(const Family &fam, int klass, unsigned m, unsigned n, unsigned k, bool need_pairs, bool have_slabs,
                                      unsigned *splitk_out, unsigned restrict_ = 0);
struct AutoChoice {
    const SolutionEntry *entry;
    unsigned splitk;
};
double grid_overhead(const SolutionEntry &e, unsigned splitk, unsigned m, unsigned n, unsigned k, int num_cus);
AutoChoice choose_auto(const Family &fam, int dev, int a_type, int b_type, bool act, unsigned m, unsigned n, unsigned k, int klass = kClassExact,
                       unsigned restrict_ = 0);
int auto_class(uint64_t solution_id);
bool is_auto_id(uint64_t solution_id);
unsigned plan_row_split(const SolutionEntry &e, unsigned splitk, unsigned m, unsigned n, unsigned k, int num_cus);
unsigned plan_row_split_native(const SolutionEntry &e, int klass, unsigned splitk, unsigned m, unsigned n, unsigned k, int num_cus);
extern std::atomic<int> g_mxfp4_default_class; // -1: $PETIT_AMD_MXFP4_ACTIVATIONS not read yet
int mxfp4_default_class();
int auto_default_class(uint64_t solution_id, int b_type, unsigned m);

// --- dispatch.hip
constexpr int kMaxDevices = 64;
constexpr uintptr_t kWorkspaceAlign = 256;
struct Workspace {
    std::atomic<void *> ptr{nullptr};
    std::atomic<uint64_t> bytes{0};
    std::atomic<uintptr_t> stream{kUnbound};
    static constexpr uintptr_t kUnbound = ~(uintptr_t)0;
};
extern Workspace g_workspace[kMaxDevices];
int current_device();
uint64_t splitk_bytes(unsigned splitk, unsigned m, unsigned n);
uint64_t workspace_need(const SolutionEntry &e, unsigned splitk, unsigned m, unsigned n, unsigned k, bool have_qa = false);
void *registered_workspace(int dev, void *stream, uint64_t need, bool *busy);
// the MFMA-native images attached to packed NVFP4 weight pointers (petit_nvfp4_native_attach)
int attach_image(const void *b, const void *image);
const void *attached_image(const void *b);

// A dense call is planned, then launched (gemm_impl); the C-ABI queries read the same plan.
struct GemmCall { // the arguments of gemm_impl but the scratch (a query has no matrices: null pointers)
    int b_type;
    unsigned *c;
    const unsigned *a, *b, *scales;
    const float *global_scale;
    unsigned m, n, k;
    const petit_solution_hints *hints;
    uint64_t solution_id;
    const petit_epilogue *epilogue;
    void *stream;
    const NativeIo *io;
    const void *image = nullptr; // NVFP4 weights: the image the call brings (a transient call's, built into its scratch); else the attached one
};
struct Scratch { // the scratch a call can use
    enum Kind { kCallBuffer, kRegistered, kQuery } kind;
    void *ptr;      // kCallBuffer: the call's own buffer (kRegistered: the workspace registered for the device, looked up per need)
    uint64_t bytes; // kCallBuffer, kQuery: its size (a query has no pointer)
};
struct LaunchPlan {
    int rc = kOk;                         // a refusal, or kOk -- with entry == nullptr: nothing to launch (m, n or k = 0)
    int klass = kClassExact;              // the accuracy class
    const SolutionEntry *entry = nullptr; // kernel and K split, after the scratch fallbacks (the split the id / row / pick names: scratch is sized for it)
    unsigned splitk = 1;
    LaunchGeometry geo{};                 // grid, spans per K part and K slices of the launch: unsplit where K is too short for the named split
    const void *nv_image = nullptr;       // NVFP4 weights on a native kernel: the MFMA-native image it reads
    uint64_t need = 0;                    // scratch bytes, and the scratch (nullptr for a query)
    void *ws = nullptr;
    bool act = false, reduce_act = false; // SiLU-mul in the kernel's epilogue / in the reduce pass of a K split (geo.slices > 1)
};
struct GemmPlan : LaunchPlan {
    unsigned bulk_rows = 0; // 0: one launch.  Else bulk + tail: the row where the tail starts, and the plans of both parts (then entry / splitk name the whole
    LaunchPlan bulk, tail;  // problem's kernel; need is the larger part's, and at least what the default class was taken for)
    bool tune = false;      // $PETIT_AMD_AUTOTUNE=1 and a default pick no table knows: the launcher tunes it, then plans again
    void *build_image = nullptr; // a transient call: the launcher builds the NVFP4 image here (offset 0 of the call's scratch) before the first part
};
// `part`: one part of a bulk + tail call, never split again
GemmPlan plan_gemm(const GemmCall &g, const Scratch &s, bool part = false);
const void *query_image(); // what a query takes for the image of an NVFP4 native-class call (it has no `b`)

} // namespace petit_amd
