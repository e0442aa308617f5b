// dispatch.hip -- the dispatcher behind every GEMM entry point (plan_gemm decides, gemm_impl launches the plan), the scratch-memory rules and the tuner's candidate list.
// Replaces fp4/gemm_fp4_fp16_grid.cc:11-77 (Dispatcher, GemmFp4Fp16GridImpl), which has no scratch, no launch-error check and no fused epilogue.
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/petit_amd.h"
#include "dispatch.h"

namespace petit_amd {

// Scratch memory.  A call that needs scratch (fp32 slabs of a cross-workgroup K split, the quantised activations of the
// native-FP4 path) takes it, in this order, from
//   1. the per-call workspace handed to petit_gemm_*_ws (caller-owned, stream-ordered by construction: what the Python
//      layer does with torch's caching allocator, and what concurrent streams / graphs must use);
//   2. the workspace registered per device with petit_set_workspace.  One buffer cannot serve two streams at once, so it
//      BINDS to the first stream that uses it; a call from any other stream is refused (PETIT_ERROR_BAD_ARGUMENT) until
//      petit_set_workspace is called again -- never a silent race.
Workspace g_workspace[kMaxDevices];

int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices)
        return 0;
    return dev;
}

uint64_t splitk_bytes(unsigned splitk, unsigned m, unsigned n) {
    return splitk > 1 ? (uint64_t)splitk * m * n * sizeof(float) : 0;
}
// bytes of scratch a (kernel, split) needs for (m, n, k): [native: quantised activations, 256-B aligned][slabs]
uint64_t workspace_need(const SolutionEntry &e, unsigned splitk, unsigned m, unsigned n, unsigned k, bool have_qa) {
    const uint64_t slabs = splitk_bytes(splitk, m, n);
    if (is_native_am(e.shape.am) && !have_qa) // (sized for MXFP8 activations; the MXFP4 form needs less)
        return slabs ? native_ws_aligned(m, k) + slabs : native_ws_bytes(m, k);
    return slabs;
}
// the registered workspace of `dev` for a call on `stream`: pointer, or nullptr (too small / none / *busy = other stream)
void *registered_workspace(int dev, void *stream, uint64_t need, bool *busy) {
    Workspace &ws = g_workspace[dev];
    void *ptr = ws.ptr.load();
    *busy = false;
    if (!ptr || ws.bytes.load() < need)
        return nullptr;
    uintptr_t expect = Workspace::kUnbound;
    if (!ws.stream.compare_exchange_strong(expect, (uintptr_t)stream) && expect != (uintptr_t)stream) {
        *busy = true;
        return nullptr;
    }
    return ptr;
}

// NVFP4 weights on the native class run on their MFMA-native image (nvnative.hip, "petit-cdna4-nv6/1").  Call sites that keep calling the reference's
// entry point with (b, scales) name the image by ATTACHING it to the packed weight pointer once at load time (petit_nvfp4_native_attach); the image
// stays the caller's memory.  Looked up only by native-class calls on NVFP4 weights (prefill-sized problems: a mutex and a hash probe).
struct ImageRegistry {
    std::mutex mu;
    std::unordered_map<const void *, const void *> map;
};
static ImageRegistry &image_registry() {
    static ImageRegistry r;
    return r;
}
const void *attached_image(const void *b) {
    ImageRegistry &r = image_registry();
    std::lock_guard<std::mutex> lock(r.mu);
    const auto it = r.map.find(b);
    return it == r.map.end() ? nullptr : it->second;
}
int attach_image(const void *b, const void *image) {
    ImageRegistry &r = image_registry();
    std::lock_guard<std::mutex> lock(r.mu);
    if (image)
        r.map[b] = image;
    else
        r.map.erase(b);
    return kOk;
}

// Candidates of a tuning run (tune.hip): every kernel of the class that can run (m, n, k) within `max_ws` bytes of scratch,
// with the K splits its kind supports.  Also the reference kernel the outputs are compared with (first element): the
// direct-path streaming kernel for the exact class (no staging, no K split: the simplest code path), the first 16x16x128
// (MXFP8) / 32x32x64 (MXFP4) native kernel for the native classes.
int tune_candidates(int a_type, int b_type, int klass, unsigned m, unsigned n, unsigned k, uint64_t max_ws, uint64_t *ids, uint64_t *needs,
                    int cap) {
    Family fam;
    b_type = canonical_b_type(b_type);
    if (!family_for(a_type, b_type, &fam) || !shape_ok(n, k) || m == 0)
        return 0;
    const unsigned nspans = k / (kTileK * span_tiles_for_k(k));
    const int num_cus = arch_info(current_device()).num_cus;
    int count = 0;
    auto push = [&](const SolutionEntry &e, unsigned sk, bool front) {
        const uint64_t need = workspace_need(e, sk, m, n, k);
        if (need > max_ws || count >= cap)
            return;
        const uint64_t id = make_solution_id(e.shape, fam.elem_b, entry_mfma(fam, e), sk);
        if (front && count) {
            ids[count] = ids[0], needs[count] = needs[0];
            ids[0] = id, needs[0] = need;
        } else {
            ids[count] = id, needs[count] = need;
        }
        ++count;
    };
    bool have_ref = false;
    for (int i = 0; i < fam.count; ++i) {
        const SolutionEntry &e = fam.entries[i];
        const StreamShape &s = e.shape;
        if (entry_class(e) != klass || !entry_fits(e, m, k))
            continue;
        const bool is_ref = !have_ref && (klass == kClassExact ? (s.am == 0 && s.wm == 1 && s.pa == 1) : true);
        have_ref |= is_ref;
        // prefill: the streaming kernels re-read W once per 16-64 rows -- tens of milliseconds per launch at M = 8192, never a winner above
        // M = 512 (0 of the 1104 measured rows there) -- so only the one that serves as the reference output is run
        if (!is_ref && m > 512 && s.am >= 0 && !is_batch(e))
            continue;
        // the batched-decode kernels beyond their regime (16-128-row workgroups that each stream their whole column block: not beyond M = 1024 / eight
        // m-blocks) are not candidates at all -- unsplit either (the cap used to sit below the push and only removed their K splits)
        static const unsigned batch_max_m = [] { // $PETIT_AMD_BATCH_MAX_M: experiments with the batched-decode kernels beyond their regime
            const char *v = getenv("PETIT_AMD_BATCH_MAX_M");
            return v && *v ? (unsigned)strtoul(v, nullptr, 10) : 1024u; // (measured: the 128 x 128 form wins `o` / `down` at M = 512 by 3-10 %: profiles/r05_summary.md)
        }();
        if (!is_ref && is_batch(e) && (m > batch_max_m || m > 8u * 16u * (unsigned)s.mt))
            continue;
        push(e, 1, is_ref);
        // K splits: the large-M kernels and the streaming kernels (direct and staged) take any split; the decode / shared-tile
        // kernels none
        // (measured: down 8192 x 28672 at M = 16, staged 16 x 64 tiles with a K split of 2: 29.0 us against 30.5 unsplit -- every CU
        // then pulls half of the activations)
        if (workgroup_tile(s).one_slice)
            continue;
        for (unsigned sk = 2; sk <= 8 && sk <= nspans; sk *= 2)
            if (guarded_splitk(e, sk, m, n, k, num_cus) == sk) // (a row must never name a split that choose_auto would take away again)
                push(e, sk, false);
    }
    // The table's own row for this problem is always a candidate: 110 rows of the 129 ... 4096 buckets name batched-decode kernels beyond the eight-m-block cap above (narrow N --
    // 576 ... 3072 columns -- where W stays in L2 and many small workgroups fill the chip; measured winners of round 5), and a row the tuner cannot time can never be
    // challenged by a newer kernel (tools/adopt_rows.py compares against the row's own time in the same session).
    if (const uint64_t row = tuned_solution(current_device(), a_type, b_type, m, n, k, klass)) {
        bool have = false;
        for (int i = 0; i < count; ++i)
            have |= ids[i] == row;
        const SolutionEntry *e = have ? nullptr : find_explicit(fam, row);
        const unsigned sk = solution_splitk(row);
        if (e && sk && entry_class(*e) == klass && entry_fits(*e, m, k))
            push(*e, sk, false);
    }
    return count;
}

const void *query_image() {
    static const char marker = 0; // (never read)
    return &marker;
}

// the native pipeline's restrictions of a call (pre-quantised activations / quantised SiLU-mul output: 32x32x64 kernels only)
static unsigned native_restrictions(const NativeIo *io) {
    return (io && io->a_format ? kNeedK32 : 0u) | (io && io->out_format ? kNeedQuantOut : 0u);
}

// rows [row0, row0 + rows) of a call as a call of their own; `auto_tail`: as PETIT_SOLUTION_AUTO with no NativeIo (the tail of the native class's bulk + tail)
static GemmCall rows_of(const GemmCall &g, unsigned row0, unsigned rows, bool auto_tail) {
    GemmCall r = g;
    r.m = rows;
    if (g.c) { // (a query has no matrices)
        const bool act = g.epilogue && activation_gated(g.epilogue->activation);
        r.c = (unsigned *)((char *)g.c + (size_t)row0 * (act ? g.n / 2 : g.n) * sizeof(uint16_t));
        r.a = (const unsigned *)((const char *)g.a + (size_t)row0 * g.k * sizeof(uint16_t));
    }
    if (auto_tail)
        r.solution_id = PETIT_SOLUTION_AUTO, r.io = nullptr;
    return r;
}

// petit_gemm_nvfp4_native_transient: the image is built per call into the front of the call's scratch -- [image, nv6_image_bytes rounded up to 256][the
// native call's own scratch] -- and the call is planned as the call it stands for, on the scratch behind the image: with 16-bit activations and result the
// attached-image call (petit_gemm_fp4_fp16_grid_ws with the sentinel: its bulk + tail row split included; the image is built once, before the bulk, and
// the exact tail reads b / scales), with pre-quantised activations or a quantised output petit_gemm_nvfp4_native on that image.  Every refusal comes
// from this plan, before the build.
static GemmPlan plan_transient(const GemmCall &g, const Scratch &s) {
    GemmPlan p;
    const auto refuse = [&p](int rc) { return p.rc = rc, p; };
    if (g.m == 0 || g.n == 0 || g.k == 0)
        return p;
    if (g.solution_id == PETIT_SOLUTION_AUTO)
        return refuse(kErrKernelShape); // (the exact class reads the packed tensors: there is nothing to build; exact ids: plan_gemm)
    if (g.n % kTileN || g.k % 256 || nv6_elem_bytes(g.n, g.k) >= (1ull << 32))
        return refuse(kErrProblemShape); // shapes the image does not take
    const uint64_t img = (nv6_image_bytes(g.n, g.k) + kWorkspaceAlign - 1) & ~(uint64_t)(kWorkspaceAlign - 1);
    void *image;
    Scratch rest;
    if (s.kind == Scratch::kQuery) {
        image = (void *)query_image();
        rest = Scratch{Scratch::kQuery, nullptr, s.bytes > img ? s.bytes - img : 0};
    } else if (s.kind == Scratch::kCallBuffer && s.bytes >= img) {
        image = s.ptr;
        rest = Scratch{Scratch::kCallBuffer, (char *)s.ptr + img, s.bytes - img};
    } else { // (the rules of a native call whose scratch is missing / too small; the registered workspace is never used for the image)
        return refuse(s.kind != Scratch::kCallBuffer || is_auto_id(g.solution_id) ? kErrKernelShape : kErrBadArgument);
    }
    NativeIo io = *g.io;
    io.transient = false;
    GemmCall gi = g;
    gi.io = (io.a_format || io.out_format) ? &io : nullptr; // (16-bit in and out: planned exactly as the attached-image call, io == nullptr)
    gi.image = image;
    p = plan_gemm(gi, rest);
    if (p.rc == kOk && p.entry)
        p.build_image = image, p.need += img;
    return p;
}

// Every check and decision of a dense call, in the order they are made, and no launch: argument and range checks, the accuracy class, the NVFP4 image, the
// pick, the bulk + tail row split, the scratch fallbacks, the launch geometry (how many K slices the named split really gives, and so whether SiLU-mul is
// the reduce pass's or the kernel's own epilogue's).  It keeps no state between calls; the registered workspace is looked up where the launcher needs it,
// which binds it to the call's stream.
GemmPlan plan_gemm(const GemmCall &g, const Scratch &s, bool part) {
    if (g.io && g.io->transient && !part)
        return plan_transient(g, s);
    GemmPlan p;
    const auto refuse = [&p](int rc) { return p.rc = rc, p; };
    const petit_epilogue *epilogue = g.epilogue;
    const NativeIo *io = g.io;
    const petit_solution_hints *hints = g.hints;
    const unsigned m = g.m, n = g.n, k = g.k;
    if (epilogue && (!activation_known(epilogue->activation) || epilogue->reserved != 0))
        return refuse(kErrBadArgument); // reject what a newer caller might ask for
    const bool act = epilogue && activation_gated(epilogue->activation); // SiLU-mul or SwiGLU-OAI: one set of rules, the kind goes to the epilogue
    const unsigned a_format = io ? io->a_format : 0u, out_format = io ? io->out_format : 0u;
    if ((a_format != 0 && a_format != 8 && a_format != 6 && a_format != 4) || (out_format != 0 && out_format != 8 && out_format != 6 && out_format != 4))
        return refuse(kErrBadArgument);
    if (m == 0 || n == 0 || k == 0)
        return p; // gemm_fp4_fp16_grid.cc:42-44
    if (!hints)
        return refuse(kErrBadArgument);
    if (hints->c_type != hints->a_type)
        return refuse(kErrKernelShape);
    Family fam;
    if (!family_for(hints->a_type, g.b_type, &fam))
        return refuse(kErrKernelShape);
    if (!shape_ok(n, k))
        return refuse(kErrProblemShape);
    // SiLU-mul: gate / up halves made of whole n-tiles, and one descriptor spans half the matrix
    if (act && (n % 32 != 0 || (uint64_t)n * k / 2 >= (1ull << 32)))
        return refuse(kErrProblemShape);
    // 32-bit buffer offsets inside one n-tile row / activation block
    if ((uint64_t)k * 16 * 4 * 2 >= (1ull << 31) || (uint64_t)k * 64 * 4 >= (1ull << 31))
        return refuse(kErrProblemShape);
    // M: every kernel addresses A and C per workgroup (64-bit base + a 32-bit offset inside at most 256 rows), so the exact kernels take any M
    // up to the tables' last bucket (prefill chunks of 16375 x 57344 included); beyond it, refuse rather than wrap a grid dimension
    if (m > kMaxM)
        return refuse(kErrProblemShape);
    // the native pipeline: pre-quantised activations / quantised SiLU-mul output (MXFP4 weights, 32x32x64 kernels only)
    const unsigned restrict_ = native_restrictions(io);
    if (out_format && !act)
        return refuse(kErrBadArgument); // (the quantised output is the SiLU-mul epilogue's)
    if (out_format && (n % 512 != 0 || ((uintptr_t)g.c & 15)))
        return refuse(kErrProblemShape); // the consumer's K = n / 2 must be a whole number of 256-column producer tiles
    if (a_format && ((uintptr_t)g.a & 15))
        return refuse(kErrBadArgument);

    const int dev = current_device();
    // scratch of `need` bytes: the call's own buffer (a query's byte count) when large enough, else the registered workspace when it is and serves this
    // stream (busy: it is bound to another)
    bool busy = false;
    const auto take = [&](uint64_t need, void **ws) {
        void *const ptr = s.kind == Scratch::kRegistered ? registered_workspace(dev, g.stream, need, &busy) : s.bytes >= need ? s.ptr : nullptr;
        if (ws)
            *ws = ptr;
        return s.kind == Scratch::kRegistered ? ptr != nullptr : s.bytes >= need;
    };
    const auto attached = [&] { return g.image ? g.image : s.kind == Scratch::kQuery ? query_image() : attached_image(g.b); };
    const bool is_auto = is_auto_id(g.solution_id);
    int klass = auto_class(g.solution_id);
    uint64_t need_class = 0;
    if (const int dflt = (restrict_ == 0) ? auto_default_class(g.solution_id, g.b_type, m) : kClassExact) {
        // the process-wide default class: taken when the scratch of this call (its own, else the registered one) covers the class's pick
        const AutoChoice chn = choose_auto(fam, dev, hints->a_type, g.b_type, act, m, n, k, dflt, 0);
        const uint64_t need_n = chn.entry ? workspace_need(*chn.entry, chn.splitk, m, n, k) : 0;
        if (chn.entry && take(need_n, nullptr))
            klass = dflt, need_class = need_n;
    }
    p.klass = klass;
    // NVFP4 weights: the native class runs on the weights' MFMA-native image (e4m3 group scales are not E8M0 block scales: nvnative.hip), handed
    // over by petit_gemm_nvfp4_native or attached to `b` beforehand; without one the call is refused, never served by another accuracy class
    const void *nv_image = g.b_type != kDataTypeFp4e2m1 ? nullptr : (io && io->image) ? io->image : klass != kClassExact ? attached() : nullptr;
    if (klass != kClassExact && g.b_type == kDataTypeFp4e2m1 && !nv_image)
        return refuse(kErrKernelShape);
    // the native kernels read the quantised activations (k-tile major, up to m * k bytes) through ONE 32-bit buffer descriptor, and the
    // quantiser's grid has one row per activation row
    if ((klass != kClassExact || a_format) && ((uint64_t)m * k >= (1ull << 32) || m > 65535u))
        return refuse(kErrProblemShape);
    if (restrict_ && is_auto && klass == kClassExact)
        return refuse(kErrKernelShape); // quantised I/O is the native class's: name it (a sentinel or an explicit native id)
    if (a_format && klass != kClassExact && (unsigned)klass != a_format)
        return refuse(kErrKernelShape); // activations quantised to one format, kernel class of the other
    const SolutionEntry *entry = nullptr;
    unsigned splitk = 1;
    if (is_auto) {
        p.tune = klass == kClassExact && !act && autotune_enabled() && tuned_solution(dev, hints->a_type, g.b_type, m, n, k, kClassExact) == 0;
        const AutoChoice ch = choose_auto(fam, dev, hints->a_type, g.b_type, act, m, n, k, klass, restrict_);
        entry = ch.entry, splitk = ch.splitk;
        if (!entry)
            return refuse(kErrKernelShape);
        // bulk + tail: two default-pick launches on row ranges of A and C, same stream, same scratch (the launches are ordered) -- in the exact class
        // (plan_row_split), or the native class at a ragged prefill M (plan_row_split_native): bulk in the class, the few dozen rows of the tail through the
        // exact default.  (io == nullptr: the entry points that take petit_native_args refuse PETIT_SOLUTION_AUTO.)
        unsigned m1 = 0;
        if (!part && !autotune_enabled()) {
            if (klass == kClassExact && !io)
                m1 = plan_row_split(*entry, splitk, m, n, k, arch_info(dev).num_cus);
            else if (klass != kClassExact && restrict_ == 0 && !(io && io->image))
                m1 = plan_row_split_native(*entry, klass, splitk, m, n, k, arch_info(dev).num_cus);
        }
        if (m1) {
            // BOTH parts are planned before either is launched: a tail that cannot run must not leave C half written or one launch in a stream capture
            //  -- the call then runs as the single launch it would have been
            p.bulk = plan_gemm(rows_of(g, 0, m1, false), s, true);
            if (p.bulk.rc == kOk)
                p.tail = plan_gemm(rows_of(g, m1, m - m1, klass != kClassExact), s, true);
            if (p.bulk.rc == kOk && p.tail.rc == kOk) {
                p.bulk_rows = m1;
                p.entry = entry, p.splitk = splitk, p.need = std::max({need_class, p.bulk.need, p.tail.need});
                return p;
            }
        }
    } else {
        entry = find_explicit(fam, g.solution_id);
        if (!entry)
            return refuse(kErrKernelShape);
        if (!entry_fits(*entry, m, k))
            return refuse(kErrProblemShape);
        splitk = solution_splitk(g.solution_id);
        if (splitk == 0)
            return refuse(kErrKernelShape);
        if (splitk > 1 && workgroup_tile(entry->shape).one_slice)
            return refuse(kErrKernelShape); // decode / mid take no K split across workgroups: what their launchers refuse, the queries refuse too
        if (act && !act_runs(*entry, splitk, restrict_))
            return refuse(kErrKernelShape); // unsplit: needs an even number of n-tiles per wave; split: a 16-bit output (the reduce pass applies SiLU-mul)
        if (!entry_allows(*entry, restrict_) || (a_format && (unsigned)entry_class(*entry) != a_format))
            return refuse(kErrKernelShape);
        if (g.b_type == kDataTypeFp4e2m1 && ((io && io->image) || g.image) && entry_class(*entry) == kClassExact)
            return refuse(kErrKernelShape); // an image names the native class: an exact kernel would read image bytes as packed weights
    }

    if (is_native_am(entry->shape.am) && ((uint64_t)m * k >= (1ull << 32) || m > 65535u))
        return refuse(kErrProblemShape); // (an explicit native id: the same descriptor range as above)
    if (is_native_am(entry->shape.am) && g.b_type == kDataTypeFp4e2m1) {
        if (!nv_image)
            nv_image = attached(); // (an explicit native id)
        if (!nv_image)
            return refuse(kErrKernelShape); // an explicit native id on NVFP4 weights that have no image attached
        if (nv6_elem_bytes(n, k) >= (1ull << 32))
            return refuse(kErrProblemShape); // (the image's element part is read through one 32-bit buffer descriptor)
        p.nv_image = nv_image;
    }

    const bool have_qa = a_format != 0;
    uint64_t need = workspace_need(*entry, splitk, m, n, k, have_qa);
    void *ws = nullptr;
    if (need) {
        bool got = take(need, &ws);
        if (!is_auto && (s.kind == Scratch::kRegistered ? busy : !got))
            return refuse(kErrBadArgument); // too small for the kernel the caller named / the registered workspace is bound to another stream: pass one per call
        if (!got && klass != kClassExact && is_auto && splitk > 1) {
            // native default pick with a K split, scratch (per call or registered) covers the activations only, or they came quantised: the
            // same kernel unsplit.  SiLU-mul rode on the reduce pass of the split (act_runs): unsplit it is the kernel's own epilogue's job, which
            // needs gate and up tile in one wave (act_ok) -- a row like the 64 x 320 kernel (five n-tiles per wave) x split 4 cannot, and returned
            // kOk with C unwritten: re-pick
            if (act && !act_ok(*entry)) {
                unsigned sk1 = 1;
                const SolutionEntry *e1 = heuristic_native(fam, klass, m, n, k, true, /*have_slabs=*/false, &sk1, restrict_);
                if (!e1)
                    return refuse(kErrKernelShape);
                entry = e1;
            }
            const uint64_t need1 = workspace_need(*entry, 1, m, n, k, have_qa);
            if (!need1)
                splitk = 1, need = 0;
            else if (take(need1, &ws))
                splitk = 1, need = need1, got = true;
        }
        if (!got && need) {
            if (!is_auto || klass != kClassExact)
                return refuse(kErrKernelShape); // explicit id (or the native class) that needs scratch nobody provided
            // AUTO without scratch: the best kernel that needs none (not the K-split pick minus its split: a tiled kernel
            // chosen FOR its split leaves most of the chip idle without it)
            entry = heuristic(fam, m, n, k, act);
            splitk = 1, need = 0;
            if (!entry || workspace_need(*entry, 1, m, n, k))
                return refuse(kErrKernelShape); // (unreachable: the heuristic never picks a native kernel)
        }
    }
    // SiLU-mul: in the kernel's epilogue unsplit; by the reduce pass over plain slabs with a cross-workgroup K split
    p.act = act && splitk == 1;
    p.reduce_act = act && splitk > 1;
    p.geo = launch_geometry(entry->shape, splitk, m, n, k);
    if (p.reduce_act && p.geo.slices <= 1 && !p.geo.one_slice) {
        // K is too short for the split the id (or the table row) names: one slice, no reduce pass -- the launch is unsplit and SiLU-mul its own epilogue's job.
        // (`need` stays the named split's: what the call was sized for.  The decode / mid kernels take no split at all: their launchers refuse one.)
        if (!act_ok(*entry)) {
            if (!is_auto)
                return refuse(kErrKernelShape);
            if (klass != kClassExact) { // native class: the class's best kernel whose own epilogue applies SiLU-mul, within the scratch at hand
                unsigned sk1 = 1;
                const SolutionEntry *e1 = heuristic_native(fam, klass, m, n, k, true, /*have_slabs=*/false, &sk1, restrict_);
                if (!e1 || workspace_need(*e1, 1, m, n, k, have_qa) > workspace_need(*entry, splitk, m, n, k, have_qa))
                    return refuse(kErrKernelShape);
                entry = e1;
            } else {
                entry = heuristic(fam, m, n, k, true);
                if (!entry || workspace_need(*entry, 1, m, n, k))
                    return refuse(kErrKernelShape);
            }
            splitk = 1;
        }
        p.act = true, p.reduce_act = false;
        p.geo = launch_geometry(entry->shape, 1, m, n, k);
    }
    p.entry = entry, p.splitk = splitk, p.need = need, p.ws = ws;
    return p;
}

// one planned launch
static int launch(const GemmCall &g, const LaunchPlan &p) {
    if (p.rc != kOk || !p.entry)
        return p.rc;
    const unsigned a_format = g.io ? g.io->a_format : 0u;
    GemmArgs args{};
    args.c = g.c, args.a = g.a, args.w = g.b, args.s = g.scales, args.gs = g.global_scale;
    if (p.nv_image)
        args.w = p.nv_image, args.s = (const char *)p.nv_image + nv6_elem_bytes(g.n, g.k);
    args.m = g.m, args.n = g.n, args.k = g.k;
    args.bias = g.epilogue ? g.epilogue->bias : nullptr;
    args.qa = a_format ? (const void *)g.a : nullptr, args.qa_format = a_format, args.out_format = g.io ? g.io->out_format : 0u;
    args.workspace = (float *)p.ws;
    const unsigned kind = g.epilogue ? (unsigned)g.epilogue->activation : 0u; // 1 SiLU-mul / 2 SwiGLU-OAI where p.act or p.reduce_act
    args.act = p.act ? kind : 0u, args.reduce_act = p.reduce_act ? kind : 0u;
    return p.entry->launch(args, p.geo, (hipStream_t)g.stream);
}

int gemm_impl(int b_type, unsigned *c, const unsigned *a, const unsigned *b, const unsigned *scales,
              const float *global_scale, unsigned m, unsigned n, unsigned k,
              const petit_solution_hints *hints, uint64_t solution_id, const petit_epilogue *epilogue,
              void *call_ws, uint64_t call_ws_bytes, void *stream, const NativeIo *io) {
    // the matrices and the call's scratch, which queries have not (a call with m, n or k = 0 has nothing to do, whatever its pointers).  Scratch: f32x4
    // slabs and 16-byte activation loads -- the contract is 256-byte alignment (petit_amd.h)
    if (m && n && k && (!c || !a || !b || !scales || !global_scale || (!call_ws && call_ws_bytes) || ((uintptr_t)call_ws & (kWorkspaceAlign - 1))))
        return kErrBadArgument;
    const GemmCall g{b_type, c, a, b, scales, global_scale, m, n, k, hints, solution_id, epilogue, stream, io};
    const Scratch s = call_ws ? Scratch{Scratch::kCallBuffer, call_ws, call_ws_bytes} : Scratch{Scratch::kRegistered, nullptr, 0};
    GemmPlan p = plan_gemm(g, s);
    if (p.tune) {
        // $PETIT_AMD_AUTOTUNE=1: a problem no table knows is tuned once, here, before its first real launch (tune.hip), and planned again.  The
        // candidates are limited to the scratch THIS call can use: its own, else the registered workspace if it serves this stream
        void *tws = call_ws;
        uint64_t tws_bytes = call_ws ? call_ws_bytes : 0;
        if (!tws) {
            bool busy = false;
            const int dev = current_device();
            const uint64_t reg = g_workspace[dev].bytes.load();
            tws = reg ? registered_workspace(dev, stream, reg, &busy) : nullptr;
            tws_bytes = tws ? reg : 0;
        }
        autotune_on_first_sight(b_type, c, a, b, scales, global_scale, m, n, k, hints->a_type, tws, tws_bytes, stream);
        p = plan_gemm(g, s);
    }
    if (p.rc == kOk && p.build_image) { // a transient call: its image first, in stream order on the same stream
        const int rc = nv6_image(p.build_image, b, scales, n, k, (hipStream_t)stream);
        if (rc != kOk)
            return rc;
    }
    if (!p.bulk_rows)
        return launch(g, p);
    const int rc = launch(rows_of(g, 0, p.bulk_rows, false), p.bulk);
    if (rc != kOk)
        return rc; // (a launch error of the device: nothing a different plan would have avoided)
    return launch(rows_of(g, p.bulk_rows, m - p.bulk_rows, p.klass != kClassExact), p.tail);
}

} // namespace petit_amd
