// moe_route.hip -- the routing around the MoE launches (include/petit_amd.h "Routing on the device"): petit_moe_align sorts the
// (token, slot) entries of a top-k routing by expert, petit_moe_combine reduces each token's top-k results.  No host sync, no result
// that depends on the order of atomics: both are bit-reproducible and graph-capturable.
//
// Align: the flat entries are cut into chunks of kChunk, one workgroup each.  The position of entry p with id e is
//     (entries of experts < e) + (entries of expert e in earlier chunks) + (entries of expert e before p in p's chunk)
// The first two terms come from per-chunk histograms (LDS counters: a count does not depend on the order of its increments) and a
// scan over (expert, chunk); the third from the chunk's ids in LDS, each entry counting its equals among the entries before it.
// One chunk (num_tokens * topk <= kChunk, every decode batch) does all of it in ONE launch; more take three (count, scan, place).
//
// Route: petit_moe_route turns router logits into top-k ids and weights, one wave per token: lane l holds the keys of experts l, l + 64, ...
// in registers (E <= 1024: 16 at most) as order-preserving unsigned ranks, and every selection -- of groups, then of experts -- is a round of
// a wave-wide arg-max on (rank, lowest index) with the winner masked out.  No LDS, no atomics.  petit_moe_route_align runs the same code in
// the align's single workgroup when the routing is one chunk: the ids go to the LDS array the align sorts, route + align are ONE launch.
// The _ex entries (petit_route_slots) make the same launch write the complete slot list of a token: the routed ids through an expert map
// (global -> local, -1 when not local), then S shared-expert slots with ids L .. L + S - 1 -- lanes topk .. topk + S - 1 of the token's wave.
// From the hidden state (petit_moe_route_hidden, "The router's GEMM"): the router GEMM of moe_router.hip leaves fp32 partial slabs, and the
// kSlab instantiations of the same route code read a logit as the sum of the slabs in order plus the router bias; everything after the logit
// is the code above.  Above 512 experts (the 16-key form has no register to spare) a finishing launch sums the slabs in front of the route.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/petit_amd.h"
#include "device_common.hpp"
#include "numfmt.h"
#include "petit_internal.h"

using namespace petit_amd;

namespace {

constexpr unsigned kChunk = 1024; // entries per workgroup = threads per workgroup

__device__ __forceinline__ int routed_id(const void *ids, bool i64, unsigned p, unsigned num_experts) {
    const long long v = i64 ? ((const long long *)ids)[p] : (long long)((const int *)ids)[p];
    return (v >= 0 && v < (long long)num_experts) ? (int)v : -1;
}

// exclusive scan of one value per thread over the workgroup (kChunk threads); *total gets the sum.  LDS scratch: 16 words.
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned *wave_sums, unsigned *total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (unsigned d = 1; d < 64; d *= 2) {
        const unsigned u = __shfl_up(incl, d);
        if (lane >= d)
            incl += u;
    }
    if (lane == 63)
        wave_sums[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (unsigned w = 0; w < kChunk / 64; ++w) {
        const unsigned s = wave_sums[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    __syncthreads(); // (wave_sums may be reused by the caller)
    *total = all;
    return before + incl - v;
}

// the histogram of the chunk's ids (one per thread) into cnt[0 .. num_experts); the caller's barrier publishes it
__device__ __forceinline__ void chunk_histogram(int id, unsigned *cnt) {
    cnt[threadIdx.x] = 0; // (num_experts <= kChunk)
    __syncthreads();
    if (id >= 0)
        atomicAdd(&cnt[id], 1u);
}

// the chunk's ids into LDS (-1: unrouted or past the end); the chunk's histogram into cnt[0 .. num_experts) when cnt is given
__device__ __forceinline__ int load_chunk(const void *ids, bool i64, unsigned n_entries, unsigned num_experts, unsigned chunk, int *ids_s,
                                          unsigned *cnt) {
    const unsigned p = chunk * kChunk + threadIdx.x;
    const int id = p < n_entries ? routed_id(ids, i64, p, num_experts) : -1;
    ids_s[threadIdx.x] = id;
    if (cnt)
        chunk_histogram(id, cnt);
    __syncthreads();
    return id;
}

// entries of the chunk before this thread's with the same id (stable order inside the chunk)
__device__ __forceinline__ unsigned rank_in_chunk(const int *ids_s, int id) {
    const unsigned end = (threadIdx.x & ~63u) + 64; // wave-uniform bound: everything before the wave's last entry
    unsigned rank = 0;
    for (unsigned i = 0; i < end; i += 4) {
        const int4 q = *reinterpret_cast<const int4 *>(ids_s + i);
        rank += (i + 0 < threadIdx.x && q.x == id) + (i + 1 < threadIdx.x && q.y == id) + (i + 2 < threadIdx.x && q.z == id) +
                (i + 3 < threadIdx.x && q.w == id);
    }
    return rank;
}

__device__ __forceinline__ void place(unsigned pos, unsigned topk, int *sorted_pos, int *token_index) {
    const unsigned p = blockIdx.x * kChunk + threadIdx.x;
    sorted_pos[pos] = (int)p;
    token_index[pos] = (int)(p / topk);
}

// rows [routed, n_entries) of the outputs: -1 (grid-stride over the launch's threads)
__device__ __forceinline__ void fill_tail(unsigned routed, unsigned n_entries, int *sorted_pos, int *token_index) {
    for (unsigned r = routed + blockIdx.x * kChunk + threadIdx.x; r < n_entries; r += gridDim.x * kChunk)
        sorted_pos[r] = -1, token_index[r] = -1;
}

// one chunk, after the scan of its histogram: the offsets, every entry to its position, the unrouted tail
__device__ __forceinline__ void align_one_place(int id, const int *ids_s, unsigned *cnt, unsigned base, unsigned routed, unsigned n_entries,
                                                unsigned topk, unsigned num_experts, int *offsets, int *sorted_pos, int *token_index) {
    if (threadIdx.x < num_experts)
        offsets[threadIdx.x] = (int)base;
    if (threadIdx.x == 0)
        offsets[num_experts] = (int)routed;
    cnt[threadIdx.x] = base; // (every thread has read its count: the scan's barriers)
    __syncthreads();
    if (id >= 0)
        place(cnt[id] + rank_in_chunk(ids_s, id), topk, sorted_pos, token_index);
    fill_tail(routed, n_entries, sorted_pos, token_index);
}

// one chunk: everything in one workgroup
__global__ __launch_bounds__(kChunk) void moe_align_one_kernel(const void *ids, unsigned i64, unsigned n_entries, unsigned topk,
                                                               unsigned num_experts, int *offsets, int *sorted_pos, int *token_index) {
    __shared__ __attribute__((aligned(16))) int ids_s[kChunk]; // (read as int4: rank_in_chunk)
    __shared__ unsigned cnt[kChunk], wave_sums[kChunk / 64];
    const int id = load_chunk(ids, i64 != 0, n_entries, num_experts, 0, ids_s, cnt);
    const unsigned c = threadIdx.x < num_experts ? cnt[threadIdx.x] : 0u;
    unsigned routed;
    const unsigned base = block_exclusive_scan(c, wave_sums, &routed);
    align_one_place(id, ids_s, cnt, base, routed, n_entries, topk, num_experts, offsets, sorted_pos, token_index);
}

// several chunks, 1/3: the per-chunk histograms, ws[chunk][expert]
__global__ __launch_bounds__(kChunk) void moe_align_count_kernel(const void *ids, unsigned i64, unsigned n_entries, unsigned num_experts,
                                                                 unsigned *ws) {
    __shared__ __attribute__((aligned(16))) int ids_s[kChunk]; // (read as int4: rank_in_chunk)
    __shared__ unsigned cnt[kChunk];
    load_chunk(ids, i64 != 0, n_entries, num_experts, blockIdx.x, ids_s, cnt);
    if (threadIdx.x < num_experts)
        ws[(size_t)blockIdx.x * num_experts + threadIdx.x] = cnt[threadIdx.x];
}

// 2/3 (one workgroup, thread e = expert e): ws[chunk][e] := the position of the chunk's first entry of expert e; the offsets
__global__ __launch_bounds__(kChunk) void moe_align_scan_kernel(unsigned chunks, unsigned num_experts, unsigned *ws, int *offsets) {
    __shared__ unsigned wave_sums[kChunk / 64];
    const unsigned e = threadIdx.x;
    unsigned run = 0;
    if (e < num_experts)
        for (unsigned b = 0; b < chunks; ++b) {
            const unsigned c = ws[(size_t)b * num_experts + e];
            ws[(size_t)b * num_experts + e] = run;
            run += c;
        }
    unsigned routed;
    const unsigned base = block_exclusive_scan(run, wave_sums, &routed);
    if (e < num_experts) {
        for (unsigned b = 0; b < chunks; ++b)
            ws[(size_t)b * num_experts + e] += base;
        offsets[e] = (int)base;
    }
    if (e == 0)
        offsets[num_experts] = (int)routed;
}

// 3/3: every entry to its position; the unrouted tail
__global__ __launch_bounds__(kChunk) void moe_align_place_kernel(const void *ids, unsigned i64, unsigned n_entries, unsigned topk,
                                                                 unsigned num_experts, const unsigned *ws, const int *offsets, int *sorted_pos,
                                                                 int *token_index) {
    __shared__ __attribute__((aligned(16))) int ids_s[kChunk]; // (read as int4: rank_in_chunk)
    const int id = load_chunk(ids, i64 != 0, n_entries, num_experts, blockIdx.x, ids_s, nullptr);
    if (id >= 0)
        place(ws[(size_t)blockIdx.x * num_experts + id] + rank_in_chunk(ids_s, id), topk, sorted_pos, token_index);
    fill_tail((unsigned)offsets[num_experts], n_entries, sorted_pos, token_index);
}

// Combine: one thread per 8 consecutive columns of one token (16-byte loads of each slot row, coalesced along n), grid-stride.
template <bool kBf16>
__global__ __launch_bounds__(256) void moe_combine_kernel(void *out, const void *slot_out, const float *weights, const void *ids, unsigned i64,
                                                          unsigned num_tokens, unsigned topk, unsigned n, unsigned num_experts) {
#pragma clang fp contract(off)
    const unsigned per_row = n / 8;
    const uint64_t items = (uint64_t)num_tokens * per_row;
    for (uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (uint64_t)gridDim.x * 256) {
        const unsigned t = (unsigned)(it / per_row), col = (unsigned)(it % per_row) * 8;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (unsigned j = 0; j < topk; ++j) {
            const unsigned p = t * topk + j;
            if (routed_id(ids, i64 != 0, p, num_experts) < 0)
                continue;
            const float w = weights[p];
            const uint4 v = *reinterpret_cast<const uint4 *>((const char *)slot_out + ((size_t)p * n + col) * 2);
            const unsigned words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float x = h16_f32<kBf16>((unsigned short)(words[q / 2] >> (16 * (q % 2))));
                const float prod = x * w;
                acc[q] = acc[q] + prod;
            }
        }
        uint4 o;
        unsigned ow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (kBf16) {
                const bf16x2 h = __builtin_convertvector(f32x2{acc[2 * q], acc[2 * q + 1]}, bf16x2); // RNE
                ow[q] = __builtin_bit_cast(unsigned, h);
            } else {
                const f16x2 h = __builtin_convertvector(f32x2{acc[2 * q], acc[2 * q + 1]}, f16x2); // RNE
                ow[q] = __builtin_bit_cast(unsigned, h);
            }
        }
        o.x = ow[0], o.y = ow[1], o.z = ow[2], o.w = ow[3];
        *reinterpret_cast<uint4 *>((char *)out + ((size_t)t * n + col) * 2) = o;
    }
}

// --- Route: router logits -> top-k ids and weights (the definition: include/petit_amd.h "Routing on the device") ---------------------------

constexpr unsigned kMaxTopk = 64;        // PETIT_MOE_MAX_TOPK: slot r of a token is lane r's
constexpr unsigned kRouteWaves = 4;      // waves (= tokens) per workgroup of the grid form
constexpr int kDataTypeFp32 = 100;       // PETIT_DTYPE_FP32

struct RouteArgs {
    const void *logits; // [num_tokens][num_experts], dtype
    const float *bias;  // [num_experts] or null (sigmoid scoring)
    int *ids;           // [num_tokens][topk + num_shared]
    float *weights;     // [num_tokens][topk + num_shared]
    float *keys;        // [num_tokens][num_experts] or null
    int dtype;
    unsigned num_tokens, num_experts, topk; // num_experts: the E global experts the routing ranks
    unsigned sigmoid, renorm, n_group, topk_group; // n_group 1: no groups
    float scale;
    // the slot list (petit_route_slots); without one: no map, num_local = num_experts, num_shared = 0
    unsigned num_local, num_shared; // L: ids the map may name; S: shared slots, ids L .. L + S - 1.  The align sorts L + S experts
    float shared_weight;
    const int *expert_map;   // [num_experts] or null: global id -> local id
    const void *shared_gate; // [num_tokens][num_shared], dtype, or null
};

// the slab form's arguments (petit_moe_route_hidden): logits = slab 0 of n_slabs fp32 slabs [num_tokens][num_experts], slab_stride elements apart
struct RouteSlabArgs : RouteArgs {
    const float *router_bias; // [num_experts] or null: the router linear's own bias
    size_t slab_stride;
    unsigned n_slabs;
};
template <bool kSlab> using RouteArgsOf = std::conditional_t<kSlab, RouteSlabArgs, RouteArgs>;

__device__ __forceinline__ float route_logit(const void *logits, int dtype, size_t i) {
    if (dtype == kDataTypeFp32)
        return ((const float *)logits)[i];
    const unsigned short h = ((const unsigned short *)logits)[i];
    return dtype == kDataTypeBf16 ? h16_f32<true>(h) : h16_f32<false>(h);
}

// The logit of expert e of the row, element i = row + e.  kSlab: the router GEMM's definition -- the slabs added in order, then the router bias.
template <bool kSlab, class Args> __device__ __forceinline__ float route_source(const Args &ra, size_t i, unsigned e) {
    if constexpr (!kSlab) {
        return route_logit(ra.logits, ra.dtype, i);
    } else {
#pragma clang fp contract(off)
        // every load first (one memory latency, not one per slab): slab min(s, n_slabs - 1) for s < kRouterMaxSlices -- a repeated
        // address past the last slab, never an address outside them -- then the additions of the slabs that exist, in order
        const float *p = (const float *)ra.logits + i;
        const unsigned last = ra.n_slabs - 1;
        float q[kRouterMaxSlices];
#pragma unroll
        for (unsigned s = 0; s < kRouterMaxSlices; ++s)
            q[s] = p[(size_t)(s < last ? s : last) * ra.slab_stride];
        const float b = ra.router_bias ? ra.router_bias[e] : 0.f;
        float v = q[0];
#pragma unroll
        for (unsigned s = 1; s < kRouterMaxSlices; ++s)
            v = s <= last ? v + q[s] : v;
        return ra.router_bias ? v + b : v;
    }
}

__device__ __forceinline__ float route_sigmoid(float x) {
#pragma clang fp contract(off)
    return 1.f / (1.f + expf(-x));
}

// A key as an unsigned that orders as the selection does: larger key = larger rank, NaN as -inf, -0 as +0.  Every key's rank is > 0: 0 marks
// an entry that cannot be selected (past E, outside the kept groups, already taken).  rank_key is the inverse on ranks > 0.
__device__ __forceinline__ unsigned key_rank(float k) {
    const float c = k != k ? -__builtin_inff() : (k == 0.f ? 0.f : k);
    const unsigned b = __builtin_bit_cast(unsigned, c);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rank_key(unsigned u) { return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// The value of a lane in the other half of this lane's aligned group of 2 d lanes, for butterfly reductions whose lanes all hold their group's
// result after every step (so "a lane of the other half" is all a step needs): DPP inside a row of 16, a permute across rows.
template <int kCtrl> __device__ __forceinline__ unsigned dpp_mov(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, 0xf, 0xf, false);
}
template <unsigned d> __device__ __forceinline__ unsigned other_half(unsigned v) {
    if constexpr (d == 1)
        return dpp_mov<0xB1>(v); // quad_perm [1, 0, 3, 2]
    else if constexpr (d == 2)
        return dpp_mov<0x4E>(v); // quad_perm [2, 3, 0, 1]
    else if constexpr (d == 4)
        return dpp_mov<0x141>(v); // row_half_mirror
    else if constexpr (d == 8)
        return dpp_mov<0x140>(v); // row_mirror
    else
        return (unsigned)__shfl_xor((int)v, (int)d);
}
template <unsigned d> __device__ __forceinline__ float other_half(float v) {
    return __builtin_bit_cast(float, other_half<d>(__builtin_bit_cast(unsigned, v)));
}

template <unsigned d> __device__ __forceinline__ void select_step(unsigned &hi, unsigned &lo) {
    const unsigned oh = other_half<d>(hi), ol = other_half<d>(lo);
    const bool take = oh > hi || (oh == hi && ol > lo);
    hi = take ? oh : hi;
    lo = take ? ol : lo;
}

// One selection round over the wave's N * 64 entries (entry j * 64 + lane has rank u[j]): the index of the largest rank, the LOWEST index
// among equal ranks; every lane gets it.  (The pair (rank, ~index) is maximised: a total order, so the result does not depend on the
// reduction's shape.)
template <int N> __device__ __forceinline__ unsigned wave_select(const unsigned (&u)[N], unsigned lane) {
    unsigned hi = 0, lo = 0;
#pragma unroll
    for (int j = N - 1; j >= 0; --j)
        if (u[j] >= hi)
            hi = u[j], lo = ~((unsigned)j * 64u + lane);
    select_step<1>(hi, lo);
    select_step<2>(hi, lo);
    select_step<4>(hi, lo);
    select_step<8>(hi, lo);
    select_step<16>(hi, lo);
    select_step<32>(hi, lo);
    return ~lo;
}

// the wave's sum, a fixed tree: lanes pairwise, then pairs, ... (6 additions deep); every lane gets it
__device__ __forceinline__ float wave_sum(float v) {
#pragma clang fp contract(off)
    v = v + other_half<1>(v);
    v = v + other_half<2>(v);
    v = v + other_half<4>(v);
    v = v + other_half<8>(v);
    v = v + other_half<16>(v);
    v = v + other_half<32>(v);
    return v;
}

template <unsigned d> __device__ __forceinline__ void top2_step(float &a1, float &a2) {
    const float b1 = other_half<d>(a1), b2 = other_half<d>(a2);
    a2 = fmaxf(fminf(a1, b1), fmaxf(a2, b2));
    a1 = fmaxf(a1, b1);
}

// One token by one wave (all 64 lanes, wave-uniform control flow).  NJ = ceil(E / 64) rounded up to a power of two: keys per lane.
// Lane r < topk returns slot r's id and weight.  kSlab: the logits come from the router GEMM's slabs (route_source).
template <int NJ, bool kSlab = false>
__device__ __forceinline__ void route_token(const RouteArgsOf<kSlab> &ra, unsigned t, unsigned lane, int *id_out, float *w_out) {
#pragma clang fp contract(off)
    const unsigned E = ra.num_experts;
    const size_t row = (size_t)t * E;
    unsigned u[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const unsigned e = (unsigned)j * 64u + lane;
        u[j] = 0;
        if (e < E) {
            float key = route_source<kSlab>(ra, row + e, e);
            if (ra.sigmoid) {
                key = route_sigmoid(key);
                if (ra.bias)
                    key = key + ra.bias[e];
            }
            if (ra.keys)
                ra.keys[row + e] = key;
            u[j] = key_rank(key);
        }
    }

    if (ra.n_group > 1) {
        // group scores: the sum of each group's two largest keys, group g's in lane g % 64, slot g / 64
        constexpr int NG = NJ > 1 ? NJ / 2 : 1; // (groups hold >= 2 experts: n_group <= 32 NJ)
        const unsigned G = E / ra.n_group;
        unsigned gu[NG];
#pragma unroll
        for (int s = 0; s < NG; ++s)
            gu[s] = 0;
        for (unsigned g = 0; g < ra.n_group; ++g) {
            const unsigned lo = g * G, hi = lo + G;
            float a1 = -__builtin_inff(), a2 = -__builtin_inff();
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (hi <= (unsigned)j * 64u || lo >= (unsigned)(j + 1) * 64u)
                    continue; // (wave-uniform)
                const unsigned e = (unsigned)j * 64u + lane;
                const float v = (e >= lo && e < hi) ? rank_key(u[j]) : -__builtin_inff();
                a2 = fmaxf(a2, fminf(a1, v));
                a1 = fmaxf(a1, v);
            }
            top2_step<1>(a1, a2);
            top2_step<2>(a1, a2);
            top2_step<4>(a1, a2);
            top2_step<8>(a1, a2);
            top2_step<16>(a1, a2);
            top2_step<32>(a1, a2);
            const unsigned r = key_rank(a1 + a2);
#pragma unroll
            for (int s = 0; s < NG; ++s)
                if (g == (unsigned)s * 64u + lane)
                    gu[s] = r;
        }
        // the topk_group best groups; only their experts stay selectable
        unsigned allow = 0;
        for (unsigned r = 0; r < ra.topk_group; ++r) {
            const unsigned g = wave_select<NG>(gu, lane);
#pragma unroll
            for (int s = 0; s < NG; ++s)
                if (g == (unsigned)s * 64u + lane)
                    gu[s] = 0;
            const unsigned lo = g * G, hi = lo + G;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const unsigned e = (unsigned)j * 64u + lane;
                allow |= (e >= lo && e < hi) ? 1u << j : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            u[j] = (allow >> j & 1u) ? u[j] : 0u;
    }

    unsigned my_id = 0;
    for (unsigned r = 0; r < ra.topk; ++r) {
        unsigned e = wave_select<NJ>(u, lane);
        e = e < E ? e : E - 1; // (always true: topk selectable entries exist; keeps the loads below inside the row whatever happens)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (e == (unsigned)j * 64u + lane)
                u[j] = 0;
        if (lane == r)
            my_id = e;
    }

    // weights: lane r < topk holds slot r
    const bool mine = lane < ra.topk;
    const float x = mine ? route_source<kSlab>(ra, row + my_id, my_id) : 0.f;
    float v, denom = 1.f;
    bool divide = ra.renorm != 0;
    if (ra.sigmoid) {
        v = mine ? route_sigmoid(x) : 0.f;
        if (divide)
            denom = wave_sum(v) + 1e-20f;
    } else {
        const float mx = __shfl(x, 0); // slot 0 is the row's largest logit
        v = mine ? expf(x - mx) : 0.f;
        if (divide) {
            denom = wave_sum(v);
        } else { // the softmax over all E: each lane's experts in ascending order, then the wave's tree
            float part = 0.f;
            for (unsigned e = lane; e < E; e += 64)
                part = part + expf(route_source<kSlab>(ra, row + e, e) - mx);
            denom = wave_sum(part);
            divide = true;
        }
    }
    float w = v;
    if (divide)
        w = w / denom;
    w = w * ra.scale;
    *id_out = (int)my_id;
    *w_out = w;
}

// route_token's (id, weight) of lane r to slot r of the token's slot list: lanes < topk map their global id (one gathered load; a value
// outside [0, L) is -1), lanes topk + s, s < S, take shared expert s: id L + s, weight shared_weight (* sigmoid(gate logit), one multiply).
// Both branches are wave-uniform; without a map and without shared experts nothing changes.
template <class Args> __device__ __forceinline__ void route_slots(const Args &ra, unsigned t, unsigned lane, int *id, float *w) {
#pragma clang fp contract(off)
    if (ra.expert_map) {
        const unsigned e = (unsigned)*id < ra.num_experts ? (unsigned)*id : ra.num_experts - 1; // (always true: keeps the load inside the map)
        const int m = ra.expert_map[e];
        *id = (m >= 0 && (unsigned)m < ra.num_local) ? m : -1;
    }
    if (ra.num_shared) {
        const unsigned s = lane - ra.topk;
        if (lane >= ra.topk && s < ra.num_shared) {
            float sw = ra.shared_weight;
            if (ra.shared_gate)
                sw = sw * route_sigmoid(route_logit(ra.shared_gate, ra.dtype, (size_t)t * ra.num_shared + s));
            *id = (int)(ra.num_local + s);
            *w = sw;
        }
    }
}

// the grid form: one wave per token
template <int NJ, bool kSlab = false> __global__ __launch_bounds__(kRouteWaves * 64) void moe_route_kernel(RouteArgsOf<kSlab> ra) {
    const unsigned lane = threadIdx.x & 63u, t = blockIdx.x * kRouteWaves + (threadIdx.x >> 6);
    if (t >= ra.num_tokens)
        return; // (a whole wave)
    int id;
    float w;
    route_token<NJ, kSlab>(ra, t, lane, &id, &w);
    route_slots(ra, t, lane, &id, &w);
    const unsigned slots = ra.topk + ra.num_shared; // (<= kMaxTopk: one lane each)
    if (lane < slots) {
        ra.ids[(size_t)t * slots + lane] = id;
        ra.weights[(size_t)t * slots + lane] = w;
    }
}

// one chunk (num_tokens * (topk + num_shared) <= kChunk): the workgroup's 16 waves route the tokens, the slot ids go to LDS as load_chunk leaves
// them (and to memory with the weights, for the combine), and the align's one-chunk code follows on the L + S experts the slot ids name
template <int NJ, bool kSlab = false>
__global__ __launch_bounds__(kChunk) void moe_route_align_one_kernel(RouteArgsOf<kSlab> ra, int *offsets, int *sorted_pos, int *token_index) {
    __shared__ __attribute__((aligned(16))) int ids_s[kChunk]; // (read as int4: rank_in_chunk)
    __shared__ unsigned cnt[kChunk], wave_sums[kChunk / 64];
    const unsigned lane = threadIdx.x & 63u, slots = ra.topk + ra.num_shared, n_entries = ra.num_tokens * slots;
    const unsigned align_experts = ra.num_local + ra.num_shared; // (<= kChunk; the routing above it ranks ra.num_experts)
    if (threadIdx.x >= n_entries)
        ids_s[threadIdx.x] = -1;
    for (unsigned t = threadIdx.x >> 6; t < ra.num_tokens; t += kChunk / 64) {
        int id;
        float w;
        route_token<NJ, kSlab>(ra, t, lane, &id, &w);
        if constexpr (NJ == 16) {
            // the 16-key form has no register to spare for the slot list's arguments across route_token: read them from the kernel
            // argument segment (scalar loads, RouteArgs is the first argument) once per token instead
            typedef const __attribute__((address_space(4))) RouteArgsOf<kSlab> *KernArgs;
            KernArgs ka = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(ka));
            route_slots(*ka, t, lane, &id, &w);
        } else {
            route_slots(ra, t, lane, &id, &w);
        }
        if (lane < slots) {
            const unsigned p = t * slots + lane; // (< n_entries <= kChunk)
            ra.ids[p] = id;
            ra.weights[p] = w;
            ids_s[p] = id;
        }
    }
    __syncthreads();
    const int id = ids_s[threadIdx.x];
    chunk_histogram(id, cnt);
    __syncthreads();
    const unsigned c = threadIdx.x < align_experts ? cnt[threadIdx.x] : 0u;
    unsigned routed;
    const unsigned base = block_exclusive_scan(c, wave_sums, &routed);
    align_one_place(id, ids_s, cnt, base, routed, n_entries, slots, align_experts, offsets, sorted_pos, token_index);
}

bool route_shape_ok(unsigned num_tokens, unsigned topk, unsigned num_experts) {
    return topk != 0 && num_experts != 0 && num_experts <= kMoeMaxExperts && (uint64_t)num_tokens * topk < (1ull << 31);
}

unsigned align_chunks(unsigned num_tokens, unsigned topk) { return (unsigned)(((uint64_t)num_tokens * topk + kChunk - 1) / kChunk); }

// every refusal of petit_moe_route(_ex) / petit_moe_route_align(_ex) that does not depend on an output pointer; fills ra's scalar fields and
// the slot list's two input pointers
int route_check(int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk, const petit_route_desc *desc,
                const petit_route_slots *slots, RouteArgs *ra) {
    static const petit_route_desc kDefault = {};
    static const petit_route_slots kNoSlots = {};
    const petit_route_desc &d = desc ? *desc : kDefault;
    const petit_route_slots &sl = slots ? *slots : kNoSlots;
    if (!route_shape_ok(num_tokens, topk, num_experts) || topk > num_experts || topk > kMaxTopk)
        return kErrProblemShape;
    if (logits_dtype != kDataTypeFp32 && logits_dtype != kDataTypeBf16 && logits_dtype != kDataTypeFp16)
        return kErrBadArgument;
    if (d.scoring != PETIT_ROUTE_SOFTMAX && d.scoring != PETIT_ROUTE_SIGMOID)
        return kErrBadArgument;
    const unsigned n_group = d.n_group ? d.n_group : 1u;
    if (n_group > 1) {
        if (d.scoring != PETIT_ROUTE_SIGMOID || num_experts % n_group != 0 || num_experts / n_group < 2 || d.topk_group < 1 ||
            d.topk_group > n_group || (uint64_t)topk > (uint64_t)d.topk_group * (num_experts / n_group))
            return kErrProblemShape;
    } else if (d.topk_group > 1) {
        return kErrProblemShape; // topk_group outside 1..n_group
    }
    if (d.bias && d.scoring != PETIT_ROUTE_SIGMOID)
        return kErrProblemShape;
    ra->bias = d.bias;
    ra->dtype = logits_dtype;
    ra->num_tokens = num_tokens, ra->num_experts = num_experts, ra->topk = topk;
    ra->sigmoid = d.scoring == PETIT_ROUTE_SIGMOID, ra->renorm = d.renormalize != 0;
    ra->n_group = n_group, ra->topk_group = n_group > 1 ? d.topk_group : 1u;
    ra->scale = d.routed_scaling_factor == 0.f ? 1.f : d.routed_scaling_factor;
    // the slot list: L local experts, S shared slots
    const unsigned L = sl.num_local_experts ? sl.num_local_experts : num_experts, S = sl.num_shared;
    if (L > num_experts || (!sl.expert_map && L != num_experts) || (uint64_t)topk + S > kMaxTopk || (uint64_t)L + S > kMoeMaxExperts ||
        (uint64_t)num_tokens * ((uint64_t)topk + S) >= (1ull << 31) || (sl.shared_gate_logits && S == 0))
        return kErrProblemShape;
    ra->num_local = L, ra->num_shared = S;
    ra->shared_weight = sl.shared_weight == 0.f ? 1.f : sl.shared_weight;
    ra->expert_map = sl.expert_map, ra->shared_gate = sl.shared_gate_logits;
    return kOk;
}

template <int NJ, bool kSlab = false>
void launch_route(const RouteArgsOf<kSlab> &ra, bool with_align, int32_t *offsets, int32_t *sorted_pos, int32_t *token_index, hipStream_t s) {
    if (with_align)
        hipLaunchKernelGGL((moe_route_align_one_kernel<NJ, kSlab>), dim3(1), dim3(kChunk), 0, s, ra, offsets, sorted_pos, token_index);
    else
        hipLaunchKernelGGL((moe_route_kernel<NJ, kSlab>), dim3((ra.num_tokens + kRouteWaves - 1) / kRouteWaves), dim3(kRouteWaves * 64), 0, s, ra);
}

// the slab form, E <= 512 (above: a finishing launch and the plain form, petit_moe_route_hidden)
void launch_route_slabs(const RouteSlabArgs &ra, bool with_align, int32_t *offsets, int32_t *sorted_pos, int32_t *token_index, hipStream_t s) {
    const unsigned E = ra.num_experts;
    if (E <= 64)
        launch_route<1, true>(ra, with_align, offsets, sorted_pos, token_index, s);
    else if (E <= 128)
        launch_route<2, true>(ra, with_align, offsets, sorted_pos, token_index, s);
    else if (E <= 256)
        launch_route<4, true>(ra, with_align, offsets, sorted_pos, token_index, s);
    else
        launch_route<8, true>(ra, with_align, offsets, sorted_pos, token_index, s);
}

void launch_route(const RouteArgs &ra, bool with_align, int32_t *offsets, int32_t *sorted_pos, int32_t *token_index, hipStream_t s) {
    const unsigned E = ra.num_experts;
    if (E <= 64)
        launch_route<1>(ra, with_align, offsets, sorted_pos, token_index, s);
    else if (E <= 128)
        launch_route<2>(ra, with_align, offsets, sorted_pos, token_index, s);
    else if (E <= 256)
        launch_route<4>(ra, with_align, offsets, sorted_pos, token_index, s);
    else if (E <= 512)
        launch_route<8>(ra, with_align, offsets, sorted_pos, token_index, s);
    else
        launch_route<16>(ra, with_align, offsets, sorted_pos, token_index, s);
}

} // namespace

extern "C" {

uint64_t petit_moe_align_workspace_bytes(unsigned num_tokens, unsigned topk, unsigned num_experts) {
    if (!route_shape_ok(num_tokens, topk, num_experts))
        return 0;
    const unsigned chunks = align_chunks(num_tokens, topk);
    return chunks <= 1 ? 0 : (uint64_t)chunks * num_experts * 4;
}

int petit_moe_align(const void *topk_ids, int ids_are_int64, unsigned num_tokens, unsigned topk, unsigned num_experts, int32_t *expert_offsets,
                    int32_t *sorted_pos, int32_t *token_index, void *workspace, void *stream) {
    if (!route_shape_ok(num_tokens, topk, num_experts) || !expert_offsets)
        return kErrProblemShape;
    const unsigned n_entries = num_tokens * topk, chunks = align_chunks(num_tokens, topk);
    if (n_entries && (!topk_ids || !sorted_pos || !token_index))
        return kErrProblemShape;
    if (chunks > 1 && !workspace)
        return kErrProblemShape;
    const hipStream_t s = (hipStream_t)stream;
    const unsigned i64 = ids_are_int64 ? 1u : 0u;
    if (chunks <= 1) {
        hipLaunchKernelGGL(moe_align_one_kernel, dim3(1), dim3(kChunk), 0, s, topk_ids, i64, n_entries, topk, num_experts, expert_offsets,
                           sorted_pos, token_index);
    } else {
        unsigned *ws = (unsigned *)workspace;
        hipLaunchKernelGGL(moe_align_count_kernel, dim3(chunks), dim3(kChunk), 0, s, topk_ids, i64, n_entries, num_experts, ws);
        hipLaunchKernelGGL(moe_align_scan_kernel, dim3(1), dim3(kChunk), 0, s, chunks, num_experts, ws, expert_offsets);
        hipLaunchKernelGGL(moe_align_place_kernel, dim3(chunks), dim3(kChunk), 0, s, topk_ids, i64, n_entries, topk, num_experts, ws,
                           expert_offsets, sorted_pos, token_index);
    }
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int petit_moe_combine(void *out, const void *slot_out, const float *topk_weights, const void *topk_ids, int ids_are_int64, unsigned num_tokens,
                      unsigned topk, unsigned n, unsigned num_experts, int dtype, void *stream) {
    if (!route_shape_ok(num_tokens, topk, num_experts) || n == 0 || n % 8 != 0)
        return kErrProblemShape;
    if (dtype != kDataTypeBf16 && dtype != kDataTypeFp16)
        return kErrBadArgument;
    if (num_tokens == 0)
        return kOk;
    if (!out || !slot_out || !topk_weights || !topk_ids)
        return kErrProblemShape;
    const uint64_t items = (uint64_t)num_tokens * (n / 8);
    const unsigned blocks = (unsigned)((items + 255) / 256 < 65536 ? (items + 255) / 256 : 65536);
    const unsigned i64 = ids_are_int64 ? 1u : 0u;
    if (dtype == kDataTypeBf16)
        hipLaunchKernelGGL(moe_combine_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, slot_out, topk_weights, topk_ids, i64,
                           num_tokens, topk, n, num_experts);
    else
        hipLaunchKernelGGL(moe_combine_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, slot_out, topk_weights, topk_ids, i64,
                           num_tokens, topk, n, num_experts);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int petit_moe_route_ex(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                       const petit_route_desc *desc, const petit_route_slots *slots, int32_t *topk_ids, float *topk_weights, float *keys_out,
                       void *stream) {
    RouteArgs ra;
    const int rc = route_check(logits_dtype, num_tokens, num_experts, topk, desc, slots, &ra);
    if (rc != kOk)
        return rc;
    if (num_tokens == 0)
        return kOk;
    if (!router_logits || !topk_ids || !topk_weights)
        return kErrProblemShape;
    ra.logits = router_logits, ra.ids = topk_ids, ra.weights = topk_weights, ra.keys = keys_out;
    launch_route(ra, false, nullptr, nullptr, nullptr, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int petit_moe_route(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                    const petit_route_desc *desc, int32_t *topk_ids, float *topk_weights, float *keys_out, void *stream) {
    return petit_moe_route_ex(router_logits, logits_dtype, num_tokens, num_experts, topk, desc, nullptr, topk_ids, topk_weights, keys_out, stream);
}

uint64_t petit_moe_route_align_ex_workspace_bytes(unsigned num_tokens, unsigned topk, unsigned num_experts, const petit_route_slots *slots) {
    const unsigned L = slots && slots->num_local_experts ? slots->num_local_experts : num_experts, S = slots ? slots->num_shared : 0u;
    if ((uint64_t)topk + S > kMaxTopk || (uint64_t)L + S > kMoeMaxExperts)
        return 0;
    return petit_moe_align_workspace_bytes(num_tokens, topk + S, L + S);
}

uint64_t petit_moe_route_align_workspace_bytes(unsigned num_tokens, unsigned topk, unsigned num_experts) {
    return petit_moe_align_workspace_bytes(num_tokens, topk, num_experts);
}

int petit_moe_route_align_ex(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                             const petit_route_desc *desc, const petit_route_slots *slots, int32_t *topk_ids, float *topk_weights,
                             float *keys_out, int32_t *expert_offsets, int32_t *sorted_pos, int32_t *token_index, void *workspace, void *stream) {
    RouteArgs ra;
    const int rc = route_check(logits_dtype, num_tokens, num_experts, topk, desc, slots, &ra);
    if (rc != kOk)
        return rc;
    if (!expert_offsets)
        return kErrProblemShape;
    if (num_tokens && (!router_logits || !topk_ids || !topk_weights || !sorted_pos || !token_index))
        return kErrProblemShape;
    const unsigned n_slots = topk + ra.num_shared, align_experts = ra.num_local + ra.num_shared;
    if (align_chunks(num_tokens, n_slots) > 1 && !workspace)
        return kErrProblemShape;
    if (num_tokens == 0 || align_chunks(num_tokens, n_slots) > 1) { // nothing to route, or several chunks: the route grid, then the align's launches
        if (num_tokens) {
            const int rr = petit_moe_route_ex(router_logits, logits_dtype, num_tokens, num_experts, topk, desc, slots, topk_ids, topk_weights,
                                              keys_out, stream);
            if (rr != kOk)
                return rr;
        }
        return petit_moe_align(topk_ids, 0, num_tokens, n_slots, align_experts, expert_offsets, sorted_pos, token_index, workspace, stream);
    }
    ra.logits = router_logits, ra.ids = topk_ids, ra.weights = topk_weights, ra.keys = keys_out;
    launch_route(ra, true, expert_offsets, sorted_pos, token_index, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

int petit_moe_route_align(const void *router_logits, int logits_dtype, unsigned num_tokens, unsigned num_experts, unsigned topk,
                          const petit_route_desc *desc, int32_t *topk_ids, float *topk_weights, float *keys_out, int32_t *expert_offsets,
                          int32_t *sorted_pos, int32_t *token_index, void *workspace, void *stream) {
    return petit_moe_route_align_ex(router_logits, logits_dtype, num_tokens, num_experts, topk, desc, nullptr, topk_ids, topk_weights, keys_out,
                                    expert_offsets, sorted_pos, token_index, workspace, stream);
}

// --- from the hidden state: the router GEMM (moe_router.hip), then the route on its slabs ("The router's GEMM") --------------------------------
// workspace: [the GEMM's slabs][E > 512: the finished logits][the align's workspace], each rounded up to 256 bytes

static uint64_t route_hidden_logit_bytes(unsigned num_tokens, unsigned num_experts) {
    return num_experts > 512 ? ((uint64_t)num_tokens * num_experts * 4 + 255) / 256 * 256 : 0;
}

uint64_t petit_moe_route_hidden_workspace_bytes(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type, unsigned topk,
                                                const petit_route_slots *slots) {
    if (router_shape_rc(num_tokens, num_experts, k, a_type) != kOk)
        return 0;
    return router_slab_bytes(num_tokens, num_experts, k, a_type) + route_hidden_logit_bytes(num_tokens, num_experts) +
           petit_moe_route_align_ex_workspace_bytes(num_tokens, topk, num_experts, slots);
}

int petit_moe_route_hidden(const void *hidden, const void *weight, const float *router_bias, int a_type, unsigned num_tokens, unsigned num_experts,
                           unsigned k, unsigned topk, const petit_route_desc *desc, const petit_route_slots *slots, int32_t *topk_ids,
                           float *topk_weights, float *keys_out, int32_t *expert_offsets, int32_t *sorted_pos, int32_t *token_index, void *workspace,
                           void *stream) {
    int rc = router_shape_rc(num_tokens, num_experts, k, a_type);
    if (rc != kOk)
        return rc;
    RouteSlabArgs ra;
    rc = route_check(kDataTypeFp32, num_tokens, num_experts, topk, desc, slots, &ra); // (the logits, and a shared gate's, are fp32 here)
    if (rc != kOk)
        return rc;
    const bool with_align = expert_offsets != nullptr;
    const unsigned n_slots = topk + ra.num_shared, align_experts = ra.num_local + ra.num_shared;
    if (num_tokens == 0)
        return with_align ? petit_moe_align(topk_ids, 0, 0, n_slots, align_experts, expert_offsets, sorted_pos, token_index, nullptr, stream) : kOk;
    if (!hidden || !weight || !topk_ids || !topk_weights || !workspace || (with_align && (!sorted_pos || !token_index)) ||
        ((uintptr_t)hidden | (uintptr_t)weight) % 16 != 0)
        return kErrProblemShape;
    const hipStream_t s = (hipStream_t)stream;
    float *slabs = (float *)workspace;
    const uint64_t slab_bytes = router_slab_bytes(num_tokens, num_experts, k, a_type);
    float *finished = (float *)((char *)workspace + slab_bytes);
    void *align_ws = (char *)workspace + slab_bytes + route_hidden_logit_bytes(num_tokens, num_experts);
    const unsigned n_slabs = router_slabs(num_tokens, num_experts, k, a_type);
    const bool one_launch = with_align && align_chunks(num_tokens, n_slots) <= 1;

    router_gemm_launch(slabs, hidden, weight, a_type, num_tokens, num_experts, k, s);
    ra.ids = topk_ids, ra.weights = topk_weights, ra.keys = keys_out;
    if (n_slabs == 1 && !router_bias) { // the one slab IS the logits: the plain route reads it
        ra.logits = slabs;
        launch_route(ra, one_launch, expert_offsets, sorted_pos, token_index, s);
    } else if (num_experts > 512) {
        router_finish_launch(finished, slabs, n_slabs, router_bias, num_tokens, num_experts, s);
        ra.logits = finished;
        launch_route(ra, one_launch, expert_offsets, sorted_pos, token_index, s);
    } else {
        ra.logits = slabs, ra.router_bias = router_bias, ra.slab_stride = (size_t)num_tokens * num_experts, ra.n_slabs = n_slabs;
        launch_route_slabs(ra, one_launch, expert_offsets, sorted_pos, token_index, s);
    }
    if (hipGetLastError() != hipSuccess)
        return kErrLaunch;
    if (with_align && !one_launch)
        return petit_moe_align(topk_ids, 0, num_tokens, n_slots, align_experts, expert_offsets, sorted_pos, token_index, align_ws, stream);
    return kOk;
}

} // extern "C"
