// moe_route.hip -- the routing around the MoE launches (include/petit_amd.h "Routing on the device"): petit_moe_align sorts the
// (token, slot) entries of a top-k routing by expert, petit_moe_combine reduces each token's top-k results.  No host sync, no result
// that depends on the order of atomics: both are bit-reproducible and graph-capturable.
//
// Align: the flat entries are cut into chunks of kChunk, one workgroup each.  The position of entry p with id e is
//     (entries of experts < e) + (entries of expert e in earlier chunks) + (entries of expert e before p in p's chunk)
// The first two terms come from per-chunk histograms (LDS counters: a count does not depend on the order of its increments) and a
// scan over (expert, chunk); the third from the chunk's ids in LDS, each entry counting its equals among the entries before it.
// One chunk (num_tokens * topk <= kChunk, every decode batch) does all of it in ONE launch; more take three (count, scan, place).
#include <hip/hip_runtime.h>

#include "../../include/petit_amd.h"
#include "device_common.hpp"
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

// the chunk's ids into LDS (-1: unrouted or past the end); the chunk's histogram into cnt[0 .. num_experts) when cnt is given
__device__ __forceinline__ int load_chunk(const void *ids, bool i64, unsigned n_entries, unsigned num_experts, unsigned chunk, int *ids_s,
                                          unsigned *cnt) {
    const unsigned p = chunk * kChunk + threadIdx.x;
    const int id = p < n_entries ? routed_id(ids, i64, p, num_experts) : -1;
    ids_s[threadIdx.x] = id;
    if (cnt) {
        cnt[threadIdx.x] = 0; // (num_experts <= kChunk)
        __syncthreads();
        if (id >= 0)
            atomicAdd(&cnt[id], 1u);
    }
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

// one chunk: everything in one workgroup
__global__ __launch_bounds__(kChunk) void moe_align_one_kernel(const void *ids, unsigned i64, unsigned n_entries, unsigned topk,
                                                               unsigned num_experts, int *offsets, int *sorted_pos, int *token_index) {
    __shared__ __attribute__((aligned(16))) int ids_s[kChunk]; // (read as int4: rank_in_chunk)
    __shared__ unsigned cnt[kChunk], wave_sums[kChunk / 64];
    const int id = load_chunk(ids, i64 != 0, n_entries, num_experts, 0, ids_s, cnt);
    const unsigned c = threadIdx.x < num_experts ? cnt[threadIdx.x] : 0u;
    unsigned routed;
    const unsigned base = block_exclusive_scan(c, wave_sums, &routed);
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
template <bool kBf16> __device__ __forceinline__ float half_to_f32(unsigned short h) {
    if constexpr (kBf16) {
        return __builtin_bit_cast(float, (unsigned)h << 16);
    } else {
        const _Float16 f = __builtin_bit_cast(_Float16, h);
        return (float)f;
    }
}

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
                const float x = half_to_f32<kBf16>((unsigned short)(words[q / 2] >> (16 * (q % 2))));
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

bool route_shape_ok(unsigned num_tokens, unsigned topk, unsigned num_experts) {
    return topk != 0 && num_experts != 0 && num_experts <= kMoeMaxExperts && (uint64_t)num_tokens * topk < (1ull << 31);
}

unsigned align_chunks(unsigned num_tokens, unsigned topk) { return (unsigned)(((uint64_t)num_tokens * topk + kChunk - 1) / kChunk); }

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

} // extern "C"
