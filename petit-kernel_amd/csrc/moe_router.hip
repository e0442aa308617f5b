// moe_router.hip -- the router's GEMM (include/petit_amd.h "The router's GEMM"): logits [T][E] = hidden [T][K] . W[E][K]^T (+ bias), 16-bit
// inputs, fp32 accumulation on v_mfma_f32_16x16x32_{bf16,f16}.  A skinny, weight-streaming GEMM: no dequantisation, no FP4, no LDS.
//
// One wave owns 16 x 16 output tiles.  The hidden rows are the MFMA's A operand, the router's rows (W[e][k], the checkpoint's layout) its B
// operand: lane l reads 16 bytes at row (l & 15), k = k0 + 8 (l >> 4) of either, so neither tensor is repacked.  K is cut into S slices of L
// (router_geometry: a function of E and K alone); the partial sum of a slice is ONE chain of L / 32 MFMAs from a zero accumulator, k ascending,
// and a logit is ((p_0 + p_1) + ... + p_{S-1}) + bias in fp32.  Two forms produce those bits:
//   split (T <= kSplitMaxT): grid = n-blocks x S slices x m-tiles, a workgroup's 4 waves take 4 neighbouring n-tiles of one slice and store the
//     partial tile to slab s of [S][T][E] with plain stores; whoever reads the slabs adds them in order (the route kernels, or router_finish).
//   whole (above): grid = n-blocks x m-blocks, a wave walks all S slices of 1 m-tile x 4 n-tiles (an A fragment feeds 4 MFMAs; the 4 waves of
//     a workgroup make the m-block 64 rows, so W comes from L2 once per 64 rows); each slice accumulates from zero and joins the running total
//     with one plain fp32 add -- the slab sum's additions -- and ONE slab is stored.
// Rows past T and experts past E are read as the last row / expert (the loads stay inside the tensors) and never stored.  An MFMA computes
// every output element from its own row and column alone, so a token's logits depend on nothing but its hidden state: not on T, not on the
// row's position in its tile, not on the form.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/petit_amd.h"
#include "device_common.hpp"
#include "petit_internal.h"

using namespace petit_amd;

namespace {

constexpr unsigned kSplitMaxT = 1024; // the largest T of the split form (profiles/moe_router.md has the timings that chose it)
constexpr unsigned kMaxSlices = kRouterMaxSlices;
constexpr unsigned kMaxK = 16384;
constexpr unsigned kWholeTiles = 4;  // n-tiles per wave of the whole form

template <class T> __device__ __forceinline__ typename T::frag load_frag(const unsigned short *p) {
    return __builtin_bit_cast(typename T::frag, *reinterpret_cast<const u32x4 *>(p));
}

// KU consecutive k-steps of the wave's NT tiles from k = kk on: every load first, then the MFMAs, per tile in ascending k
template <class T, int NT, int KU>
__device__ __forceinline__ void k_steps(f32x4 (&acc)[NT], const unsigned short *a_ptr, const unsigned short *(&b_ptr)[NT], unsigned kk) {
    typename T::frag a[KU], b[NT][KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        a[u] = load_frag<T>(a_ptr + kk + 32 * u);
#pragma unroll
        for (int j = 0; j < NT; ++j)
            b[j][u] = load_frag<T>(b_ptr[j] + kk + 32 * u);
    }
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int j = 0; j < NT; ++j)
            acc[j] = mfma16(a[u], b[j][u], acc[j]);
}

// T: Bf16 / Fp16.  NT n-tiles per wave.  kWhole: see the head of the file.
template <class T, int NT, bool kWhole>
__global__ __launch_bounds__(256) void moe_router_gemm_kernel(float *slabs, const unsigned short *hidden, const unsigned short *weight,
                                                              unsigned num_tokens, unsigned num_experts, unsigned k, unsigned slice_k,
                                                              unsigned slices) {
#pragma clang fp contract(off)
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned m0, n0, s_lo, s_hi;
    if constexpr (kWhole) {
        n0 = blockIdx.x * (NT * 16u), m0 = (blockIdx.y * 4u + wave) * 16u, s_lo = 0, s_hi = slices;
    } else {
        n0 = (blockIdx.x * 4u + wave) * (NT * 16u), m0 = blockIdx.z * 16u, s_lo = blockIdx.y, s_hi = s_lo + 1;
    }
    if (m0 >= num_tokens || n0 >= num_experts)
        return; // (a whole wave)
    const unsigned kq = (lane >> 4) * 8u;
    const unsigned a_row = min(m0 + (lane & 15u), num_tokens - 1);
    const unsigned short *a_ptr = hidden + (size_t)a_row * k + kq;
    const unsigned short *b_ptr[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
        b_ptr[j] = weight + (size_t)min(n0 + 16u * j + (lane & 15u), num_experts - 1) * k + kq;

    f32x4 total[NT];
    for (unsigned s = s_lo; s < s_hi; ++s) {
        const unsigned k_end = min(k, (s + 1) * slice_k);
        f32x4 acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // KU k-steps at a time, the largest batches first: one memory latency per batch, the MFMAs of a tile always in ascending k
        unsigned kk = s * slice_k;
        constexpr int KU = kWhole ? 4 : 8;
        for (; kk + 32 * KU <= k_end; kk += 32 * KU)
            k_steps<T, NT, KU>(acc, a_ptr, b_ptr, kk);
        if constexpr (KU > 4)
            if (kk + 128 <= k_end)
                k_steps<T, NT, 4>(acc, a_ptr, b_ptr, kk), kk += 128;
        if (kk + 64 <= k_end)
            k_steps<T, NT, 2>(acc, a_ptr, b_ptr, kk), kk += 64;
        if (kk < k_end)
            k_steps<T, NT, 1>(acc, a_ptr, b_ptr, kk);
        // the accumulators leave the loop's basic block: see mfma_join_pin (device_common.hpp)
#pragma unroll
        for (int j = 0; j < NT; ++j)
            mfma_join_pin(acc[j]);
        mfma_join_settle();
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            mfma_join_pin(acc[j]);
            if (s == s_lo)
                total[j] = acc[j];
            else
                total[j] = total[j] + acc[j];
        }
    }

    float *out = slabs + (kWhole ? (size_t)0 : (size_t)s_lo * num_tokens * num_experts);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const unsigned e = n0 + 16u * j + (lane & 15u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned t = m0 + (lane >> 4) * 4u + i;
            const float v = total[j][i];
            if (t < num_tokens && e < num_experts)
                out[(size_t)t * num_experts + e] = v;
        }
    }
}

// the definition's additions for one logit per thread: the slabs in order, then the bias
__global__ __launch_bounds__(256) void moe_router_finish_kernel(float *logits, const float *slabs, unsigned n_slabs, const float *router_bias,
                                                                unsigned num_experts, size_t count) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        float v = slabs[i];
        for (unsigned s = 1; s < n_slabs; ++s)
            v = v + slabs[(size_t)s * count + i];
        if (router_bias)
            v = v + router_bias[i % num_experts];
        logits[i] = v;
    }
}

// S and L from (E, K): slices of at least 128 k (256 from 129 experts on, where the n-tiles alone fill the chip), and no more than kMaxSlices
// of them.  a_type does not enter today; it is an argument so that it may.
void geometry(unsigned num_experts, unsigned k, int /*a_type*/, unsigned *slices, unsigned *slice_k) {
    const unsigned base = num_experts <= 128 ? 128u : 256u;
    const unsigned cap = ((k + kMaxSlices - 1) / kMaxSlices + 31u) / 32u * 32u;
    const unsigned L = base > cap ? base : cap;
    *slice_k = L;
    *slices = k ? (k + L - 1) / L : 1u;
}

unsigned split_max_t() {
    // $PETIT_AMD_ROUTER_SPLIT_MAX_T: the form switch, for measuring it (tools/moe_bench.py); read once
    static const unsigned v = [] {
        const char *e = std::getenv("PETIT_AMD_ROUTER_SPLIT_MAX_T");
        return e && *e ? (unsigned)std::strtoul(e, nullptr, 10) : kSplitMaxT;
    }();
    return v;
}

template <class T> void launch_gemm(float *slabs, const void *hidden, const void *weight, unsigned num_tokens, unsigned num_experts, unsigned k,
                                    hipStream_t stream) {
    unsigned S, L;
    geometry(num_experts, k, T::kType, &S, &L);
    const unsigned short *a = (const unsigned short *)hidden, *w = (const unsigned short *)weight;
    const unsigned m_tiles = (num_tokens + 15) / 16;
    if (num_tokens <= split_max_t()) {
        const dim3 grid((num_experts + 63) / 64, S, m_tiles);
        hipLaunchKernelGGL((moe_router_gemm_kernel<T, 1, false>), grid, dim3(256), 0, stream, slabs, a, w, num_tokens, num_experts, k, L, S);
    } else {
        const dim3 grid((num_experts + 16 * kWholeTiles - 1) / (16 * kWholeTiles), (m_tiles + 3) / 4);
        hipLaunchKernelGGL((moe_router_gemm_kernel<T, (int)kWholeTiles, true>), grid, dim3(256), 0, stream, slabs, a, w, num_tokens, num_experts, k,
                           L, S);
    }
}

uint64_t round256(uint64_t b) { return (b + 255) / 256 * 256; }

} // namespace

namespace petit_amd {

int router_shape_rc(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type) {
    if (k < 32 || k > kMaxK || k % 32 != 0 || num_experts == 0 || num_experts > kMoeMaxExperts || num_tokens >= kMaxM)
        return kErrProblemShape;
    if (a_type != kDataTypeBf16 && a_type != kDataTypeFp16)
        return kErrBadArgument;
    return kOk;
}

unsigned router_slabs(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type) {
    unsigned S, L;
    geometry(num_experts, k, a_type, &S, &L);
    return num_tokens <= split_max_t() ? S : 1u;
}

uint64_t router_slab_bytes(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type) {
    return round256((uint64_t)router_slabs(num_tokens, num_experts, k, a_type) * num_tokens * num_experts * 4);
}

void router_gemm_launch(float *slabs, const void *hidden, const void *weight, int a_type, unsigned num_tokens, unsigned num_experts, unsigned k,
                        hipStream_t stream) {
    if (a_type == kDataTypeBf16)
        launch_gemm<Bf16>(slabs, hidden, weight, num_tokens, num_experts, k, stream);
    else
        launch_gemm<Fp16>(slabs, hidden, weight, num_tokens, num_experts, k, stream);
}

void router_finish_launch(float *logits, const float *slabs, unsigned n_slabs, const float *router_bias, unsigned num_tokens,
                          unsigned num_experts, hipStream_t stream) {
    const size_t count = (size_t)num_tokens * num_experts;
    const unsigned blocks = (unsigned)((count + 255) / 256 < 4096 ? (count + 255) / 256 : 4096);
    hipLaunchKernelGGL(moe_router_finish_kernel, dim3(blocks), dim3(256), 0, stream, logits, slabs, n_slabs, router_bias, num_experts, count);
}

} // namespace petit_amd

extern "C" {

void petit_moe_router_geometry(unsigned num_experts, unsigned k, int a_type, unsigned *slices, unsigned *slice_k) {
    unsigned S, L;
    geometry(num_experts, k, a_type, &S, &L);
    if (slices)
        *slices = S;
    if (slice_k)
        *slice_k = L;
}

unsigned petit_moe_router_slabs(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type) {
    return router_slabs(num_tokens, num_experts, k, a_type);
}

uint64_t petit_moe_router_workspace_bytes(unsigned num_tokens, unsigned num_experts, unsigned k, int a_type) {
    if (router_shape_rc(num_tokens, num_experts, k, a_type) != kOk)
        return 0;
    return router_slab_bytes(num_tokens, num_experts, k, a_type);
}

int petit_moe_router_logits(float *logits, const void *hidden, const void *weight, const float *router_bias, int a_type, unsigned num_tokens,
                            unsigned num_experts, unsigned k, void *workspace, void *stream) {
    const int rc = router_shape_rc(num_tokens, num_experts, k, a_type);
    if (rc != kOk)
        return rc;
    if (num_tokens == 0)
        return kOk;
    if (!logits || !hidden || !weight || !workspace || ((uintptr_t)hidden | (uintptr_t)weight) % 16 != 0)
        return kErrProblemShape;
    const unsigned n_slabs = router_slabs(num_tokens, num_experts, k, a_type);
    const hipStream_t s = (hipStream_t)stream;
    if (n_slabs == 1 && !router_bias) {
        router_gemm_launch(logits, hidden, weight, a_type, num_tokens, num_experts, k, s);
    } else {
        router_gemm_launch((float *)workspace, hidden, weight, a_type, num_tokens, num_experts, k, s);
        router_finish_launch(logits, (const float *)workspace, n_slabs, router_bias, num_tokens, num_experts, s);
    }
    return hipGetLastError() == hipSuccess ? kOk : kErrLaunch;
}

} // extern "C"
