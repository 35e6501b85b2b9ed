// Code length of a symbol sequence under the coding tables, on the device: what the range coder (csrc/rans_host.cpp,
// rans_encode_run; csrc/rans_lanes.hip) would spend on "these symbols under these tables", added up in exact integer
// arithmetic without writing a plane, sorting a row or leaving the GPU.  One probe of the target-rate search (DESIGN.md
// "Target-rate coding") is h_a, h_s and two of these launches.
//
// Per symbol s under table t, as the coder walks it: v = s - offset[t], maxv = cdf_sizes[t] - 2.
//   0 <= v < maxv : one table put,                                cost[t][v]
//   otherwise     : the escape slot, then the value in 4-bit bypass puts: raw = -2v - 1 (v < 0) or 2 (v - maxv), nb = its
//                   nibbles, nb / 15 + 1 puts for the count and nb for the value,   cost[t][maxv] + 4 (nb + nb / 15 + 1) bits
// cost is the host-built Q16 matrix of pcc_code_length_tables_build (-1 marks a slot the coder cannot code).
//
// Shape: a grid-stride loop over the [N, C] elements with the channel fastest (coalesced rows); a thread whose stride is a
// multiple of C stays on one channel and keeps its sum in a register, any other thread hands its sum to the workgroup's LDS
// bin whenever its channel moves on.  The bins go out as one 64-bit integer atomic per channel per workgroup: integer sums
// do not depend on the order of the additions, so two runs agree bit for bit.  The cost gathers (a few tens of KB per model)
// are left to the caches.
#include "common.h"
#include "entropy_prep.h"

namespace pcc {

constexpr int CL_THREADS = 256;
constexpr int CL_ELEMS = 4;                  // elements per thread before the grid stops growing
constexpr unsigned CL_MAX_BLOCKS = 1024;     // 256 CUs x 4: the pass is bound by the read of y and its parameters
constexpr int CL_MAX_CHANNELS = 4096;        // (C + 3) 64-bit LDS bins per workgroup
constexpr uint32_t CL_FLAG_INDEX = 2u, CL_FLAG_FREQ0 = 4u;      // the lane coder's bits (rans_lanes.h)

struct CostTables {
    const int32_t* cost;       // [n_tables, stride] Q16 bits, -1 = frequency 0
    const int32_t* sizes;      // cdf_sizes
    const int32_t* offsets;
    int32_t stride, n_tables;
};

// the running sums of one thread
struct CostSum {
    int64_t q16 = 0, ops = 0, escapes = 0;
    uint32_t flags = 0;
};

__device__ __forceinline__ void add_symbol(const CostTables& t, int32_t ix, int32_t s, CostSum& sum) {
    if ((uint32_t)ix >= (uint32_t)t.n_tables) { sum.flags |= CL_FLAG_INDEX; return; }
    const int32_t maxv = t.sizes[ix] - 2;
    if (maxv < 0 || maxv >= t.stride) { sum.flags |= CL_FLAG_INDEX; return; }      // not a table: nothing of it is read
    int32_t v = (int32_t)((uint32_t)s - (uint32_t)t.offsets[ix]);
    int puts = 0;                                 // bypass puts of an escaped value
    const bool escape = (uint32_t)v >= (uint32_t)maxv;
    if (escape) {
        const uint32_t raw = v < 0 ? 0u - 2u * (uint32_t)v - 1u : 2u * (uint32_t)(v - maxv);
        const int nb = raw ? (35 - __clz((int)raw)) / 4 : 0;
        puts = nb + nb / 15 + 1;
        v = maxv;
    }
    const int32_t cost = t.cost[(int64_t)ix * t.stride + v];
    if (cost < 0) { sum.flags |= CL_FLAG_FREQ0; return; }
    sum.q16 += cost + (int64_t)puts * (4 << 16);
    sum.ops += 1 + puts;
    sum.escapes += escape ? 1 : 0;
}

// bins: [c] Q16 sums, then operations, escapes, flags
__device__ __forceinline__ void bins_clear(unsigned long long* bins, int c) {
    for (int i = threadIdx.x; i < c + 3; i += CL_THREADS) bins[i] = 0ull;
    __syncthreads();
}

__device__ __forceinline__ void bins_finish(unsigned long long* bins, int c, const CostSum& sum, unsigned long long* out) {
    if (sum.ops) atomicAdd(&bins[c], (unsigned long long)sum.ops);
    if (sum.escapes) atomicAdd(&bins[c + 1], (unsigned long long)sum.escapes);
    if (sum.flags) atomicOr(&bins[c + 2], (unsigned long long)sum.flags);
    __syncthreads();
    for (int i = threadIdx.x; i < c + 3; i += CL_THREADS) {
        const unsigned long long b = bins[i];
        if (!b) continue;
        if (i == c + 2) atomicOr(&out[i], b);
        else atomicAdd(&out[i], b);
    }
}

enum { CL_GC = 0, CL_EB = 1 };

// a: y (CL_GC) or z (CL_EB), [N, C]; params: [N, 2C] (CL_GC); aux: the scale table (CL_GC) or the medians (CL_EB)
template <int MODE>
__global__ __launch_bounds__(CL_THREADS) void code_length_kernel(const float* __restrict__ a, const float* __restrict__ params,
                                                                 const float* __restrict__ aux, int64_t total, int c, int levels,
                                                                 CostTables t, unsigned long long* __restrict__ out) {
    extern __shared__ unsigned long long bins[];
    __shared__ float tb[256];
    if constexpr (MODE == CL_GC)
        for (int i = threadIdx.x; i < levels; i += CL_THREADS) tb[i] = aux[i];
    bins_clear(bins, c);
    const int64_t stride = (int64_t)gridDim.x * CL_THREADS;
    const int step = (int)(stride % c);          // 0: this thread's channel never changes
    int64_t e = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
    int ch = (int)(e % c), held = ch;
    CostSum sum;
    for (; e < total; e += stride) {
        if (ch != held) {
            if (sum.q16) atomicAdd(&bins[held], (unsigned long long)sum.q16);
            sum.q16 = 0;
            held = ch;
        }
        if constexpr (MODE == CL_GC) {
            const int64_t p = 2 * e - ch;          // row * 2C + ch
            const float mean = params[p + c];
            add_symbol(t, gc_scale_index(params[p], tb, levels), gc_symbol(a[e], mean), sum);
        } else {
            add_symbol(t, ch, (int32_t)eb_symbol_f(a[e], aux[ch]), sum);
        }
        ch += step;
        ch -= ch >= c ? c : 0;
    }
    if (sum.q16) atomicAdd(&bins[held], (unsigned long long)sum.q16);
    bins_finish(bins, c, sum, out);
}

// the planes that exist already, [C, N] channel-major: blockIdx.y is the channel
__global__ __launch_bounds__(CL_THREADS) void code_length_planes_kernel(const int32_t* __restrict__ sym, const int32_t* __restrict__ idx,
                                                                        int64_t n, int c, CostTables t,
                                                                        unsigned long long* __restrict__ out) {
    extern __shared__ unsigned long long bins[];
    bins_clear(bins, c);
    const int ch = blockIdx.y;
    const int64_t base = (int64_t)ch * n;
    CostSum sum;
    for (int64_t r = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * CL_THREADS)
        add_symbol(t, idx[base + r], sym[base + r], sum);
    if (sum.q16) atomicAdd(&bins[ch], (unsigned long long)sum.q16);
    bins_finish(bins, c, sum, out);
}

static int check_tables(const char* who, int32_t c, const int32_t* cost, int32_t cdf_stride, const int32_t* cdf_sizes,
                        const int32_t* offsets, int32_t n_tables, const int64_t* out) {
    PCC_REQUIRE(c >= 1 && c <= CL_MAX_CHANNELS, "%s: %d channels (1 .. %d)", who, c, CL_MAX_CHANNELS);
    PCC_REQUIRE(cost && cdf_sizes && offsets && out, "%s: the cost matrix, cdf_sizes, offsets and out are required", who);
    PCC_REQUIRE(cdf_stride >= 1 && n_tables >= 1, "%s: %d tables of stride %d", who, n_tables, cdf_stride);
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;

#define CL_GRID(total) dim3(blocks_for((total), CL_THREADS * CL_ELEMS, CL_MAX_BLOCKS)), dim3(CL_THREADS), \
                       (size_t)(c + 3) * sizeof(unsigned long long), as_stream(stream)

extern "C" {

int pcc_gc_code_length(const float* y, const float* params, int64_t n, int32_t c, const float* scale_table, int32_t levels,
                       const int32_t* cost, int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int64_t* out,
                       void* stream) {
    if (int rc = check_tables("pcc_gc_code_length", c, cost, cdf_stride, cdf_sizes, offsets, levels, out)) return rc;
    PCC_REQUIRE(levels >= 2 && levels <= 256, "pcc_gc_code_length: levels %d out of range", levels);
    PCC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)(c + 3) * sizeof(int64_t), as_stream(stream)));
    if (n <= 0) return PCC_OK;
    PCC_REQUIRE(y && params && scale_table, "pcc_gc_code_length: y, params and the scale table are required");
    const CostTables t{cost, cdf_sizes, offsets, cdf_stride, levels};      // one table per scale level
    hipLaunchKernelGGL(code_length_kernel<CL_GC>, CL_GRID(n * c), y, params, scale_table, n * c, c, levels, t,
                       reinterpret_cast<unsigned long long*>(out));
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_eb_code_length(const float* z, int64_t n, int32_t c, const float* medians, const int32_t* cost, int32_t cdf_stride,
                       const int32_t* cdf_sizes, const int32_t* offsets, int64_t* out, void* stream) {
    if (int rc = check_tables("pcc_eb_code_length", c, cost, cdf_stride, cdf_sizes, offsets, c, out)) return rc;
    PCC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)(c + 3) * sizeof(int64_t), as_stream(stream)));
    if (n <= 0) return PCC_OK;
    PCC_REQUIRE(z && medians, "pcc_eb_code_length: z and the medians are required");
    const CostTables t{cost, cdf_sizes, offsets, cdf_stride, c};          // one table per channel
    hipLaunchKernelGGL(code_length_kernel<CL_EB>, CL_GRID(n * c), z, (const float*)nullptr, medians, n * c, c, 0, t,
                       reinterpret_cast<unsigned long long*>(out));
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_code_length_planes(const int32_t* symbols, const int32_t* indexes, int64_t n, int32_t c, const int32_t* cost,
                           int32_t cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int32_t n_tables, int64_t* out,
                           void* stream) {
    if (int rc = check_tables("pcc_code_length_planes", c, cost, cdf_stride, cdf_sizes, offsets, n_tables, out)) return rc;
    PCC_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)(c + 3) * sizeof(int64_t), as_stream(stream)));
    if (n <= 0) return PCC_OK;
    PCC_REQUIRE(symbols && indexes, "pcc_code_length_planes: the symbol and index planes are required");
    const CostTables t{cost, cdf_sizes, offsets, cdf_stride, n_tables};
    const unsigned per_channel = CL_MAX_BLOCKS / (unsigned)c ? CL_MAX_BLOCKS / (unsigned)c : 1u;
    hipLaunchKernelGGL(code_length_planes_kernel, dim3(blocks_for(n, CL_THREADS * CL_ELEMS, per_channel), (unsigned)c), dim3(CL_THREADS),
                       (size_t)(c + 3) * sizeof(unsigned long long), as_stream(stream), symbols, indexes, n, c, t,
                       reinterpret_cast<unsigned long long*>(out));
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
