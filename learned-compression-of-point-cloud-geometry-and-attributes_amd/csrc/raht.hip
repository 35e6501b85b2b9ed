// RAHT, the region-adaptive hierarchical transform (de Queiroz & Chou 2016) of per-voxel attributes: the transform of G-PCC's
// attribute coder, here the attribute half of the octree + RAHT anchor codec (../raht.py, ../anchor.py).  The contract is in
// include/pcc_hip.h (pcc_raht_plan / pcc_raht_transform).
//
// Rows are the voxels in ascending Morton order (the child index (x << 2) | (y << 1) | z of octree.hip at every level, so
// pcc_octree_expand's output is already in row order).  The transform has 3 * depth steps, one per key bit, finest first; at
// step s two nodes whose keys agree in key >> (s + 1) merge.  A node's value lives in its FIRST row: the low-pass result stays in
// the first row of the left node, the high-pass coefficient goes to the first row of the right node and is final there.
//
// The plan is closed form, one thread per row and no per-level compaction: row i > 0 is the first row of a right node at exactly
// one step, step[i] = the highest bit in which key[i] differs from key[i - 1]; its partner is left[i], the first row with the same
// key >> (step + 1); the weights are run lengths, found by two binary searches over the sorted keys.  The rows are then bucketed by
// step (one stable radix pass), so a step's launch covers only its own rows.
//
// The transform is one launch per step, thread = (row of the step, channel), and one launch for all the small steps at the top.  Within a step no row is read or written by two
// pairs and a finalised row is never touched again: no atomics, and the bytes of the result do not depend on the schedule.  Every
// operation is a separately rounded float64 one (the file is compiled with -ffp-contract=off; sqrt and the division are the
// correctly rounded ones), in the order the header states.
#include "common.h"
#include "sort.h"

namespace pcc {

constexpr int RAHT_BLOCK = 256;
constexpr int RAHT_MAX_CHANNELS = 16;
constexpr int RAHT_MAX_DEPTH = 17;            // 2^17 > COORD_LIMIT: every coordinate extent the library accepts
constexpr int RAHT_FOLD_ROWS = 256;            // steps of at most this many rows at the top of the tree share one launch
constexpr int RAHT_FOLD_BLOCK = 1024;
constexpr uint32_t RAHT_NO_STEP = 63;         // bucket key of the rows that belong to no step (row 0, duplicates): sorts last

__device__ __forceinline__ uint64_t raht_spread3(uint32_t v) {       // bit b -> bit 3 b (21 bits), as octree.hip
    uint64_t x = v & 0x1fffffu;
    x = (x | (x << 32)) & 0x1f00000000ffffull;
    x = (x | (x << 16)) & 0x1f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(RAHT_BLOCK) void raht_keys_kernel(const int32_t* __restrict__ coords, int64_t n, int ox, int oy, int oz,
                                                               int depth, uint64_t* __restrict__ keys, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (i >= n) return;
    // 64-bit differences: a coordinate and an origin of opposite signs must not wrap into the grid
    const int64_t gx = (int64_t)coords[4 * i + 1] - ox, gy = (int64_t)coords[4 * i + 2] - oy, gz = (int64_t)coords[4 * i + 3] - oz;
    const int64_t lim = 1ll << depth;
    const bool ok = gx >= 0 && gy >= 0 && gz >= 0 && gx < lim && gy < lim && gz < lim;
    if (!ok) atomicAdd(&status[0], 1);
    keys[i] = ok ? ((raht_spread3((uint32_t)gx) << 2) | (raht_spread3((uint32_t)gy) << 1) | raht_spread3((uint32_t)gz)) : 0ull;
}

// first row in [0, n) whose key is >= target (n when there is none)
__device__ __forceinline__ int64_t raht_lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t target) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(RAHT_BLOCK) void raht_plan_kernel(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ step,
                                                               int32_t* __restrict__ left, int32_t* __restrict__ w0, int32_t* __restrict__ w1,
                                                               uint32_t* __restrict__ bucket, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    const uint64_t diff = i ? (k ^ keys[i - 1]) : 0ull;
    if (diff == 0) {                                   // row 0 (the DC), or a second row of one voxel: in no step
        if (i) atomicAdd(&status[1], 1);
        step[i] = -1; left[i] = (int32_t)i; w0[i] = 0; w1[i] = 0;
        bucket[i] = RAHT_NO_STEP;
        return;
    }
    const int s = 63 - __clzll((long long)diff);       // <= 3 * 17 - 1: the shifts below stay under 64
    const uint64_t group = (k >> (s + 1)) << (s + 1);  // first key of the parent node; this row opens its right child
    const int64_t first = raht_lower_bound(keys, i, group);
    const int64_t end = raht_lower_bound(keys + i, n - i, ((k >> s) + 1) << s) + i;
    step[i] = s; left[i] = (int32_t)first; w0[i] = (int32_t)(i - first); w1[i] = (int32_t)(end - i);
    bucket[i] = (uint32_t)s;
}

// offsets[s] = the number of rows whose step is below s, s = 0 .. nsteps (sorted: the bucket keys in ascending order)
__global__ __launch_bounds__(64) void raht_offsets_kernel(const uint32_t* __restrict__ sorted, int64_t n, int nsteps, int32_t* __restrict__ offsets) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s > nsteps) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < (uint32_t)s) lo = mid + 1; else hi = mid;
    }
    offsets[s] = (int32_t)lo;
}

// One pair of a step: rows[0 .. m) are the first rows of the step's right nodes, t = (row of the step, channel).  forward: (a0, a1)
// -> (low, high); inverse: (low, high) -> (a0, a1).  Four roundings per output: two products, their sum or difference, the division.
template <bool INVERSE>
__device__ __forceinline__ void raht_pair(double* val, int64_t n, int c, const int32_t* __restrict__ rows, int64_t t,
                                          const int32_t* __restrict__ left, const int32_t* __restrict__ w0, const int32_t* __restrict__ w1) {
    const int64_t j = (t >> 32) ? t / c : (int64_t)((uint32_t)t / (uint32_t)c);      // (a 64-bit division is ~100 instructions)
    const int ch = (int)(t - j * c);
    const int64_t r = rows[j];
    if ((uint64_t)r >= (uint64_t)n) return;            // a plan that is not one never writes outside the values
    const int64_t l = left[r];
    const int32_t a = w0[r], b = w1[r];
    if ((uint64_t)l >= (uint64_t)n || l == r || a <= 0 || b <= 0) return;
    const double s0 = sqrt((double)a), s1 = sqrt((double)b), sn = sqrt((double)a + (double)b);
    const double p = val[l * c + ch], q = val[r * c + ch];
    if (INVERSE) {
        val[l * c + ch] = (s0 * p - s1 * q) / sn;
        val[r * c + ch] = (s1 * p + s0 * q) / sn;
    } else {
        val[l * c + ch] = (s0 * p + s1 * q) / sn;
        val[r * c + ch] = (s0 * q - s1 * p) / sn;
    }
}

template <bool INVERSE>
__global__ __launch_bounds__(RAHT_BLOCK) void raht_step_kernel(double* __restrict__ val, int64_t n, int c, const int32_t* __restrict__ rows,
                                                               int64_t m, const int32_t* __restrict__ left, const int32_t* __restrict__ w0,
                                                               const int32_t* __restrict__ w1) {
    const int64_t t = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (t < m * c) raht_pair<INVERSE>(val, n, c, rows, t, left, w0, w1);
}

// The top of the tree in ONE launch: steps [lo, hi), each of at most RAHT_FOLD_ROWS rows, run by one workgroup with a barrier
// between steps (a step reads what the step before wrote; the barrier orders the workgroup's global accesses).  The operations
// and their order are those of raht_step_kernel, so the bytes are the same.  A frame of 850 k voxels has some 15 such steps, a
// cloud of a few hundred rows nothing else.
struct RahtOffsets { int32_t at[3 * RAHT_MAX_DEPTH + 1]; };

template <bool INVERSE>
__global__ __launch_bounds__(RAHT_FOLD_BLOCK) void raht_fold_kernel(double* val, int64_t n, int c, const int32_t* __restrict__ step_rows,
                                                                    RahtOffsets off, int lo, int hi, const int32_t* __restrict__ left,
                                                                    const int32_t* __restrict__ w0, const int32_t* __restrict__ w1) {
    for (int k = 0; k < hi - lo; ++k) {
        const int s = INVERSE ? hi - 1 - k : lo + k;
        const int64_t work = (int64_t)(off.at[s + 1] - off.at[s]) * c;
        for (int64_t t = threadIdx.x; t < work; t += RAHT_FOLD_BLOCK) raht_pair<INVERSE>(val, n, c, step_rows + off.at[s], t, left, w0, w1);
        __syncthreads();
    }
}

struct RahtScratch {
    uint64_t *keys_a, *keys_b;
    int32_t *vals_a, *vals_b, *rows_a;
    uint32_t *bucket_a, *bucket_b;
    void* counters;
    RahtScratch(void* scratch, int64_t n) {
        char* p = reinterpret_cast<char*>(scratch);
        keys_a = reinterpret_cast<uint64_t*>(p); p += align256(n * 8);
        keys_b = reinterpret_cast<uint64_t*>(p); p += align256(n * 8);
        vals_a = reinterpret_cast<int32_t*>(p); p += align256(n * 4);
        vals_b = reinterpret_cast<int32_t*>(p); p += align256(n * 4);
        rows_a = reinterpret_cast<int32_t*>(p); p += align256(n * 4);
        bucket_a = reinterpret_cast<uint32_t*>(p); p += align256(n * 4);
        bucket_b = reinterpret_cast<uint32_t*>(p); p += align256(n * 4);
        counters = p;
    }
};

}  // namespace pcc

using namespace pcc;

extern "C" {

int64_t pcc_raht_scratch_bytes(int64_t n) {
    if (n < 1) n = 1;
    return 2 * align256(n * 8) + 5 * align256(n * 4) + radix_sort_counter_bytes(n) + 256;
}

int pcc_raht_plan(const int32_t* coords, int64_t n, const int32_t* origin, int32_t depth, int32_t* perm, int32_t* step, int32_t* left,
                  int32_t* w0, int32_t* w1, int32_t* step_rows, int32_t* step_offsets, int32_t* status, void* scratch,
                  int64_t scratch_bytes, void* stream) {
    PCC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "pcc_raht_plan: bad row count %lld", (long long)n);
    PCC_REQUIRE(depth >= 0 && depth <= RAHT_MAX_DEPTH, "pcc_raht_plan: depth %d outside 0..%d", depth, RAHT_MAX_DEPTH);
    PCC_REQUIRE(coords && origin && perm && step && left && w0 && w1 && step_rows && step_offsets && status && scratch,
                "pcc_raht_plan: null coordinates, origin, output, status or scratch");
    PCC_REQUIRE(scratch_bytes >= pcc_raht_scratch_bytes(n), "pcc_raht_plan: scratch of %lld bytes, needs %lld", (long long)scratch_bytes,
                (long long)pcc_raht_scratch_bytes(n));
    hipStream_t st = as_stream(stream);
    const RahtScratch S(scratch, n);
    const unsigned nb = blocks_for(n, RAHT_BLOCK);
    PCC_CHECK_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(raht_keys_kernel, dim3(nb), dim3(RAHT_BLOCK), 0, st, coords, n, origin[0], origin[1], origin[2], depth, S.keys_a, status);
    const uint64_t* sorted = S.keys_a;
    if (depth > 0) {
        const int rc = radix_sort_pairs_u64(S.keys_a, S.keys_b, S.vals_a, S.vals_b, true, n, 0, 3 * depth, S.counters, st);
        if (rc) return rc;
        const bool in_b = radix_sort_result_in_b(0, 3 * depth);
        sorted = in_b ? S.keys_b : S.keys_a;
        PCC_CHECK_HIP(hipMemcpyAsync(perm, in_b ? S.vals_b : S.vals_a, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    } else {
        PCC_CHECK_HIP(hipMemsetAsync(perm, 0, (size_t)n * 4, st));      // every key is 0: one voxel, or duplicates (reported)
    }
    hipLaunchKernelGGL(raht_plan_kernel, dim3(nb), dim3(RAHT_BLOCK), 0, st, sorted, n, step, left, w0, w1, S.bucket_a, status);
    // rows in order of (step, row): one stable pass over the 6-bit bucket keys; the result of an odd number of passes is in *_b
    {
        const int rc = radix_sort_pairs_u32(S.bucket_a, S.bucket_b, S.rows_a, step_rows, true, n, 0, 6, S.counters, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(raht_offsets_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)S.bucket_b, n, 3 * depth, step_offsets);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_raht_transform(double* values, int64_t n, int32_t c, const int32_t* left, const int32_t* w0, const int32_t* w1,
                       const int32_t* step_rows, const int32_t* step_offsets_host, int32_t depth, int32_t inverse, void* stream) {
    PCC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "pcc_raht_transform: bad row count %lld", (long long)n);
    PCC_REQUIRE(c >= 1 && c <= RAHT_MAX_CHANNELS, "pcc_raht_transform: %d channels outside 1..%d", c, RAHT_MAX_CHANNELS);
    PCC_REQUIRE(depth >= 0 && depth <= RAHT_MAX_DEPTH, "pcc_raht_transform: depth %d outside 0..%d", depth, RAHT_MAX_DEPTH);
    PCC_REQUIRE(inverse == 0 || inverse == 1, "pcc_raht_transform: inverse %d is neither 0 nor 1", inverse);
    PCC_REQUIRE(values && left && w0 && w1 && step_rows && step_offsets_host, "pcc_raht_transform: null values or plan");
    const int nsteps = 3 * depth;
    PCC_REQUIRE(step_offsets_host[0] == 0, "pcc_raht_transform: step_offsets[0] = %d, not 0", step_offsets_host[0]);
    for (int s = 0; s < nsteps; ++s)
        PCC_REQUIRE(step_offsets_host[s] <= step_offsets_host[s + 1] && step_offsets_host[s + 1] <= n,
                    "pcc_raht_transform: step_offsets[%d] = %d after %d with %lld rows", s + 1, step_offsets_host[s + 1], step_offsets_host[s],
                    (long long)n);
    hipStream_t st = as_stream(stream);
    // the steps from `fold` upward have at most RAHT_FOLD_ROWS rows each: one launch for all of them
    RahtOffsets off;
    for (int s = 0; s <= nsteps; ++s) off.at[s] = step_offsets_host[s];
    int fold = nsteps;
    while (fold > 0 && off.at[fold] - off.at[fold - 1] <= RAHT_FOLD_ROWS) --fold;
    const bool folded = nsteps - fold >= 2 && off.at[nsteps] > off.at[fold];
    if (!folded) fold = nsteps;
    if (inverse && folded)
        hipLaunchKernelGGL(raht_fold_kernel<true>, dim3(1), dim3(RAHT_FOLD_BLOCK), 0, st, values, n, (int)c, step_rows, off, fold, nsteps, left, w0, w1);
    for (int k = 0; k < fold; ++k) {
        const int s = inverse ? fold - 1 - k : k;
        const int64_t m = (int64_t)off.at[s + 1] - off.at[s];
        if (m == 0) continue;
        const dim3 grid(blocks_for(m * c, RAHT_BLOCK));
        if (inverse)
            hipLaunchKernelGGL(raht_step_kernel<true>, grid, dim3(RAHT_BLOCK), 0, st, values, n, (int)c, step_rows + off.at[s], m, left, w0, w1);
        else
            hipLaunchKernelGGL(raht_step_kernel<false>, grid, dim3(RAHT_BLOCK), 0, st, values, n, (int)c, step_rows + off.at[s], m, left, w0, w1);
    }
    if (!inverse && folded)
        hipLaunchKernelGGL(raht_fold_kernel<false>, dim3(1), dim3(RAHT_FOLD_BLOCK), 0, st, values, n, (int)c, step_rows, off, fold, nsteps, left, w0, w1);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
