// RAHT, the region-adaptive hierarchical transform (de Queiroz & Chou 2016) of per-voxel attributes: the transform of G-PCC's
// attribute coder, here the attribute half of the octree + RAHT anchor codec (../raht.py, ../anchor.py).  The contract is in
// include/pcc_hip.h (pcc_raht_plan / pcc_raht_transform, and for region-wise quantisation pcc_raht_blocks / pcc_raht_block_levels /
// pcc_raht_coeff_levels / pcc_raht_quantize / pcc_raht_dequantize).
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

// ---- region-wise quantisation ("PCR2", ../raht.py): blocks of rows, one quantisation level per block, one per coefficient -------
// A block is the run of rows inside one cube of edge 2^block_log2: in Morton order a row opens a block iff its key differs from
// the row before it at or above bit 3 * block_log2, which is what step[i] >= 3 * block_log2 says.  The plan is all that is needed.
constexpr int RAHT_LEVELS = 64;               // quantisation levels 0 .. 63, one per Gaussian table spacing (raht.py: level_steps)

__global__ __launch_bounds__(RAHT_BLOCK) void raht_block_flags_kernel(const int32_t* __restrict__ step, int64_t n, int first_step,
                                                                      int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (i < n) flags[i] = (i > 0 && step[i] >= first_step) ? 1 : 0;
}

__global__ __launch_bounds__(64) void raht_block_count_kernel(const int32_t* __restrict__ block_of_row, int64_t n, int32_t* __restrict__ n_blocks) {
    if (blockIdx.x == 0 && threadIdx.x == 0) n_blocks[0] = block_of_row[n - 1] + 1;
}

__global__ __launch_bounds__(RAHT_BLOCK) void raht_fill_kernel(int32_t* __restrict__ out, int64_t m, int32_t value) {
    const int64_t i = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (i < m) out[i] = value;
}

// block_level[b] = min over the block's rows of levels[perm[row]].  Rows of one block are consecutive, so inside a wave the lanes
// of a block form a segment: a segmented min scan over the wave (six shuffle rounds), then the last lane of every segment sends
// one atomicMin.  Integer min only: the result does not depend on the order in which the waves arrive.
__global__ __launch_bounds__(RAHT_BLOCK) void raht_block_levels_kernel(const uint8_t* __restrict__ levels, const int32_t* __restrict__ perm,
                                                                       const int32_t* __restrict__ block_of_row, int64_t n, int64_t n_blocks,
                                                                       int32_t* __restrict__ block_level, int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int blk = -1, lvl = RAHT_LEVELS - 1;
    if (i < n) {
        const int64_t src = perm[i];
        const int64_t b = block_of_row[i];
        if ((uint64_t)src < (uint64_t)n && (uint64_t)b < (uint64_t)n_blocks) {        // a plan that is not one reads and writes nothing
            blk = (int)b;
            lvl = levels[src];
            if (lvl >= RAHT_LEVELS) { atomicAdd(&status[0], 1); lvl = RAHT_LEVELS - 1; }
        }
    }
    for (int d = 1; d < 64; d <<= 1) {
        const int other_lvl = __shfl_up(lvl, d, 64), other_blk = __shfl_up(blk, d, 64);
        if (lane >= d && other_blk == blk) lvl = min(lvl, other_lvl);
    }
    const int next_blk = __shfl_down(blk, 1, 64);
    if (blk >= 0 && (lane == 63 || next_blk != blk)) atomicMin(&block_level[blk], lvl);
}

// lev[i] = coeff_level[i] = block_level[block_of_row[i]]: the walk's working array, and the level of the rows no step owns.  One
// thread per four rows, so that the byte-wide output leaves as one 32-bit word per thread where the pointer allows it.
__global__ __launch_bounds__(RAHT_BLOCK) void raht_expand_levels_kernel(const int32_t* __restrict__ block_level, int64_t n_blocks,
                                                                        const int32_t* __restrict__ block_of_row, int64_t n,
                                                                        int32_t* __restrict__ lev, uint8_t* __restrict__ coeff_level, int word_stores) {
    const int64_t i0 = ((int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x) * 4;
    if (i0 >= n) return;
    uint32_t word = 0;
    const int rows = (int)min((int64_t)4, n - i0);
    for (int k = 0; k < rows; ++k) {
        const int64_t b = block_of_row[i0 + k];
        int v = (uint64_t)b < (uint64_t)n_blocks ? block_level[b] : RAHT_LEVELS - 1;
        v = min(max(v, 0), RAHT_LEVELS - 1);
        lev[i0 + k] = v;
        word |= (uint32_t)v << (8 * k);
    }
    if (word_stores && rows == 4) {
        *reinterpret_cast<uint32_t*>(coeff_level + i0) = word;
    } else {
        for (int k = 0; k < rows; ++k) coeff_level[i0 + k] = (uint8_t)(word >> (8 * k));
    }
}

// One pair of a step of the level walk: the coefficient of row r summarises the rows [left[r], r + w1[r]), and its level is the
// finest (smallest) level inside them; lev[left] carries the minimum of the merged node upward.  Rows as in raht_pair: within a
// step no row belongs to two pairs.
__device__ __forceinline__ void raht_level_pair(int32_t* lev, uint8_t* coeff_level, int64_t n, const int32_t* __restrict__ rows, int64_t j,
                                                const int32_t* __restrict__ left) {
    const int64_t r = rows[j];
    if ((uint64_t)r >= (uint64_t)n) return;
    const int64_t l = left[r];
    if ((uint64_t)l >= (uint64_t)n || l == r) return;
    const int m = min(lev[l], lev[r]);
    coeff_level[r] = (uint8_t)m;
    lev[l] = m;
}

__global__ __launch_bounds__(RAHT_BLOCK) void raht_level_step_kernel(int32_t* __restrict__ lev, uint8_t* __restrict__ coeff_level, int64_t n,
                                                                     const int32_t* __restrict__ rows, int64_t m, const int32_t* __restrict__ left) {
    const int64_t j = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (j < m) raht_level_pair(lev, coeff_level, n, rows, j, left);
}

// the folded top steps [lo, hi) of the walk in one workgroup, then the DC's level: lev[0] after the last step, the global minimum
__global__ __launch_bounds__(RAHT_FOLD_BLOCK) void raht_level_fold_kernel(int32_t* lev, uint8_t* coeff_level, int64_t n, const int32_t* __restrict__ step_rows,
                                                                          RahtOffsets off, int lo, int hi, const int32_t* __restrict__ left) {
    for (int s = lo; s < hi; ++s) {
        const int64_t work = off.at[s + 1] - off.at[s];
        for (int64_t j = threadIdx.x; j < work; j += RAHT_FOLD_BLOCK) raht_level_pair(lev, coeff_level, n, step_rows + off.at[s], j, left);
        __syncthreads();
    }
    if (threadIdx.x == 0) coeff_level[0] = (uint8_t)lev[0];
}

struct RahtSteps { double at[RAHT_LEVELS]; };

// thread = (row, channel): symbol = rint(coefficient / step[level of the row]), ties to even, a true division
__global__ __launch_bounds__(RAHT_BLOCK) void raht_quantize_kernel(const double* __restrict__ coeffs, int64_t n, int c, const uint8_t* __restrict__ coeff_level,
                                                                   RahtSteps steps, int32_t* __restrict__ symbols, int32_t* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (t >= n * c) return;
    const int64_t row = (t >> 32) ? t / c : (int64_t)((uint32_t)t / (uint32_t)c);
    const int level = min((int)coeff_level[row], RAHT_LEVELS - 1);
    const double q = rint(coeffs[t] / steps.at[level]);
    const bool ok = fabs(q) < 268435456.0;             // 2^28; false for a NaN too
    if (!ok) atomicAdd(&status[0], 1);
    symbols[t] = ok ? (int32_t)q : 0;
}

__global__ __launch_bounds__(RAHT_BLOCK) void raht_dequantize_kernel(const int32_t* __restrict__ symbols, int64_t n, int c, const uint8_t* __restrict__ coeff_level,
                                                                     RahtSteps steps, double* __restrict__ coeffs) {
    const int64_t t = (int64_t)blockIdx.x * RAHT_BLOCK + threadIdx.x;
    if (t >= n * c) return;
    const int64_t row = (t >> 32) ? t / c : (int64_t)((uint32_t)t / (uint32_t)c);
    const int level = min((int)coeff_level[row], RAHT_LEVELS - 1);
    coeffs[t] = (double)symbols[t] * steps.at[level];
}

static bool raht_steps_ok(const double* steps_host, RahtSteps* out) {
    for (int l = 0; l < RAHT_LEVELS; ++l) {
        if (!(steps_host[l] > 0.0) || !std::isfinite(steps_host[l])) return false;
        out->at[l] = steps_host[l];
    }
    return true;
}

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

int pcc_raht_blocks(const int32_t* step, int64_t n, int32_t block_log2, int32_t* block_of_row, int32_t* n_blocks, void* scratch,
                    int64_t scratch_bytes, void* stream) {
    PCC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "pcc_raht_blocks: bad row count %lld", (long long)n);
    PCC_REQUIRE(block_log2 >= 0 && block_log2 <= RAHT_MAX_DEPTH, "pcc_raht_blocks: block_log2 %d outside 0..%d", block_log2, RAHT_MAX_DEPTH);
    PCC_REQUIRE(step && block_of_row && n_blocks && scratch, "pcc_raht_blocks: null step, output or scratch");
    PCC_REQUIRE(scratch_bytes >= pcc_raht_scratch_bytes(n), "pcc_raht_blocks: scratch of %lld bytes, needs %lld", (long long)scratch_bytes,
                (long long)pcc_raht_scratch_bytes(n));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(raht_block_flags_kernel, dim3(blocks_for(n, RAHT_BLOCK)), dim3(RAHT_BLOCK), 0, st, step, n, 3 * (int)block_log2, block_of_row);
    // the inclusive scan of the block-start flags, in place: row 0 carries no flag, so the sums are the block indices
    const int rc = scan_flags(block_of_row, n, block_of_row, reinterpret_cast<int32_t*>(scratch), nullptr, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(raht_block_count_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)block_of_row, n, n_blocks);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_raht_block_levels(const uint8_t* levels, const int32_t* perm, const int32_t* block_of_row, int64_t n, int64_t n_blocks,
                          int32_t* block_level, int32_t* status, void* stream) {
    PCC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "pcc_raht_block_levels: bad row count %lld", (long long)n);
    PCC_REQUIRE(n_blocks >= 1 && n_blocks <= n, "pcc_raht_block_levels: %lld blocks for %lld rows", (long long)n_blocks, (long long)n);
    PCC_REQUIRE(levels && perm && block_of_row && block_level && status, "pcc_raht_block_levels: null levels, plan, output or status");
    hipStream_t st = as_stream(stream);
    PCC_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(raht_fill_kernel, dim3(blocks_for(n_blocks, RAHT_BLOCK)), dim3(RAHT_BLOCK), 0, st, block_level, n_blocks, RAHT_LEVELS - 1);
    hipLaunchKernelGGL(raht_block_levels_kernel, dim3(blocks_for(n, RAHT_BLOCK)), dim3(RAHT_BLOCK), 0, st, levels, perm, block_of_row, n, n_blocks,
                       block_level, status);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_raht_coeff_levels(const int32_t* block_level, const int32_t* block_of_row, int64_t n, int64_t n_blocks, const int32_t* left,
                          const int32_t* step_rows, const int32_t* step_offsets_host, int32_t depth, uint8_t* coeff_level, int32_t* lev,
                          void* stream) {
    PCC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "pcc_raht_coeff_levels: bad row count %lld", (long long)n);
    PCC_REQUIRE(n_blocks >= 1 && n_blocks <= n, "pcc_raht_coeff_levels: %lld blocks for %lld rows", (long long)n_blocks, (long long)n);
    PCC_REQUIRE(depth >= 0 && depth <= RAHT_MAX_DEPTH, "pcc_raht_coeff_levels: depth %d outside 0..%d", depth, RAHT_MAX_DEPTH);
    PCC_REQUIRE(block_level && block_of_row && left && step_rows && step_offsets_host && coeff_level && lev,
                "pcc_raht_coeff_levels: null levels, plan, output or scratch");
    const int nsteps = 3 * depth;
    PCC_REQUIRE(step_offsets_host[0] == 0, "pcc_raht_coeff_levels: step_offsets[0] = %d, not 0", step_offsets_host[0]);
    for (int s = 0; s < nsteps; ++s)
        PCC_REQUIRE(step_offsets_host[s] <= step_offsets_host[s + 1] && step_offsets_host[s + 1] <= n,
                    "pcc_raht_coeff_levels: step_offsets[%d] = %d after %d with %lld rows", s + 1, step_offsets_host[s + 1], step_offsets_host[s],
                    (long long)n);
    hipStream_t st = as_stream(stream);
    const int word_stores = (reinterpret_cast<uintptr_t>(coeff_level) & 3) == 0;
    hipLaunchKernelGGL(raht_expand_levels_kernel, dim3(blocks_for((n + 3) / 4, RAHT_BLOCK)), dim3(RAHT_BLOCK), 0, st, block_level, n_blocks,
                       block_of_row, n, lev, coeff_level, word_stores);
    // the launch plan of pcc_raht_transform (forward): one launch per non-empty step, the small steps at the top in one workgroup
    RahtOffsets off;
    for (int s = 0; s <= nsteps; ++s) off.at[s] = step_offsets_host[s];
    int fold = nsteps;
    while (fold > 0 && off.at[fold] - off.at[fold - 1] <= RAHT_FOLD_ROWS) --fold;
    if (nsteps - fold < 2 || off.at[nsteps] == off.at[fold]) fold = nsteps;
    for (int s = 0; s < fold; ++s) {
        const int64_t m = (int64_t)off.at[s + 1] - off.at[s];
        if (m == 0) continue;
        hipLaunchKernelGGL(raht_level_step_kernel, dim3(blocks_for(m, RAHT_BLOCK)), dim3(RAHT_BLOCK), 0, st, lev, coeff_level, n, step_rows + off.at[s], m, left);
    }
    // (with nothing folded the launch runs no step and only writes the DC's level)
    hipLaunchKernelGGL(raht_level_fold_kernel, dim3(1), dim3(RAHT_FOLD_BLOCK), 0, st, lev, coeff_level, n, step_rows, off, fold, nsteps, left);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_raht_quantize(const double* coeffs, int64_t n, int32_t c, const uint8_t* coeff_level, const double* steps_host, int32_t* symbols,
                      int32_t* status, void* stream) {
    PCC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "pcc_raht_quantize: bad row count %lld", (long long)n);
    PCC_REQUIRE(c >= 1 && c <= RAHT_MAX_CHANNELS, "pcc_raht_quantize: %d channels outside 1..%d", c, RAHT_MAX_CHANNELS);
    PCC_REQUIRE(coeffs && coeff_level && steps_host && symbols && status, "pcc_raht_quantize: null coefficients, levels, steps, output or status");
    RahtSteps steps;
    PCC_REQUIRE(raht_steps_ok(steps_host, &steps), "pcc_raht_quantize: a step of the table is not a positive finite number");
    hipStream_t st = as_stream(stream);
    PCC_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(raht_quantize_kernel, dim3(blocks_for(n * c, RAHT_BLOCK)), dim3(RAHT_BLOCK), 0, st, coeffs, n, (int)c, coeff_level, steps, symbols, status);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_raht_dequantize(const int32_t* symbols, int64_t n, int32_t c, const uint8_t* coeff_level, const double* steps_host, double* coeffs,
                        void* stream) {
    PCC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "pcc_raht_dequantize: bad row count %lld", (long long)n);
    PCC_REQUIRE(c >= 1 && c <= RAHT_MAX_CHANNELS, "pcc_raht_dequantize: %d channels outside 1..%d", c, RAHT_MAX_CHANNELS);
    PCC_REQUIRE(symbols && coeff_level && steps_host && coeffs, "pcc_raht_dequantize: null symbols, levels, steps or output");
    RahtSteps steps;
    PCC_REQUIRE(raht_steps_ok(steps_host, &steps), "pcc_raht_dequantize: a step of the table is not a positive finite number");
    hipLaunchKernelGGL(raht_dequantize_kernel, dim3(blocks_for(n * c, RAHT_BLOCK)), dim3(RAHT_BLOCK), 0, as_stream(stream), symbols, n, (int)c, coeff_level,
                       steps, coeffs);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
