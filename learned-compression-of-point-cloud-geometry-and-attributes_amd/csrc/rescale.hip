// Position scaling: lossy geometry the way a conventional coder makes it.  Integer voxel coordinates are quantised by a rational
// scale s = num / den <= 1 onto a cell lattice, the cells are what gets coded, and a decoder scales them back to positions on the
// original grid.  The arithmetic is the contract of include/pcc_hip.h, in integers with floor division:
//     cell(p) = floor((2 p num + den) / (2 den))        pos(c) = floor((2 c den + num) / (2 num))
//
// pcc_scaled_cells: the distinct (batch, cell) in order of first appearance with the exact Q32 attribute sums of each cell's own
// points — the first-row set of first_rows.h over an integer cell functor, then the accumulation pass of the voxelisation
// (row_fold.h).  Eight launches.
//
// pcc_scaled_transfer ("recolouring"): for every source point the cell whose POSITION is nearest to it, and per cell the exact
// attribute sums of the points that chose it.  One thread per point walks shells k = 0, 1, 2 ... of Chebyshev radius k in the
// CELL domain around cell(p) and measures true distances to pos(c) in the original domain.  Every cell of shell k differs from
// cell(p) by exactly k along some axis a, and pos is strictly increasing with pos(cell(p) - 1) < p < pos(cell(p) + 1), so its
// squared distance is at least
//     L(k) = min over a of min((pos(c0_a + k) - p_a)^2, (p_a - pos(c0_a - k))^2),
// which does not decrease with k.  The walk stops before shell k once best < L(k) (at best == L(k) a tie may still sit in shell
// k).  Shell 0 is the point's own cell, which is in the set, so the walk always ends: there is no maximum radius and no retry on
// the host.  Equidistant candidates resolve to the smallest (x, y, z) — pos is monotone, so that is the smallest cell key, the
// rule of pcc_nn_search.  A cell of another batch item has another key and is never found.  Two launches (clear, walk).
#include "common.h"
#include "first_rows.h"
#include "row_fold.h"

namespace pcc {

constexpr int RESCALE_BLOCK = 256;
constexpr int SCALE_MAX = 255;

// floor(a / b) for b > 0 (C++ division truncates towards zero)
__host__ __device__ __forceinline__ int floor_div(int a, int b) {
    const int q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

// 32-bit arithmetic throughout (a 64-bit division is emulated at several times the cost): with |p| <= COORD_LIMIT and den <= 255,
// |2 p num + den| < 2^27; |cell| <= |p|, and the walk leaves a point's own cell by fewer than 8 steps (per axis its own position
// is within d = den / (2 num) + 1 of it, so best <= 3 d^2, and L(k) >= (k den / num - 1 - d)^2), so |2 c den + num| < 2^27 too.
__host__ __device__ __forceinline__ int scaled_cell(int p, int num, int den) { return floor_div(2 * p * num + den, 2 * den); }
__host__ __device__ __forceinline__ int scaled_pos(int c, int num, int den) { return floor_div(2 * c * den + num, 2 * num); }

struct Scaler {
    const int32_t* coords;    // [n, 4] (batch, x, y, z)
    const float* attr;        // [n, c]
    int c;
    int num, den;
    static constexpr int shift = 0;      // the output set has tensor stride 1
    static constexpr int REJECT = 1 << 30;
    __device__ __forceinline__ int cell(int p) const {
        return ((unsigned)(p + COORD_LIMIT) <= 2u * COORD_LIMIT) ? scaled_cell(p, num, den) : REJECT;      // |cell| <= |p|: s <= 1
    }
    __device__ __forceinline__ int4 get(int64_t i) const {
        const int4 p = reinterpret_cast<const int4*>(coords)[i];
        if ((unsigned)p.x > (unsigned)BATCH_LIMIT) return make_int4(-1, REJECT, REJECT, REJECT);
        return make_int4(p.x, cell(p.y), cell(p.z), cell(p.w));
    }
    // a point with a coordinate out of range, a batch index beyond the key's or an attribute that is not finite or exceeds 1 in
    // magnitude raises the error word and takes no part in the set (slot_of = mask + 1)
    __device__ __forceinline__ bool ok(int64_t i, bool ok) const { return attributes_ok(attr, c, i, ok); }
};

// the accumulation pass of the voxelisation (voxelize.hip), over the cell rows
__global__ __launch_bounds__(RESCALE_BLOCK) void scaled_accumulate_kernel(int64_t n, const float* __restrict__ attr, int c,
                                                                          const int32_t* __restrict__ vals, uint32_t mask,
                                                                          const int32_t* __restrict__ slot_of, int32_t* __restrict__ out_row,
                                                                          int32_t* __restrict__ out_npts, int64_t* __restrict__ out_sum) {
    // (no early return: the lanes behind the last point of a ragged wave take part in the shuffles, as runs of their own)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t row = -1;
    if (i < n) {
        const uint32_t slot = (uint32_t)slot_of[i];
        if (slot <= mask) row = vals[slot];
        out_row[i] = row;
    }
    fold_accumulate(row, i, attr, c, out_npts, out_sum);
}

__global__ __launch_bounds__(RESCALE_BLOCK) void scaled_clear_kernel(int64_t m, int c, int32_t* __restrict__ out_npts,
                                                                     int64_t* __restrict__ out_sum) {
    const int64_t total = m * (c + 1);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < m) out_npts[i] = 0;
        else out_sum[i - m] = 0;
    }
}

__device__ __forceinline__ int64_t sq(int64_t v) { return v * v; }
__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(RESCALE_BLOCK) void scaled_transfer_kernel(const int32_t* __restrict__ coords, int64_t n,
                                                                        const float* __restrict__ attr, int c, int num, int den,
                                                                        const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                                        uint64_t mask, int32_t m, int32_t* __restrict__ out_nearest,
                                                                        int64_t* __restrict__ out_d2, int32_t* __restrict__ out_npts,
                                                                        int64_t* __restrict__ out_sum) {
    // (no early return: every lane reaches fold_accumulate, converged)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t best_idx = -1;
    int64_t best = INT64_MAX;
    if (i < n) {
        const int4 p = reinterpret_cast<const int4*>(coords)[i];
        if (coord_in_range(p.x, p.y, p.z, p.w)) {
            const int c0x = scaled_cell(p.y, num, den), c0y = scaled_cell(p.z, num, den), c0z = scaled_cell(p.w, num, den);
            uint64_t best_key = KEY_EMPTY;
            for (int k = 0;; ++k) {
                if (k > 0) {
                    // shell 0 missed: (keys, vals) is not the table of these points' cells.  Nothing to walk towards.
                    if (best_idx < 0) break;
                    int64_t bound = sq(scaled_pos(c0x + k, num, den) - p.y);
                    bound = min64(bound, sq(p.y - scaled_pos(c0x - k, num, den)));
                    bound = min64(bound, sq(scaled_pos(c0y + k, num, den) - p.z));
                    bound = min64(bound, sq(p.z - scaled_pos(c0y - k, num, den)));
                    bound = min64(bound, sq(scaled_pos(c0z + k, num, den) - p.w));
                    bound = min64(bound, sq(p.w - scaled_pos(c0z - k, num, den)));
                    if (best < bound) break;
                }
                for (int dx = -k; dx <= k; ++dx) {
                    const int cx = c0x + dx;
                    const int64_t ex = sq(scaled_pos(cx, num, den) - p.y);
                    if (ex > best) continue;
                    const bool fx = dx == -k || dx == k;
                    for (int dy = -k; dy <= k; ++dy) {
                        const int cy = c0y + dy;
                        const int64_t exy = ex + sq(scaled_pos(cy, num, den) - p.z);
                        if (exy > best) continue;
                        const bool fy = fx || dy == -k || dy == k;
                        const int step = fy ? 1 : (k > 0 ? 2 * k : 1);      // interior columns: only the two end caps
                        for (int dz = -k; dz <= k; dz += step) {
                            const int cz = c0z + dz;
                            const int64_t d2 = exy + sq(scaled_pos(cz, num, den) - p.w);
                            if (d2 > best || !coord_in_range(p.x, cx, cy, cz)) continue;      // (a cell out of range is in no set)
                            const uint64_t key = pack_key(p.x, cx, cy, cz);
                            const int idx = table_find(keys, vals, mask, 0, key);
                            if (idx < 0) continue;
                            if (d2 < best) {
                                best = d2; best_key = key; best_idx = idx;
                            } else if (key < best_key) {
                                best_key = key; best_idx = idx;
                            }
                        }
                    }
                }
            }
        }
        if ((uint32_t)best_idx >= (uint32_t)m) best_idx = -1;      // a row the accumulators do not have (a foreign table)
        out_nearest[i] = best_idx;
        out_d2[i] = best_idx >= 0 ? best : -1;
    }
    fold_accumulate(best_idx, i, attr, c, out_npts, out_sum);
}

static int check_scale(const char* who, int32_t num, int32_t den, int32_t c) {
    PCC_REQUIRE(num >= 1 && num <= den && den <= SCALE_MAX, "%s: the scale %d / %d is not 1 <= num <= den <= %d", who, num, den, SCALE_MAX);
    PCC_REQUIRE(c >= 0 && c <= FOLD_MAX_CHANNELS, "%s: %d attribute channels outside 0..%d", who, c, FOLD_MAX_CHANNELS);
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;

extern "C" {

int pcc_scaled_cells(const int32_t* coords, int64_t n, const float* attr, int32_t c, int32_t num, int32_t den, uint64_t* keys,
                     int32_t* vals, int64_t cap, int32_t* scratch, int32_t* out_coords, int32_t* out_first, int32_t* out_npts,
                     int64_t* out_sum, int32_t* out_row, int64_t* out_count, void* stream) {
    PCC_REQUIRE(n >= 0 && n < (1ll << 31) - 1, "pcc_scaled_cells: bad point count %lld", (long long)n);
    if (const int rc = check_scale("pcc_scaled_cells", num, den, c)) return rc;
    PCC_REQUIRE(cap > 0 && (cap & (cap - 1)) == 0 && cap >= 2 * n && cap <= (1ll << 31), "pcc_scaled_cells: bad capacity %lld for n=%lld",
                (long long)cap, (long long)n);
    PCC_REQUIRE(keys && vals && scratch && out_count, "pcc_scaled_cells: null table, scratch or count");
    PCC_REQUIRE(n == 0 || (coords && out_coords && out_first && out_npts && out_row), "pcc_scaled_cells: null points or outputs");
    PCC_REQUIRE(n == 0 || c == 0 || (attr && out_sum), "pcc_scaled_cells: null attributes or sums with c = %d", c);
    hipStream_t st = as_stream(stream);
    const int rc = first_rows_build(Scaler{coords, attr, c, num, den}, VoxelSink{c, out_first, out_npts, out_sum}, n, keys, vals, cap, scratch,
                                    out_coords, out_count, st);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(scaled_accumulate_kernel, dim3(blocks_for(n, RESCALE_BLOCK)), dim3(RESCALE_BLOCK), 0, st, n, attr, c, (const int32_t*)vals,
                       (uint32_t)(cap - 1), (const int32_t*)FirstRowsScratch(scratch, n).slot_of, out_row, out_npts, out_sum);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_scaled_transfer(const int32_t* coords, int64_t n, const float* attr, int32_t c, int32_t num, int32_t den, const uint64_t* keys,
                        const int32_t* vals, int64_t cap, int64_t m, int32_t* out_nearest, int64_t* out_d2, int32_t* out_npts,
                        int64_t* out_sum, void* stream) {
    PCC_REQUIRE(n >= 0 && n < (1ll << 31) - 1, "pcc_scaled_transfer: bad point count %lld", (long long)n);
    if (const int rc = check_scale("pcc_scaled_transfer", num, den, c)) return rc;
    PCC_REQUIRE(cap >= 2 && (cap & (cap - 1)) == 0 && cap <= (1ll << 31), "pcc_scaled_transfer: bad capacity %lld", (long long)cap);
    PCC_REQUIRE(m >= 0 && m <= n, "pcc_scaled_transfer: %lld cell rows for %lld points", (long long)m, (long long)n);
    PCC_REQUIRE(keys && vals, "pcc_scaled_transfer: null table");
    PCC_REQUIRE(n == 0 || (m >= 1 && coords && out_nearest && out_d2 && out_npts), "pcc_scaled_transfer: null points or outputs, or no cell rows");
    PCC_REQUIRE(n == 0 || c == 0 || (attr && out_sum), "pcc_scaled_transfer: null attributes or sums with c = %d", c);
    if (n == 0) return PCC_OK;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(scaled_clear_kernel, dim3(blocks_for(m * (c + 1), RESCALE_BLOCK, 4096)), dim3(RESCALE_BLOCK), 0, st, m, c, out_npts, out_sum);
    hipLaunchKernelGGL(scaled_transfer_kernel, dim3(blocks_for(n, RESCALE_BLOCK)), dim3(RESCALE_BLOCK), 0, st, coords, n, attr, c, num, den, keys,
                       vals, (uint64_t)(cap - 1), (int32_t)m, out_nearest, out_d2, out_npts, out_sum);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
