// Voxelisation: N points (float xyz, optional batch index, optional C attribute channels) onto a voxel grid -> the distinct voxels
// in order of first appearance, per voxel the point count and the EXACT sum of its attributes (Q32 fixed point in int64), per
// point its voxel row.  The arithmetic is the contract of include/pcc_hip.h (pcc_voxelize): per axis (p - origin) / voxel, every
// operation rounded separately in fp32 (the file is compiled with -ffp-contract=off; the division is hipcc's default correctly
// rounded one, not a multiplication by a reciprocal), then floorf or rintf.  A quotient that is not finite or lies beyond the key
// range is never converted to an integer.
//
// The coordinate set is the first-row set of first_rows.h (seven launches); every winner also records its point and zeroes its
// accumulators.  Then ONE accumulation pass over the points: row = vals[slot_of[i]], integer atomic adds into out_npts / out_sum.
// Integer addition commutes, so the bytes do not depend on the schedule; there is no
// float atomic anywhere.  The adds go through the in-wave fold of equal rows that row_fold.h describes (fold_accumulate), shared
// with the position scaling (rescale.hip).  Eight launches.
#include "common.h"
#include "first_rows.h"
#include "row_fold.h"

namespace pcc {

constexpr int VOX_BLOCK = 256;
constexpr int VOX_MAX_CHANNELS = FOLD_MAX_CHANNELS;

struct Voxelizer {
    const float* xyz;         // [n, 3]
    const int32_t* batch;     // [n] or null = item 0
    const float* attr;        // [n, c]
    int c;
    int nbatch;
    float ox, oy, oz, voxel;
    int rounding;             // 0 floorf, 1 rintf (ties to even)
    static constexpr int shift = 0;      // the output set has tensor stride 1
    static constexpr int REJECT = 1 << 30;
    __device__ __forceinline__ int cell(float p, float o) const {
        const float g = (p - o) / voxel;
        const float r = rounding ? rintf(g) : floorf(g);
        return (fabsf(r) <= (float)COORD_LIMIT) ? (int)r : REJECT;      // false for NaN and infinities
    }
    __device__ __forceinline__ int4 get(int64_t i) const {
        const int b = batch ? batch[i] : 0;
        if ((unsigned)b >= (unsigned)nbatch) return make_int4(-1, REJECT, REJECT, REJECT);
        return make_int4(b, cell(xyz[3 * i], ox), cell(xyz[3 * i + 1], oy), cell(xyz[3 * i + 2], oz));
    }
    // a point with a cell out of range, a batch index without an item or an attribute that is not finite or exceeds 1 in magnitude
    // raises the error word and takes no part in the set (slot_of = mask + 1)
    __device__ __forceinline__ bool ok(int64_t i, bool ok) const {
        return attributes_ok(attr, c, i, ok);
    }
};

__global__ __launch_bounds__(VOX_BLOCK) void voxelize_accumulate_kernel(int64_t n, const float* __restrict__ attr, int c,
                                                                        const int32_t* __restrict__ vals, uint32_t mask,
                                                                        const int32_t* __restrict__ slot_of, int32_t* __restrict__ out_row,
                                                                        int32_t* __restrict__ out_npts, int64_t* __restrict__ out_sum) {
    // (no early return: the lanes behind the last point of a ragged wave take part in the shuffles, as runs of their own)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t row = -1;                                  // no point, or a rejected one: adds nothing
    if (i < n) {
        const uint32_t slot = (uint32_t)slot_of[i];
        if (slot <= mask) row = vals[slot];
        out_row[i] = row;
    }
    fold_accumulate(row, i, attr, c, out_npts, out_sum);
}

}  // namespace pcc

using namespace pcc;

extern "C" {

int pcc_voxelize(const float* xyz, const int32_t* batch, int64_t n, int32_t nbatch, const float* attr, int32_t c, float ox, float oy,
                 float oz, float voxel, int32_t rounding, uint64_t* keys, int32_t* vals, int64_t cap, int32_t* scratch,
                 int32_t* out_coords, int32_t* out_first, int32_t* out_npts, int64_t* out_sum, int32_t* out_row, int64_t* out_count,
                 void* stream) {
    PCC_REQUIRE(n >= 0 && n < (1ll << 31) - 1, "pcc_voxelize: bad point count %lld", (long long)n);
    PCC_REQUIRE(nbatch >= 1 && nbatch <= BATCH_LIMIT + 1, "pcc_voxelize: nbatch %d outside 1..%d", nbatch, BATCH_LIMIT + 1);
    PCC_REQUIRE(c >= 0 && c <= VOX_MAX_CHANNELS, "pcc_voxelize: %d attribute channels outside 0..%d", c, VOX_MAX_CHANNELS);
    PCC_REQUIRE(voxel > 0.0f && voxel <= 3.0e38f, "pcc_voxelize: the voxel size must be a positive finite number (got %g)", (double)voxel);
    PCC_REQUIRE(ox - ox == 0.0f && oy - oy == 0.0f && oz - oz == 0.0f, "pcc_voxelize: the origin is not finite");
    PCC_REQUIRE(rounding == 0 || rounding == 1, "pcc_voxelize: rounding %d is neither 0 (floor) nor 1 (nearest, ties to even)", rounding);
    PCC_REQUIRE(cap > 0 && (cap & (cap - 1)) == 0 && cap >= 2 * n && cap <= (1ll << 31), "pcc_voxelize: bad capacity %lld for n=%lld",
                (long long)cap, (long long)n);
    PCC_REQUIRE(keys && vals && scratch && out_count, "pcc_voxelize: null table, scratch or count");
    PCC_REQUIRE(n == 0 || (xyz && out_coords && out_first && out_npts && out_row), "pcc_voxelize: null points or outputs");
    PCC_REQUIRE(n == 0 || c == 0 || (attr && out_sum), "pcc_voxelize: null attributes or sums with c = %d", c);
    hipStream_t st = as_stream(stream);
    const int rc = first_rows_build(Voxelizer{xyz, batch, attr, c, nbatch, ox, oy, oz, voxel, rounding}, VoxelSink{c, out_first, out_npts, out_sum},
                                    n, keys, vals, cap, scratch, out_coords, out_count, st);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(voxelize_accumulate_kernel, dim3(blocks_for(n, VOX_BLOCK)), dim3(VOX_BLOCK), 0, st, n, attr, c, (const int32_t*)vals,
                       (uint32_t)(cap - 1), (const int32_t*)FirstRowsScratch(scratch, n).slot_of, out_row, out_npts, out_sum);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
