// Exact per-row accumulation of point attributes: every point adds 1 to out_npts[row] and the Q32 fixed point of each of its
// attribute channels to out_sum[row, ch], with integer atomics only (integer addition commutes: any schedule gives the same
// bytes).  Shared by the voxelisation (voxelize.hip: row = the point's own voxel) and the position scaling (rescale.hip: row = the
// point's own cell, or the cell whose reconstructed position is nearest).
//
// Clouds arrive spatially coherent, and many adders on one destination serialise, so a wave first folds every run of consecutive
// lanes with the same row into its first lane (a segmented shuffle reduction, skipped by a wave-uniform branch when no two
// neighbouring lanes share a row) and only run heads issue atomics.
// The functions are static or inline: the header is compiled into more than one object.
#pragma once
#include "common.h"

namespace pcc {

constexpr int FOLD_MAX_CHANNELS = 16;

// The winner of a first-row set (first_rows.h) records its point and zeroes the accumulators of its row: the caller hands over
// uninitialised buffers, and only the rows in use are touched.
struct VoxelSink {
    int c;
    int32_t *out_first, *out_npts;
    int64_t* out_sum;
    __device__ __forceinline__ void operator()(int32_t row, int64_t i) const {
        out_first[row] = (int32_t)i;
        out_npts[row] = 0;
        for (int ch = 0; ch < c; ++ch) out_sum[(int64_t)row * c + ch] = 0;
    }
};

// the validity test of a point's attributes: finite and at most 1 in magnitude (false for NaN)
__device__ __forceinline__ bool attributes_ok(const float* __restrict__ attr, int c, int64_t i, bool ok) {
    for (int ch = 0; ch < c; ++ch) ok = ok && (fabsf(attr[i * c + ch]) <= 1.0f);
    return ok;
}

// sum of v over lanes [lane, end) of the wave, `end` = one past the last lane of this lane's run; every lane takes part
__device__ __forceinline__ int64_t run_sum(int64_t v, int lane, int end) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = __shfl_down(v, d, 64);
        if (lane + d < end) v += o;
    }
    return v;
}

// Point i (attributes attr[i, 0..c)) adds itself to `row`; row < 0 (no point behind the end of a ragged wave, or a rejected one)
// adds nothing.  EVERY lane of the wave must call this, converged: the lanes without a point take part in the shuffles, as runs
// of their own, and attr is read only where row >= 0.
__device__ __forceinline__ void fold_accumulate(int32_t row, int64_t i, const float* __restrict__ attr, int c,
                                                int32_t* __restrict__ out_npts, int64_t* __restrict__ out_sum) {
    const int lane = threadIdx.x & 63;
    const int32_t before = __shfl_up(row, 1, 64);
    const bool head = lane == 0 || before != row || row < 0;
    const uint64_t heads = __ballot(head);
    if (heads == ~0ull) {                              // wave-uniform: no two neighbouring lanes share a row
        if (row >= 0) {
            atomicAdd(&out_npts[row], 1);
            for (int ch = 0; ch < c; ++ch) {
                const int64_t q = llrint((double)attr[i * c + ch] * 4294967296.0);
                atomicAdd(reinterpret_cast<unsigned long long*>(&out_sum[(int64_t)row * c + ch]), (unsigned long long)q);
            }
        }
        return;
    }
    const uint64_t above = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int end = above ? lane + 1 + __builtin_ctzll(above) : 64;      // the next head, or the end of the wave
    const bool adds = head && row >= 0;
    if (adds) atomicAdd(&out_npts[row], end - lane);
    for (int ch = 0; ch < c; ++ch) {
        const int64_t q = row >= 0 ? llrint((double)attr[i * c + ch] * 4294967296.0) : 0;
        const int64_t s = run_sum(q, lane, end);
        if (adds) atomicAdd(reinterpret_cast<unsigned long long*>(&out_sum[(int64_t)row * c + ch]), (unsigned long long)s);
    }
}

}  // namespace pcc
