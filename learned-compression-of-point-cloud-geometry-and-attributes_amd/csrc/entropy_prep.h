// What the entropy models code for one latent element: the table index of a scale and the integer symbol.  One statement of
// each, shared by the kernels that write the planes (entropy.hip) and by the ones that only add up what the planes would cost
// (code_length.hip): an estimate is exact only while both derive the same symbol under the same table.
#pragma once
#include "common.h"

namespace pcc {

constexpr float SCALE_BOUND = 0.11f;

// index of max(scale, 0.11) in the ascending table `tb` of `levels` scales: the number of entries below it, at most levels - 1
__device__ __forceinline__ int gc_scale_index(float scale, const float* tb, int levels) {
    scale = fmaxf(scale, SCALE_BOUND);
    int ix = levels - 1;
    for (int i = 0; i < levels - 1; ++i) ix -= (scale <= tb[i]) ? 1 : 0;
    return ix;
}

// the Gaussian conditional's symbol of y under its mean, and the factorized model's of z under its channel's median
__device__ __forceinline__ float gc_symbol_f(float y, float mean) { return rintf(y - mean); }
__device__ __forceinline__ int32_t gc_symbol(float y, float mean) { return (int32_t)gc_symbol_f(y, mean); }
__device__ __forceinline__ float eb_symbol_f(float z, float median) { return rintf(z - median); }

}  // namespace pcc
