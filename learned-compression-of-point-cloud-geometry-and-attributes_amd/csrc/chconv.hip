// Channelwise (depthwise) window convolution on one coordinate set (ME.MinkowskiChannelwiseConvolution, stride 1: the window
// sums of the reference's ColorSSIM loss, loss.py:204-206, 391-453) and its adjoint, in one kernel that probes the set's
// hashed-voxel table and accumulates without a stored neighbour table: an [N, ksize^3] table at window 11 would be 5.3 KB per
// row on sets of one to two million rows.
//
//   y[i, ch] = sum over the offsets (dx, dy, dz) in [-h, h]^3, h = ksize / 2, whose voxel exists in the set:
//              w[k', ch] * x[row(coords[i] + (dx, dy, dz) * tensor_stride), ch]
//   k = (dx + h) + ksize (dy + h) + ksize^2 (dz + h);  k' = k (flip = 0) or ksize^3 - 1 - k (flip = 1: the adjoint)
//
// Accumulation order (fixed; the same for flip 0 and 1, for every launch and every row count): an output element starts at
// +0 and adds its present neighbours' products one at a time in ascending p = (dz + h) + ksize (dy + h) + ksize^2 (dx + h),
// i.e. z fastest, then y, then x.  Every product is rounded to fp32 before it is added: separate multiply and add, no fused
// multiply-add (the library is built with -ffp-contract=off).  No atomics.
//
// Shape of the kernel.  A wave owns two rows.  Probe phase: its 64 lanes probe 64 consecutive p of one row — adjacent lanes
// probe adjacent dz, and the table keeps the 8 voxels of an aligned z-run in one 64-byte line of `keys` (common.h) — and the
// hits are compacted IN ORDER (ballot + prefix popcount, no atomics) into the row's queue in LDS: (row id, k') pairs.
// Accumulate phase: lanes 0-31 take the first row's queue, lanes 32-63 the second's, a lane per channel, so a queue entry is
// one 128-byte read of a 32-channel row.  The two phases alternate over segments of 256 offsets, which bounds the queues at
// 3 KB per wave for every window size; the window itself is read from global memory (5.3 KB at 11^3 x 1 channel stays in the
// vector cache; 170 KB at 11^3 x 32 channels cannot sit in LDS whole and is served by L2).
#include "common.h"

namespace pcc {

constexpr int CHCONV_SEG = 256;              // offsets probed per segment and row = capacity of a row's queue
constexpr int CHCONV_WAVES = 4;              // waves per workgroup, two rows each

template <int KS>
__global__ __launch_bounds__(64 * CHCONV_WAVES) void chconv_kernel(
    const float* __restrict__ x, int n, int c, const int32_t* __restrict__ coords, const uint64_t* __restrict__ keys,
    const int32_t* __restrict__ vals, uint64_t mask, int shift, int ts, const float* __restrict__ w, int w_channels, int flip,
    float* __restrict__ y) {
    constexpr int K = KS * KS * KS, H = KS / 2;
    __shared__ int32_t q_row[CHCONV_WAVES][2][CHCONV_SEG];
    __shared__ uint16_t q_k[CHCONV_WAVES][2][CHCONV_SEG];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * CHCONV_WAVES + wave) * 2;
    const int half = lane >> 5, ch = lane & 31;
    const int64_t my_row = row0 + half;
    const bool out_lane = my_row < n && ch < c;
    const int wch = (w_channels == 1) ? 0 : ch;
    float acc = 0.0f;
    for (int seg = 0; seg < K; seg += CHCONV_SEG) {
        int count[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const bool row_ok = row0 + r < n;                         // wave-uniform
            const int4 cr = row_ok ? reinterpret_cast<const int4*>(coords)[row0 + r] : make_int4(0, 0, 0, 0);
            int base = 0;
            for (int p0 = seg; p0 < K && p0 < seg + CHCONV_SEG; p0 += 64) {
                const int p = p0 + lane;
                int id = -1, kk = 0;
                if (row_ok && p < K) {
                    const int iz = p % KS, iy = (p / KS) % KS, ix = p / (KS * KS);
                    const int k = ix + KS * iy + KS * KS * iz;
                    kk = flip ? K - 1 - k : k;
                    const int nx = cr.y + (ix - H) * ts, ny = cr.z + (iy - H) * ts, nz = cr.w + (iz - H) * ts;
                    // a neighbour outside the key's range is absent, never a wrapped key
                    if (coord_in_range(cr.x, nx, ny, nz)) id = table_find(keys, vals, mask, shift, pack_key(cr.x, nx, ny, nz));
                    if ((unsigned)id >= (unsigned)n) id = -1;         // (a table value that is no row of x reads nothing)
                }
                const unsigned long long hits = __ballot(id >= 0);
                if (id >= 0) {
                    const int pos = base + __popcll(hits & ((1ull << lane) - 1ull));
                    q_row[wave][r][pos] = id;
                    q_k[wave][r][pos] = (uint16_t)kk;
                }
                base += __popcll(hits);
            }
            count[r] = base;
        }
        __syncthreads();                                              // (every wave runs the same K / segment loop)
        const int cnt = half ? count[1] : count[0];
        if (out_lane) {
            const int32_t* qr = q_row[wave][half];
            const uint16_t* qk = q_k[wave][half];
            int j = 0;
            for (; j + 4 <= cnt; j += 4) {                            // four row reads in flight, added in queue order
                float xv[4], wv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xv[u] = x[(int64_t)qr[j + u] * c + ch];
                    wv[u] = w[(int)qk[j + u] * w_channels + wch];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = acc + wv[u] * xv[u];
            }
            for (; j < cnt; ++j) acc = acc + w[(int)qk[j] * w_channels + wch] * x[(int64_t)qr[j] * c + ch];
        }
        __syncthreads();                                              // the queues are refilled by the next segment
    }
    if (out_lane) y[my_row * c + ch] = acc;
}

}  // namespace pcc

extern "C" int pcc_chconv(const float* x, int64_t n, int32_t c, const int32_t* coords, const uint64_t* keys, const int32_t* vals,
                          int64_t cap, int32_t tensor_stride, int32_t ksize, const float* w, int32_t w_channels, int32_t flip,
                          float* y, void* stream) {
    using namespace pcc;
    if (ksize < 1 || ksize > 11 || (ksize & 1) == 0) {
        set_error("pcc_chconv: kernel size must be odd, 1 .. 11 (got %d)", ksize);
        return PCC_ERR_UNSUPPORTED;
    }
    if (c < 1 || c > 32) {
        set_error("pcc_chconv: 1 .. 32 channels (got %d)", c);
        return PCC_ERR_UNSUPPORTED;
    }
    PCC_REQUIRE(w_channels == 1 || w_channels == c, "pcc_chconv: the window has %d channels, must be 1 or %d", w_channels, c);
    PCC_REQUIRE(flip == 0 || flip == 1, "pcc_chconv: flip must be 0 or 1");
    PCC_REQUIRE(cap > 0 && (cap & (cap - 1)) == 0, "pcc_chconv: bad capacity");
    PCC_REQUIRE(tensor_stride >= 1 && tensor_stride <= (1 << 24), "pcc_chconv: tensor stride must be 1 .. 2^24");
    PCC_REQUIRE(n >= 0 && n <= 0x7fffffff, "pcc_chconv: bad row count");
    if (n == 0) return PCC_OK;
    PCC_REQUIRE(x && coords && keys && vals && w && y, "pcc_chconv: null pointer");
    const dim3 grid(blocks_for(n, 2 * CHCONV_WAVES)), block(64 * CHCONV_WAVES);
    const uint64_t tmask = (uint64_t)(cap - 1);
    const int shift = grid_shift_of(tensor_stride);
    hipStream_t st = as_stream(stream);
#define PCC_CHCONV_LAUNCH(KS)                                                                                                   \
    case KS:                                                                                                                    \
        hipLaunchKernelGGL(chconv_kernel<KS>, grid, block, 0, st, x, (int)n, c, coords, keys, vals, tmask, shift, tensor_stride, w, \
                           w_channels, flip, y);                                                                                \
        break
    switch (ksize) {
        PCC_CHCONV_LAUNCH(1);
        PCC_CHCONV_LAUNCH(3);
        PCC_CHCONV_LAUNCH(5);
        PCC_CHCONV_LAUNCH(7);
        PCC_CHCONV_LAUNCH(9);
        PCC_CHCONV_LAUNCH(11);
    }
#undef PCC_CHCONV_LAUNCH
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}
