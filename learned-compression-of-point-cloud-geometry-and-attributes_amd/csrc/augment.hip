// Training augmentation: torchvision's ColorJitter on the colours of a collated batch, one parameter set per batch item
// (data/transform.py:107-130 of the reference; the formulas are restated in include/pcc_hip.h), and RandomRotate (:425-494): rotate
// about the block centre, round to the voxel grid, drop duplicate voxels (second half of this file).
//
// The four operations are pointwise except for contrast, which blends towards the MEAN gray of the item at that stage of the
// chain.  Three launches, whatever the number of items:
//   1. jitter_partial_kernel: a workgroup per 1,024-point chunk, chunks counted from the ITEM's first point.  It applies the
//      operations in front of contrast and sums the chunk's gray values in float64 by a fixed tree (four points per thread in
//      order, the xor butterfly of the wave, the four waves in order).
//   2. jitter_mean_kernel: a thread per item adds the item's chunk sums in chunk order (float64) and divides by the count.
//   3. jitter_apply_kernel: the same chunks again; recomputes the prefix (12 B per point read a second time instead of a
//      stored intermediate), then contrast and the rest.
// No float atomics: the mean is a fixed-shape sum, so results are bitwise equal from run to run, and — chunk boundaries and
// summation shape depend on the position inside the item only — an item gives the same bytes alone and inside a batch.
#include "common.h"
#include "first_rows.h"

namespace pcc {

constexpr int JIT_BLOCK = 256;
constexpr int JIT_PER_THREAD = 4;
constexpr int JIT_CHUNK = JIT_BLOCK * JIT_PER_THREAD;
enum { JIT_BRIGHTNESS = 0, JIT_CONTRAST = 1, JIT_SATURATION = 2, JIT_HUE = 3 };      // torchvision's fn_idx numbering

struct Rgb { float r, g, b; };

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float gray_of(Rgb c) { return (0.2989f * c.r + 0.587f * c.g) + 0.114f * c.b; }
__device__ __forceinline__ float blend1(float a, float b, float f) { return clamp01(f * a + (1.0f - f) * b); }
__device__ __forceinline__ Rgb blend(Rgb c, float other, float f) {
    return Rgb{blend1(c.r, other, f), blend1(c.g, other, f), blend1(c.b, other, f)};
}

__device__ __forceinline__ Rgb hue_shift(Rgb c, float f) {
    const float maxc = fmaxf(c.r, fmaxf(c.g, c.b)), minc = fminf(c.r, fminf(c.g, c.b));
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.0f : maxc);
    const float div = eq ? 1.0f : cr;
    const float rc = (maxc - c.r) / div, gc = (maxc - c.g) / div, bc = (maxc - c.b) / div;
    float h6;
    if (maxc == c.r) h6 = bc - gc;
    else if (maxc == c.g) h6 = (2.0f + rc) - bc;
    else h6 = (4.0f + gc) - rc;
    float h = fmodf(h6 / 6.0f + 1.0f, 1.0f);
    h = h + f;
    h = h - floorf(h);                                 // into [0, 1]; a sum just below zero may round to 1: sector 6 = sector 0
    const float v = maxc;
    const float h6s = h * 6.0f;
    const float fl = floorf(h6s);
    const float t = h6s - fl;
    int i = (int)fl % 6;
    const float p = clamp01(v * (1.0f - s));
    const float q = clamp01(v * (1.0f - s * t));
    const float u = clamp01(v * (1.0f - s * (1.0f - t)));
    switch (i) {
        case 0: return Rgb{v, u, p};
        case 1: return Rgb{q, v, p};
        case 2: return Rgb{p, v, u};
        case 3: return Rgb{p, q, v};
        case 4: return Rgb{u, p, v};
        default: return Rgb{v, p, q};
    }
}

// one operation of the chain; `mean` is read by contrast only
__device__ __forceinline__ Rgb jitter_op(Rgb c, int op, float f, float mean) {
    switch (op) {
        case JIT_BRIGHTNESS: return blend(c, 0.0f, f);
        case JIT_CONTRAST: return blend(c, mean, f);
        case JIT_SATURATION: {
            const float g = gray_of(c);
            return blend(c, g, f);
        }
        case JIT_HUE: return hue_shift(c, f);
        default: return c;
    }
}

// Where a workgroup works: items own ceil(count / JIT_CHUNK) consecutive workgroups each, in item order (an empty item owns
// none).  -> false for the spare workgroups behind the last item's (the grid is sized from n and nbatch on the host, which
// does not know the counts).  The walk over the offsets is wave-uniform.
struct JitChunk { int item; int64_t first, end; int64_t chunk_id; };
__device__ __forceinline__ bool locate_chunk(const int64_t* __restrict__ offsets, int nbatch, int64_t block, JitChunk& w) {
    int64_t base = 0;
    for (int it = 0; it < nbatch; ++it) {
        const int64_t lo = offsets[it], hi = offsets[it + 1];
        if (lo < 0) return false;                      // (offsets that are no offsets: touch nothing)
        const int64_t chunks = hi > lo ? (hi - lo + JIT_CHUNK - 1) / JIT_CHUNK : 0;
        if (block < base + chunks) {
            w.item = it;
            w.first = lo + (block - base) * JIT_CHUNK;
            w.end = hi;
            w.chunk_id = block;
            return true;
        }
        base += chunks;
    }
    return false;
}

struct JitItem { int op[4]; float f[4]; int contrast_at; };
__device__ __forceinline__ JitItem load_item(const float* __restrict__ params, const int32_t* __restrict__ order, int item) {
    JitItem j;
    j.contrast_at = 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = order[4 * item + k];
        j.op[k] = op;
        j.f[k] = (op >= 0 && op < 4) ? params[4 * item + op] : 0.0f;
        if (op == JIT_CONTRAST && j.contrast_at == 4) j.contrast_at = k;
    }
    return j;
}

__device__ __forceinline__ Rgb load_rgb(const float* __restrict__ rgb, int64_t p) {
    return Rgb{rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
}

__global__ __launch_bounds__(JIT_BLOCK) void jitter_partial_kernel(const float* __restrict__ rgb, int64_t n,
                                                                   const int64_t* __restrict__ offsets, int nbatch,
                                                                   const float* __restrict__ params,
                                                                   const int32_t* __restrict__ order,
                                                                   double* __restrict__ partial) {
    __shared__ double ws[JIT_BLOCK / 64];
    JitChunk w;
    if (!locate_chunk(offsets, nbatch, blockIdx.x, w)) return;
    const JitItem j = load_item(params, order, w.item);
    double sum = 0.0;
    if (j.contrast_at < 4) {
#pragma unroll
        for (int k = 0; k < JIT_PER_THREAD; ++k) {
            const int64_t p = w.first + threadIdx.x + k * JIT_BLOCK;
            if (p < w.end && p < n) {
                Rgb c = load_rgb(rgb, p);
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    if (s < j.contrast_at) c = jitter_op(c, j.op[s], j.f[s], 0.0f);
                sum += (double)gray_of(c);
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[w.chunk_id] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__global__ __launch_bounds__(JIT_BLOCK) void jitter_mean_kernel(const int64_t* __restrict__ offsets, int nbatch,
                                                                const double* __restrict__ partial, int64_t total_chunks,
                                                                float* __restrict__ mean) {
    // (every thread walks the offsets in front of its item: nbatch is at most 1,023 and this is one workgroup)
    for (int it = threadIdx.x; it < nbatch; it += JIT_BLOCK) {
        int64_t base = 0;
        for (int k = 0; k < it; ++k) {
            const int64_t c = offsets[k + 1] - offsets[k];
            base += c > 0 ? (c + JIT_CHUNK - 1) / JIT_CHUNK : 0;
        }
        const int64_t cnt = offsets[it + 1] - offsets[it];
        const int64_t chunks = cnt > 0 ? (cnt + JIT_CHUNK - 1) / JIT_CHUNK : 0;
        double s = 0.0;
        const bool ok = base + chunks <= total_chunks;      // (else the offsets name more points than the call has)
        for (int64_t k = 0; ok && k < chunks; ++k) s += partial[base + k];
        mean[it] = (ok && cnt > 0) ? (float)(s / (double)cnt) : 0.0f;
    }
}

__global__ __launch_bounds__(JIT_BLOCK) void jitter_apply_kernel(const float* __restrict__ rgb, int64_t n,
                                                                 const int64_t* __restrict__ offsets, int nbatch,
                                                                 const float* __restrict__ params,
                                                                 const int32_t* __restrict__ order,
                                                                 const float* __restrict__ mean, float* __restrict__ out) {
    JitChunk w;
    if (!locate_chunk(offsets, nbatch, blockIdx.x, w)) return;
    const JitItem j = load_item(params, order, w.item);
    const float m = mean[w.item];
#pragma unroll
    for (int k = 0; k < JIT_PER_THREAD; ++k) {
        const int64_t p = w.first + threadIdx.x + k * JIT_BLOCK;
        if (p < w.end && p < n) {
            Rgb c = load_rgb(rgb, p);
#pragma unroll
            for (int s = 0; s < 4; ++s) c = jitter_op(c, j.op[s], j.f[s], m);
            out[3 * p] = c.r;
            out[3 * p + 1] = c.g;
            out[3 * p + 2] = c.b;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// RandomRotate: unique rotated-and-rounded rows in order of first appearance, the lowest input row wins: the first-row set of
// first_rows.h over the candidates below (seven launches).
//
// The arithmetic is the contract of include/pcc_hip.h: every product and sum rounded separately in fp32 (the file is compiled
// with -ffp-contract=off), in the sum order of torch.mm(points - s/2, R.T) + s/2, then rintf (ties to even).  A result that is not
// finite or lies beyond the key range is never converted: it becomes a coordinate coord_in_range rejects, as does a row whose batch
// index has no matrix, and the count word reports COUNT_ERR_RANGE.
// ---------------------------------------------------------------------------------------------
struct Rotation {
    const int32_t* coords;
    const float* rot;        // [nbatch, 9] row-major
    int nbatch;
    float half;
    static constexpr int shift = 0;      // the output set has tensor stride 1
    static constexpr int REJECT = 1 << 30;
    __device__ __forceinline__ int grid(float v) const {
        const float r = rintf(v);
        return (fabsf(r) <= (float)COORD_LIMIT) ? (int)r : REJECT;      // false for NaN and infinities
    }
    __device__ __forceinline__ int4 get(int64_t i) const {
        const int4 c = reinterpret_cast<const int4*>(coords)[i];
        if ((unsigned)c.x >= (unsigned)nbatch) return make_int4(-1, REJECT, REJECT, REJECT);
        const float* R = rot + 9 * (int64_t)c.x;
        const float dx = (float)c.y - half, dy = (float)c.z - half, dz = (float)c.w - half;
        return make_int4(c.x, grid(((dx * R[0] + dy * R[1]) + dz * R[2]) + half), grid(((dx * R[3] + dy * R[4]) + dz * R[5]) + half),
                         grid(((dx * R[6] + dy * R[7]) + dz * R[8]) + half));
    }
    __device__ __forceinline__ bool ok(int64_t, bool ok) const { return ok; }
};

// a winner records the input row it came from
struct RotationSink {
    int32_t* out_src;
    __device__ __forceinline__ void operator()(int32_t row, int64_t i) const { out_src[row] = (int32_t)i; }
};

}  // namespace pcc

using namespace pcc;

extern "C" {

int pcc_augment_rotate(const int32_t* coords, int64_t n, const float* rot, int32_t nbatch, float half, uint64_t* keys,
                       int32_t* vals, int64_t cap, int32_t* scratch, int32_t* out_coords, int32_t* out_src, int64_t* out_count,
                       void* stream) {
    PCC_REQUIRE(n >= 0 && n < (1ll << 31) - 1, "pcc_augment_rotate: bad row count %lld", (long long)n);
    PCC_REQUIRE(nbatch >= 1 && nbatch <= BATCH_LIMIT + 1, "pcc_augment_rotate: nbatch %d outside 1..%d", nbatch, BATCH_LIMIT + 1);
    PCC_REQUIRE(cap > 0 && (cap & (cap - 1)) == 0 && cap >= 2 * n && cap <= (1ll << 31), "pcc_augment_rotate: bad capacity %lld for n=%lld",
                (long long)cap, (long long)n);
    PCC_REQUIRE(keys && vals && scratch && out_count, "pcc_augment_rotate: null table, scratch or count");
    PCC_REQUIRE(n == 0 || (coords && rot && out_coords && out_src), "pcc_augment_rotate: null rows, matrices or outputs");
    PCC_REQUIRE(half == half, "pcc_augment_rotate: half is not a number");
    return first_rows_build(Rotation{coords, rot, nbatch, half}, RotationSink{out_src}, n, keys, vals, cap, scratch, out_coords, out_count,
                            as_stream(stream));
}

int32_t pcc_color_jitter_chunk(void) { return JIT_CHUNK; }

int64_t pcc_color_jitter_scratch_bytes(int64_t n, int32_t nbatch) {
    if (n < 0 || nbatch < 0) return 0;
    const int64_t chunks = (n + JIT_CHUNK - 1) / JIT_CHUNK + nbatch;
    return chunks * (int64_t)sizeof(double) + ((int64_t)nbatch * (int64_t)sizeof(float) + 7) / 8 * 8;
}

int pcc_color_jitter(const float* rgb, int64_t n, const int64_t* offsets, int32_t nbatch, const float* params,
                     const int32_t* order, float* out, void* scratch, int64_t scratch_bytes, void* stream) {
    PCC_REQUIRE(n >= 0 && nbatch >= 0, "pcc_color_jitter: negative size");
    if (n == 0 || nbatch == 0) return PCC_OK;
    PCC_REQUIRE(nbatch <= BATCH_LIMIT + 1, "pcc_color_jitter: nbatch %d above %d", nbatch, BATCH_LIMIT + 1);
    PCC_REQUIRE(rgb && offsets && params && order && out && scratch, "pcc_color_jitter: null argument");
    PCC_REQUIRE(scratch_bytes >= pcc_color_jitter_scratch_bytes(n, nbatch) && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0,
                "pcc_color_jitter: scratch of %lld bytes is short or not 8-byte aligned", (long long)scratch_bytes);
    // an item of c points owns ceil(c / chunk) workgroups: at most n / chunk + 1 each, n / chunk + nbatch in all
    const int64_t chunks = (n + JIT_CHUNK - 1) / JIT_CHUNK + nbatch;
    PCC_REQUIRE(chunks < (1ll << 31), "pcc_color_jitter: too many points (%lld)", (long long)n);
    double* partial = reinterpret_cast<double*>(scratch);
    float* mean = reinterpret_cast<float*>(partial + chunks);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(jitter_partial_kernel, dim3((unsigned)chunks), dim3(JIT_BLOCK), 0, st, rgb, n, offsets, nbatch, params, order,
                       partial);
    hipLaunchKernelGGL(jitter_mean_kernel, dim3(1), dim3(JIT_BLOCK), 0, st, offsets, nbatch, (const double*)partial, chunks, mean);
    hipLaunchKernelGGL(jitter_apply_kernel, dim3((unsigned)chunks), dim3(JIT_BLOCK), 0, st, rgb, n, offsets, nbatch, params, order,
                       (const float*)mean, out);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
