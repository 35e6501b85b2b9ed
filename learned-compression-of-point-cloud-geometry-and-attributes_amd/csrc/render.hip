// View rendering and view PSNR / SSIM for the view-dependent evaluation (evaluate_view_dep.py:102-305).
//
// pcc_render_view replaces render_pointviews (evaluate_view_dep.py:308-348: an open3d OpenGL window, which is neither
// available without a display nor reproducible pixel for pixel) by an exact integer projection of a voxelised cloud: an
// orthographic z-buffer splat along a signed coordinate axis — every view the reference uses is one
// (evaluate_view_dep.py:46-57).
//
//   u = right . p, v = up . p, d = front . p              (front points from the object to the camera, as open3d's set_front)
//   the point covers columns (u - u_min) scale + ox + i and rows (v_max - v) scale + oy + j,  i, j in [0, point_size)
//   pixels outside the image are dropped; the pixel shows the point with the largest d and, among equal d, the lowest row
//   index; untouched pixels show the background
//
// One z-buffer for every kind of view.  A view type (RenderView, CameraView) projects a row to a Splat: its square clipped to
// the image and a 31-bit key, larger = nearer.  Three kernels: the z-buffer is cleared to 0; splat_kernel<View>, one thread per
// point, does one 64-bit atomicMax of the word (key << 32) | (0xFFFFFFFF - row) per pixel of the splat; one thread per four
// pixels resolves the words to colours.  A maximum does not depend on the order its operands arrive in, so the image is bitwise
// reproducible although the splat is atomic.  Every key is positive, so the word of a drawn pixel is never 0; a row with a
// coordinate outside the range draws nothing.  Atomic bound: at most 16 x 16 64-bit atomics per point on H W words.
//
// pcc_view_visibility is the way back from the pixels to the points: the same clear and splat, then gather_kernel<View>, one
// thread per point, walks its splat again and reads how far the point lies behind the z-buffer front (`behind`, the minimum over
// its pixels of (front key - own key) >> View::GAP_SHIFT) and how many pixels it owns (`won`).  No image is resolved.
//
// pcc_render_view and pcc_view_visibility use the orthographic RenderView (key = d + 2^18, gap shift 0: whole voxels);
// pcc_render_camera and pcc_camera_visibility the pinhole CameraView at a position (a perspective projection in int64, key =
// 0x7FFFFFFF - depth key in 1/256 voxel, gap shift 8), whose walk back also returns each point's depth key.
//
// pcc_view_buffers / pcc_camera_buffers expose the z-buffer itself: the same clear and splat, then buffers_kernel<View>, one thread
// per pixel, unpacks the word into the row it shows (-1 for background) and its depth (View::depth_of the key).
//
// pcc_view_sample / pcc_camera_sample carry an IMAGE back to the points (screen-space quality maps): the same clear and splat, then
// sample_kernel<View, C>, one thread per point, walks its splat as gather_kernel does and adds up (and takes the maximum of) a
// C-channel int32 image over the pixels that count for the point: its own pixels (tolerance PCC_SAMPLE_OWN) or the pixels whose
// front is at most `tolerance` whole voxels in front of it, the quantity whose minimum is `behind`.  All integer, no atomics
// beyond the splat's.
//
// pcc_image_compare replaces rgb2yuv +peak_signal_noise_ratio + structural_similarity (evaluate_view_dep.py:196-204) by
// their raw sums in float64: one workgroup per IC_TILE x IC_TILE tile converts the tile and its 6-pixel apron to YUV one
// channel at a time into LDS, adds the squared differences of the pixels it owns and the SSIM map values of the 7 x 7
// windows whose top-left pixel it owns, reduces them over a fixed tree and stores its eight partials; a second kernel
// adds the partials in ascending workgroup order.  No float atomics: the result is bitwise reproducible.  Separate
// multiplies and adds throughout (the library is built with -ffp-contract=off).  pcc_image_compare_masked is the same tile
// kernel with a mask (a template flag): a pixel adds its squared differences only when it is masked, a window its SSIM value
// only when its centre pixel is; nothing else changes, so the additions happen in the same order.
#include "common.h"

namespace pcc {

constexpr int RENDER_DEPTH_BIAS = 1 << 18;
constexpr int RENDER_MAX_DIM = 8192;

// One projected point: its splat clipped to the image (rows r0 .. r1 - 1, columns c0 .. c1 - 1) and the high half of its
// z-buffer word, in (0, 2^31): the larger key is the nearer point.
struct Splat {
    int32_t r0, r1, c0, c1;
    uint32_t key;
};

// the square of `size` pixels whose top-left pixel is (row0, col0), clipped to the H x W image once, in int64
__device__ __forceinline__ void clip_splat(int64_t row0, int64_t col0, int64_t size, int32_t H, int32_t W, Splat& out) {
    const int64_t c0 = col0 < 0 ? 0 : col0, c1 = col0 + size > W ? W : col0 + size;
    const int64_t r0 = row0 < 0 ? 0 : row0, r1 = row0 + size > H ? H : row0 + size;
    // an empty range is stored as 0 .. 0: the clipped bounds of a splat far outside the image do not fit 32 bits
    const bool inside = c0 < c1 && r0 < r1;
    out.c0 = inside ? (int32_t)c0 : 0; out.c1 = inside ? (int32_t)c1 : 0;
    out.r0 = inside ? (int32_t)r0 : 0; out.r1 = inside ? (int32_t)r1 : 0;
}

__device__ __forceinline__ uint64_t splat_word(uint32_t key, int64_t row) {
    return ((uint64_t)key << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)row);
}

// ---- orthographic axis view ----
// |d| <= COORD_LIMIT < 2^18, so the key d + 2^18 is positive; keys are whole voxels, so the gap between two of them is `behind`.
struct RenderView {
    static constexpr int GAP_SHIFT = 0;
    static constexpr bool HAS_DEPTH = false;
    int32_t r[3], u[3], f[3];
    int32_t u_min, v_max, ox, oy, scale, point_size, H, W;

    // what pcc_view_buffers reports for a key: d = front . p
    static __device__ __forceinline__ int32_t depth_of(uint32_t key) { return (int32_t)key - RENDER_DEPTH_BIAS; }

    // false when the row draws nothing: a coordinate out of range
    __device__ __forceinline__ bool project(const int4 c, Splat& out) const {
        if (!coord_in_range(0, c.y, c.z, c.w)) return false;
        const int pu = r[0] * c.y + r[1] * c.z + r[2] * c.w;
        const int pv = u[0] * c.y + u[1] * c.z + u[2] * c.w;
        const int d = f[0] * c.y + f[1] * c.z + f[2] * c.w;
        // 64-bit positions: u_min / v_max / ox / oy are the caller's and may be anywhere in int32, so (pu - u_min) * scale + ox
        // reaches about 2^38; the box is narrowed to 32 bits only after it is clipped
        clip_splat(((int64_t)v_max - pv) * scale + oy, ((int64_t)pu - u_min) * scale + ox, point_size, H, W, out);
        out.key = (uint32_t)(d + RENDER_DEPTH_BIAS);
        return true;
    }
};

// ---- pinhole camera: perspective projection, all int64 ----
// The camera crosses the ABI as integers only (pcc_hip.h): pos in 1/16 voxel, the three axes in 2^-14, focal in 1/16 pixel,
// near in 1/16 voxel, the voxel edge ps in 1/16 voxel.  For a row p:
//   e = 16 p - pos;  U = right . e, V = up . e, D = -(front . e)   (2^-18 voxel; front points from the scene to the camera)
//   drawn <=> D >= near 2^14;  X = floor(focal U / D), Y = floor(focal V / D)   (1/16 pixel from the principal point)
//   s = clamp(ceil(focal ps 2^10 / D), 1, 16);  col0 = floor((8 W + X - 8 s) / 16), row0 = floor((8 H - Y - 8 s) / 16)
//   depth key dk = D >> 10 (1/256 voxel); key = 0x7FFFFFFF - dk, so the gap between two keys >> 8 is `behind` in whole voxels
// Bounds, which the host entry re-derives from the arguments it is given (check_camera): |e_k| <= |pos_k| + 16 COORD_LIMIT <
// 2^24 + 2^21, an axis row has entries of at most 2^14, so |U|, |V|, |D| < 3 2^14 (2^24 + 2^21) < 2^40, |focal U| < 2^60, dk <
// 2^30 and dk >= 16 near >= 16: the key of a drawn point is in (2^30, 2^31) and never 0.

// floor(a / b) for b > 0, through one unsigned division (C++'s `/` truncates towards zero)
__device__ __forceinline__ int64_t camera_floordiv(int64_t a, uint64_t b) {
    return a >= 0 ? (int64_t)((uint64_t)a / b) : -(int64_t)(((uint64_t)(-a) + b - 1) / b);
}

struct CameraView {
    static constexpr int GAP_SHIFT = 8;
    static constexpr bool HAS_DEPTH = true;
    int32_t pos[3], ax[3][3];
    int32_t focal, near, ps, H, W;

    // what pcc_camera_buffers reports for a key: the depth key dk
    static __device__ __forceinline__ int32_t depth_of(uint32_t key) { return (int32_t)(0x7FFFFFFFu - key); }

    // false when the row draws nothing: a coordinate out of range, or in front of the near plane (behind the camera included)
    __device__ __forceinline__ bool project(const int4 c, Splat& out) const {
        if (!coord_in_range(0, c.y, c.z, c.w)) return false;
        const int64_t e0 = 16 * (int64_t)c.y - pos[0], e1 = 16 * (int64_t)c.z - pos[1], e2 = 16 * (int64_t)c.w - pos[2];
        const int64_t U = ax[0][0] * e0 + ax[0][1] * e1 + ax[0][2] * e2;
        const int64_t V = ax[1][0] * e0 + ax[1][1] * e1 + ax[1][2] * e2;
        const int64_t D = -(ax[2][0] * e0 + ax[2][1] * e1 + ax[2][2] * e2);
        if (D < ((int64_t)near << 14)) return false;
        const uint64_t d = (uint64_t)D;
        const int64_t X = camera_floordiv((int64_t)focal * U, d), Y = camera_floordiv((int64_t)focal * V, d);
        const uint64_t edge = ((((uint64_t)focal * (uint64_t)ps) << 10) + d - 1) / d;
        const int64_t s = edge < 1 ? 1 : (edge > 16 ? 16 : (int64_t)edge);
        clip_splat((8 * (int64_t)H - Y - 8 * s) >> 4, (8 * (int64_t)W + X - 8 * s) >> 4, s, H, W, out);   // >> floors
        out.key = 0x7FFFFFFFu - (uint32_t)(d >> 10);
        return true;
    }
};

__global__ __launch_bounds__(256) void render_clear_kernel(uint64_t* __restrict__ zbuf, int64_t npix) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npix) zbuf[i] = 0ull;
}

// one thread per point, at most 16 x 16 atomics each; the splat is clipped first, so every index is inside H W
template <class View>
__global__ __launch_bounds__(256) void splat_kernel(const int32_t* __restrict__ coords, int64_t n, View a, uint64_t* __restrict__ zbuf) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];                  // (batch, x, y, z): the batch is ignored
    Splat sp;
    if (!a.project(c, sp)) return;
    const uint64_t word = splat_word(sp.key, row);
    for (int32_t py = sp.r0; py < sp.r1; ++py)
        for (int32_t px = sp.c0; px < sp.c1; ++px)
            atomicMax(reinterpret_cast<unsigned long long*>(zbuf) + ((int64_t)py * a.W + px), (unsigned long long)word);
}

// four pixels (12 bytes = three aligned words of the image) per thread
__global__ __launch_bounds__(256) void render_resolve_kernel(const uint64_t* __restrict__ zbuf, const uint8_t* __restrict__ rgb8,
                                                             uint32_t background, int64_t npix, uint8_t* __restrict__ image) {
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    uint8_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t word = p0 + k < npix ? zbuf[p0 + k] : 0ull;
        if (word == 0ull) {
            b[3 * k] = (uint8_t)background; b[3 * k + 1] = (uint8_t)(background >> 8); b[3 * k + 2] = (uint8_t)(background >> 16);
        } else {
            const int64_t row = (int64_t)(0xFFFFFFFFu - (uint32_t)word);
            b[3 * k] = rgb8[3 * row]; b[3 * k + 1] = rgb8[3 * row + 1]; b[3 * k + 2] = rgb8[3 * row + 2];
        }
    }
    if (p0 + 4 <= npix && (reinterpret_cast<uintptr_t>(image) & 3u) == 0) {
        uint32_t* out = reinterpret_cast<uint32_t*>(image + 3 * p0);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            out[w] = (uint32_t)b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) | ((uint32_t)b[4 * w + 3] << 24);
    } else {
        for (int k = 0; k < 12 && p0 * 3 + k < npix * 3; ++k) image[3 * p0 + k] = b[k];
    }
}

// ---- visibility: the way back from the z-buffer's pixels to the points ----
// One thread per point walks the point's splat again, over the z-buffer the splat kernel has finished: behind = the smallest
// ((key of the pixel's winner) - (key of this point)) >> View::GAP_SHIFT over its pixels inside the image, won = the pixels whose
// word is this row's own, depth (View::HAS_DEPTH only, decided at compile time) = 0x7FFFFFFF - key, the point's depth key.
// Every pixel of the splat holds a word of key >= this row's (it took part in the maximum), so behind >= 0, and it is 0 exactly
// where the front of a pixel is less than one voxel in front of this point (at its own depth, for the orthographic view); the tie
// to the lowest row decides only `won`.  A thread owns its row's outputs: no atomics, and `accumulate` is a plain
// read-modify-write (min of behind and depth, sum of won).
template <class View>
__global__ __launch_bounds__(256) void gather_kernel(const int32_t* __restrict__ coords, int64_t n, View a, const uint64_t* __restrict__ zbuf,
                                                     int accumulate, int32_t* __restrict__ behind, int32_t* __restrict__ won,
                                                     int32_t* __restrict__ depth) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];
    int32_t best = PCC_VIS_OFFSCREEN, count = 0, dist = PCC_VIS_OFFSCREEN;
    Splat sp;
    if (a.project(c, sp) && sp.r0 < sp.r1) {
        const uint64_t own = splat_word(sp.key, row);
        dist = (int32_t)(0x7FFFFFFFu - sp.key);
        for (int32_t py = sp.r0; py < sp.r1; ++py) {
            for (int32_t px = sp.c0; px < sp.c1; ++px) {
                const uint64_t word = zbuf[(int64_t)py * a.W + px];
                const int32_t gap = (int32_t)(((uint32_t)(word >> 32) - sp.key) >> View::GAP_SHIFT);
                best = gap < best ? gap : best;
                count += word == own;
            }
        }
    }
    if (accumulate) {
        const int32_t old = behind[row];
        best = old < best ? old : best;
        count += won[row];
    }
    behind[row] = best;
    won[row] = count;
    if constexpr (View::HAS_DEPTH) {
        if (accumulate) {
            const int32_t old = depth[row];
            dist = old < dist ? old : dist;
        }
        depth[row] = dist;
    }
}

// ---- the z-buffer's planes: the row and the depth every pixel shows ----
// One thread per pixel unpacks its word: index = the row under the full winner rule (the low half, 0xFFFFFFFF - row), depth =
// View::depth_of(the key); a word of 0 (no splat reached the pixel) is background: -1 and PCC_VIS_OFFSCREEN.
template <class View>
__global__ __launch_bounds__(256) void buffers_kernel(const uint64_t* __restrict__ zbuf, int64_t npix, int32_t* __restrict__ index,
                                                      int32_t* __restrict__ depth) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const uint64_t word = zbuf[p];
    index[p] = word == 0ull ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)word);
    depth[p] = word == 0ull ? PCC_VIS_OFFSCREEN : View::depth_of((uint32_t)(word >> 32));
}

// ---- back-projection: an image's values carried to the points ----
// gather_kernel's walk.  A pixel of the splat counts for the row when its word is the row's own (tolerance == PCC_SAMPLE_OWN:
// the pixels that show the point) or when (front key - own key) >> View::GAP_SHIFT <= tolerance (tolerance >= 0: the gap whose
// minimum is `behind`, so count > 0 exactly where behind <= tolerance).  Over the counted pixels: total = the sum of the image
// (int64: at most 256 pixels of |value| < 2^31 per call), count, peak = the maximum (PCC_SAMPLE_NONE when nothing counted).  C is
// a template parameter so that the per-channel accumulators stay in registers (a run-time channel loop over a local array would
// put them in scratch memory).  A thread owns its row: `accumulate` is a plain read-modify-write (sum, sum, max).
template <class View, int C>
__global__ __launch_bounds__(256) void sample_kernel(const int32_t* __restrict__ coords, int64_t n, View a, const uint64_t* __restrict__ zbuf,
                                                     const int32_t* __restrict__ image, int32_t tolerance, int accumulate,
                                                     int64_t* __restrict__ total, int32_t* __restrict__ count, int32_t* __restrict__ peak) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];
    int64_t sum[C];
    int32_t top[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) { sum[ch] = 0; top[ch] = PCC_SAMPLE_NONE; }
    int32_t hits = 0;
    Splat sp;
    if (a.project(c, sp) && sp.r0 < sp.r1) {
        const uint64_t own = splat_word(sp.key, row);
        for (int32_t py = sp.r0; py < sp.r1; ++py) {
            for (int32_t px = sp.c0; px < sp.c1; ++px) {
                const int64_t at = (int64_t)py * a.W + px;
                const uint64_t word = zbuf[at];
                const int32_t gap = (int32_t)(((uint32_t)(word >> 32) - sp.key) >> View::GAP_SHIFT);
                if (tolerance < 0 ? word != own : gap > tolerance) continue;
                ++hits;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const int32_t v = image[at * C + ch];
                    sum[ch] += v;
                    top[ch] = v > top[ch] ? v : top[ch];
                }
            }
        }
    }
    if (accumulate) hits += count[row];
    count[row] = hits;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        if (accumulate) {
            const int32_t old = peak[row * C + ch];
            sum[ch] += total[row * C + ch];
            top[ch] = old > top[ch] ? old : top[ch];
        }
        total[row * C + ch] = sum[ch];
        peak[row * C + ch] = top[ch];
    }
}

// ---- image metrics ----
constexpr int IC_TILE = 32;                 // pixels a workgroup owns per side
constexpr int IC_WIN = 7;                     // structural_similarity's window
constexpr int IC_SPAN = IC_TILE + IC_WIN - 1; // the tile and its apron
constexpr int IC_THREADS = 256;

// scikit-image's yuv_from_rgb
__device__ const double IC_YUV[3][3] = {{0.299, 0.587, 0.114},
                                        {-0.14714119, -0.28886916, 0.43601035},
                                        {0.61497538, -0.51496512, -0.10001026}};

__device__ __forceinline__ double ic_yuv(const uint8_t* __restrict__ px, int ch) {
    const double r = (double)px[0] / 255.0, g = (double)px[1] / 255.0, b = (double)px[2] / 255.0;
    return (r * IC_YUV[ch][0] + g * IC_YUV[ch][1]) + b * IC_YUV[ch][2];
}

// sum / min / max of one value per thread over the workgroup, as a fixed tree in LDS (op: 0 sum, 1 min, 2 max)
__device__ __forceinline__ double ic_block_reduce(double v, int op, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = IC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            const double a = red[t], b = red[t + s];
            red[t] = op == 0 ? a + b : (op == 1 ? (b < a ? b : a) : (b > a ? b : a));
        }
        __syncthreads();
    }
    return red[0];
}

// MASKED: `mask` (uint8 [H, W], nonzero = inside) decides which pixels add their squared differences and which windows (by their
// centre pixel, top-left + 3) their SSIM value; the reference's minimum and maximum stay over every pixel.
template <bool MASKED>
__global__ __launch_bounds__(IC_THREADS) void image_compare_tile_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ img,
                                                                        const uint8_t* __restrict__ mask, int H, int W, int tiles_x,
                                                                        double* __restrict__ partials) {
    __shared__ double xs[IC_SPAN][IC_SPAN], ys[IC_SPAN][IC_SPAN];
    __shared__ double red[IC_THREADS];
    const int t = threadIdx.x;
    const int r0 = (blockIdx.x / tiles_x) * IC_TILE, c0 = (blockIdx.x % tiles_x) * IC_TILE;
    const double C1 = 1e-4, C2 = 9e-4, cov_norm = 49.0 / 48.0;
    double sse[3] = {0.0, 0.0, 0.0}, ssim[3] = {0.0, 0.0, 0.0};
    double lo = INFINITY, hi = -INFINITY;
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();                                   // the previous channel's windows are read
        for (int e = t; e < IC_SPAN * IC_SPAN; e += IC_THREADS) {
            const int lr = e / IC_SPAN, lc = e % IC_SPAN;
            const int r = r0 + lr, c = c0 + lc;
            double x = 0.0, y = 0.0;                       // outside the image: read by no window that counts
            if (r < H && c < W) {
                const int64_t at = 3 * ((int64_t)r * W + c);
                x = ic_yuv(ref + at, ch);
                y = ic_yuv(img + at, ch);
                if (lr < IC_TILE && lc < IC_TILE) {        // a pixel this workgroup owns
                    if (!MASKED || mask[(int64_t)r * W + c]) {
                        const double diff = x - y;
                        sse[ch] = sse[ch] + diff * diff;
                    }
                    lo = x < lo ? x : lo;
                    hi = x > hi ? x : hi;
                }
            }
            xs[lr][lc] = x;
            ys[lr][lc] = y;
        }
        __syncthreads();
        for (int o = t; o < IC_TILE * IC_TILE; o += IC_THREADS) {
            const int lr = o / IC_TILE, lc = o % IC_TILE;
            if (r0 + lr + IC_WIN > H || c0 + lc + IC_WIN > W) continue;      // the window leaves the image: not in the crop
            if (MASKED && !mask[(int64_t)(r0 + lr + IC_WIN / 2) * W + (c0 + lc + IC_WIN / 2)]) continue;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
            for (int j = 0; j < IC_WIN; ++j) {
#pragma unroll
                for (int i = 0; i < IC_WIN; ++i) {
                    const double x = xs[lr + j][lc + i], y = ys[lr + j][lc + i];
                    sx = sx + x; sy = sy + y;
                    sxx = sxx + x * x; syy = syy + y * y; sxy = sxy + x * y;
                }
            }
            const double ux = sx / 49.0, uy = sy / 49.0, uxx = sxx / 49.0, uyy = syy / 49.0, uxy = sxy / 49.0;
            const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
            const double S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
            ssim[ch] = ssim[ch] + S;
        }
    }
    double out[8];
    for (int ch = 0; ch < 3; ++ch) out[ch] = ic_block_reduce(sse[ch], 0, red);
    for (int ch = 0; ch < 3; ++ch) out[3 + ch] = ic_block_reduce(ssim[ch], 0, red);
    out[6] = ic_block_reduce(lo, 1, red);
    out[7] = ic_block_reduce(hi, 2, red);
    if (t < 8) partials[8 * (int64_t)blockIdx.x + t] = out[t];
}

// thread q adds (or takes the minimum / maximum of) quantity q of every workgroup, in ascending workgroup order
__global__ __launch_bounds__(64) void image_compare_sum_kernel(const double* __restrict__ partials, int tiles, double* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= 8) return;
    double acc = partials[q];
    for (int b = 1; b < tiles; ++b) {
        const double v = partials[8 * (int64_t)b + q];
        acc = q < 6 ? acc + v : (q == 6 ? (v < acc ? v : acc) : (v > acc ? v : acc));
    }
    out[q] = acc;
}

static bool signed_unit_axis(const int32_t* a) {
    const int nz = (a[0] != 0) + (a[1] != 0) + (a[2] != 0);
    return nz == 1 && a[0] * a[0] + a[1] * a[1] + a[2] * a[2] == 1;
}
static int dot3(const int32_t* a, const int32_t* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the checks every view shares: the image's size and the cloud's (a row index must fit the low half of a z-buffer word)
static int check_image(const char* who, int32_t H, int32_t W, int64_t n) {
    PCC_REQUIRE(H >= 1 && H <= RENDER_MAX_DIM && W >= 1 && W <= RENDER_MAX_DIM, "%s: H and W must be 1 .. %d (got %d x %d)", who,
                RENDER_MAX_DIM, H, W);
    PCC_REQUIRE(n >= 0 && n <= 0xFFFFFFFEll, "%s: 0 .. 2^32 - 2 points", who);
    return PCC_OK;
}

// the checks pcc_render_view and pcc_view_visibility share: the view's axes, the splat's sizes, the image's and the cloud's
static int check_view(const char* who, const int32_t* right, const int32_t* up, const int32_t* front, int32_t scale, int32_t point_size,
                      int32_t H, int32_t W, int64_t n) {
    PCC_REQUIRE(right && up && front, "%s: axes required", who);
    PCC_REQUIRE(signed_unit_axis(right) && signed_unit_axis(up) && signed_unit_axis(front),
                "%s: right, up and front must be signed unit coordinate axes", who);
    PCC_REQUIRE(dot3(right, up) == 0 && dot3(up, front) == 0 && dot3(right, front) == 0, "%s: axes must be mutually orthogonal", who);
    const int32_t cross[3] = {up[1] * front[2] - up[2] * front[1], up[2] * front[0] - up[0] * front[2], up[0] * front[1] - up[1] * front[0]};
    PCC_REQUIRE(cross[0] == right[0] && cross[1] == right[1] && cross[2] == right[2], "%s: right must be up x front", who);
    PCC_REQUIRE(scale >= 1 && scale <= 64, "%s: scale must be 1 .. 64 (got %d)", who, scale);
    PCC_REQUIRE(point_size >= 1 && point_size <= 16, "%s: point_size must be 1 .. 16 (got %d)", who, point_size);
    if (int rc = check_image(who, H, W, n)) return rc;
    return PCC_OK;
}

static RenderView make_view(const int32_t* right, const int32_t* up, const int32_t* front, int32_t u_min, int32_t v_max, int32_t ox,
                            int32_t oy, int32_t scale, int32_t point_size, int32_t H, int32_t W) {
    RenderView a;
    for (int k = 0; k < 3; ++k) { a.r[k] = right[k]; a.u[k] = up[k]; a.f[k] = front[k]; }
    a.u_min = u_min; a.v_max = v_max; a.ox = ox; a.oy = oy; a.scale = scale; a.point_size = point_size; a.H = H; a.W = W;
    return a;
}

constexpr int32_t CAMERA_POS_MAX = 1 << 24;      // 2^20 voxels in 1/16 voxel
constexpr int32_t CAMERA_AXIS_ONE = 1 << 14;
constexpr int32_t CAMERA_FOCAL_MAX = 1 << 20;

// the checks pcc_render_camera and pcc_camera_visibility share: the table of pcc_hip.h, then the overflow bound of the
// projection worked out from THESE arguments rather than taken from the table
static int check_camera(const char* who, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q, int32_t near_q, int32_t ps_q,
                        int32_t H, int32_t W, int64_t n) {
    PCC_REQUIRE(pos_q && axes_q, "%s: camera position and axes required", who);
    for (int k = 0; k < 3; ++k)
        PCC_REQUIRE(pos_q[k] >= -CAMERA_POS_MAX && pos_q[k] <= CAMERA_POS_MAX, "%s: pos_q[%d] = %d is beyond +-2^24 (2^20 voxels)", who, k,
                    pos_q[k]);
    for (int k = 0; k < 9; ++k)
        PCC_REQUIRE(axes_q[k] >= -CAMERA_AXIS_ONE && axes_q[k] <= CAMERA_AXIS_ONE, "%s: axes_q[%d] = %d is beyond +-2^14", who, k, axes_q[k]);
    PCC_REQUIRE(focal_q >= 1 && focal_q <= CAMERA_FOCAL_MAX, "%s: focal_q must be 1 .. 2^20 (got %d)", who, focal_q);
    PCC_REQUIRE(near_q >= 1, "%s: near_q must be at least 1 (got %d)", who, near_q);
    PCC_REQUIRE(ps_q >= 1 && ps_q <= 256, "%s: ps_q must be 1 .. 256 (got %d)", who, ps_q);
    if (int rc = check_image(who, H, W, n)) return rc;
    for (int r = 0; r < 3; ++r) {                         // |axis . e| <= sum |axis_k| (|pos_k| + 16 COORD_LIMIT), < 2^41 whatever the caller gave
        int64_t reach = 0;
        for (int k = 0; k < 3; ++k) {
            const int64_t ax = axes_q[3 * r + k], p = pos_q[k];
            reach += (ax < 0 ? -ax : ax) * ((p < 0 ? -p : p) + 16 * (int64_t)COORD_LIMIT);
        }
        PCC_REQUIRE(reach < (1ll << 40) && reach * focal_q < (1ll << 60) && (reach >> 10) < 0x7FFFFFFFll,
                    "%s: the projection of axis %d would leave its 60 bits", who, r);
    }
    return PCC_OK;
}

static CameraView make_camera(const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q, int32_t near_q, int32_t ps_q, int32_t H,
                              int32_t W) {
    CameraView a;
    for (int k = 0; k < 3; ++k) a.pos[k] = pos_q[k];
    for (int k = 0; k < 9; ++k) a.ax[k / 3][k % 3] = axes_q[k];
    a.focal = focal_q; a.near = near_q; a.ps = ps_q; a.H = H; a.W = W;
    return a;
}

// What the two render entries share, after the view's own checks: clear, splat, resolve.
template <class View>
static int draw(const char* who, const View& a, const int32_t* coords, const uint8_t* rgb8, int64_t n, const uint8_t* background,
                void* scratch, int64_t scratch_bytes, uint8_t* image, void* stream) {
    PCC_REQUIRE(background, "%s: background required", who);
    PCC_REQUIRE(n == 0 || (coords && rgb8), "%s: null cloud with n > 0", who);
    PCC_REQUIRE(scratch && image, "%s: z-buffer and image required", who);
    PCC_REQUIRE(scratch_bytes >= pcc_render_scratch_bytes(a.H, a.W), "%s: scratch too small", who);
    const int64_t npix = (int64_t)a.H * a.W;
    const uint32_t bg = (uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16);
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    if (n > 0) hipLaunchKernelGGL(splat_kernel<View>, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    hipLaunchKernelGGL(render_resolve_kernel, dim3(blocks_for((npix + 3) / 4, 256)), dim3(256), 0, st, zbuf, rgb8, bg, npix, image);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

// What the two visibility entries share: clear, splat, gather.  `depth` is an output only of a view that has one.
template <class View>
static int look_back(const char* who, const View& a, const int32_t* coords, int64_t n, void* scratch, int64_t scratch_bytes,
                     int32_t accumulate, int32_t* behind, int32_t* won, int32_t* depth, void* stream) {
    PCC_REQUIRE(n == 0 || (coords && behind && won && (depth || !View::HAS_DEPTH)), "%s: null cloud or outputs with n > 0", who);
    PCC_REQUIRE(scratch, "%s: z-buffer required", who);
    PCC_REQUIRE(scratch_bytes >= pcc_visibility_scratch_bytes(a.H, a.W), "%s: scratch too small", who);
    if (n == 0) return PCC_OK;                                // nothing to write, and the z-buffer is scratch: nothing to launch
    const int64_t npix = (int64_t)a.H * a.W;
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    hipLaunchKernelGGL(splat_kernel<View>, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    hipLaunchKernelGGL(gather_kernel<View>, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf, accumulate != 0, behind, won,
                       depth);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

// What the two buffers entries share: clear, splat, unpack.  n == 0 is valid: every pixel is background.
template <class View>
static int show_buffers(const char* who, const View& a, const int32_t* coords, int64_t n, void* scratch, int64_t scratch_bytes,
                        int32_t* index, int32_t* depth, void* stream) {
    PCC_REQUIRE(n == 0 || coords, "%s: null cloud with n > 0", who);
    PCC_REQUIRE(scratch && index && depth, "%s: z-buffer, index and depth required", who);
    PCC_REQUIRE(scratch_bytes >= pcc_render_scratch_bytes(a.H, a.W), "%s: scratch too small", who);
    const int64_t npix = (int64_t)a.H * a.W;
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    if (n > 0) hipLaunchKernelGGL(splat_kernel<View>, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    hipLaunchKernelGGL(buffers_kernel<View>, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix, index, depth);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

template <class View, int C>
static void launch_sample(hipStream_t st, const View& a, const int32_t* coords, int64_t n, const uint64_t* zbuf, const int32_t* image,
                          int32_t tolerance, int accumulate, int64_t* total, int32_t* count, int32_t* peak) {
    hipLaunchKernelGGL((sample_kernel<View, C>), dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf, image, tolerance,
                       accumulate, total, count, peak);
}

// What the two sample entries share: clear, splat, sample.
template <class View>
static int sample_back(const char* who, const View& a, const int32_t* coords, int64_t n, void* scratch, int64_t scratch_bytes,
                       int32_t accumulate, const int32_t* image, int32_t channels, int32_t tolerance, int64_t* total, int32_t* count,
                       int32_t* peak, void* stream) {
    PCC_REQUIRE(channels >= 1 && channels <= PCC_SAMPLE_MAX_CHANNELS, "%s: channels must be 1 .. %d (got %d)", who,
                PCC_SAMPLE_MAX_CHANNELS, channels);
    PCC_REQUIRE(tolerance >= PCC_SAMPLE_OWN, "%s: tolerance is PCC_SAMPLE_OWN (-1) or a number of voxels >= 0 (got %d)", who, tolerance);
    PCC_REQUIRE(image, "%s: image required", who);
    PCC_REQUIRE(n == 0 || (coords && total && count && peak), "%s: null cloud or outputs with n > 0", who);
    PCC_REQUIRE(scratch, "%s: z-buffer required", who);
    PCC_REQUIRE(scratch_bytes >= pcc_render_scratch_bytes(a.H, a.W), "%s: scratch too small", who);
    if (n == 0) return PCC_OK;                                // nothing to write, and the z-buffer is scratch: nothing to launch
    const int64_t npix = (int64_t)a.H * a.W;
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    hipLaunchKernelGGL(splat_kernel<View>, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    const int acc = accumulate != 0;
    switch (channels) {
        case 1: launch_sample<View, 1>(st, a, coords, n, zbuf, image, tolerance, acc, total, count, peak); break;
        case 2: launch_sample<View, 2>(st, a, coords, n, zbuf, image, tolerance, acc, total, count, peak); break;
        case 3: launch_sample<View, 3>(st, a, coords, n, zbuf, image, tolerance, acc, total, count, peak); break;
        default: launch_sample<View, 4>(st, a, coords, n, zbuf, image, tolerance, acc, total, count, peak); break;
    }
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

// What the two image-compare entries share; mask == nullptr is the unmasked kernel.
static int compare_images(const char* who, const uint8_t* ref, const uint8_t* img, const uint8_t* mask, int32_t H, int32_t W, void* scratch,
                          int64_t scratch_bytes, double* out, void* stream) {
    PCC_REQUIRE(H >= IC_WIN && W >= IC_WIN, "%s: images must be at least 7 x 7 (got %d x %d)", who, H, W);
    PCC_REQUIRE(H <= RENDER_MAX_DIM && W <= RENDER_MAX_DIM, "%s: H and W must be at most %d (got %d x %d)", who, RENDER_MAX_DIM, H, W);
    PCC_REQUIRE(ref && img && scratch && out, "%s: null pointer", who);
    PCC_REQUIRE(scratch_bytes >= pcc_image_compare_scratch_bytes(H, W), "%s: scratch too small", who);
    const int tiles_x = (W + IC_TILE - 1) / IC_TILE, tiles = tiles_x * ((H + IC_TILE - 1) / IC_TILE);
    hipStream_t st = as_stream(stream);
    double* partials = reinterpret_cast<double*>(scratch);
    if (mask)
        hipLaunchKernelGGL(image_compare_tile_kernel<true>, dim3(tiles), dim3(IC_THREADS), 0, st, ref, img, mask, H, W, tiles_x, partials);
    else
        hipLaunchKernelGGL(image_compare_tile_kernel<false>, dim3(tiles), dim3(IC_THREADS), 0, st, ref, img, mask, H, W, tiles_x, partials);
    hipLaunchKernelGGL(image_compare_sum_kernel, dim3(1), dim3(64), 0, st, partials, tiles, out);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // namespace pcc

using namespace pcc;

extern "C" {

int64_t pcc_render_scratch_bytes(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || H > RENDER_MAX_DIM || W > RENDER_MAX_DIM) return 0;
    return (int64_t)H * W * 8;
}

int64_t pcc_visibility_scratch_bytes(int32_t H, int32_t W) { return pcc_render_scratch_bytes(H, W); }

int pcc_render_view(const int32_t* coords, const uint8_t* rgb8, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front,
                    int32_t u_min, int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size, int32_t H, int32_t W,
                    const uint8_t* background, void* scratch, int64_t scratch_bytes, uint8_t* image, void* stream) {
    if (int rc = check_view("pcc_render_view", right, up, front, scale, point_size, H, W, n)) return rc;
    return draw("pcc_render_view", make_view(right, up, front, u_min, v_max, ox, oy, scale, point_size, H, W), coords, rgb8, n, background,
                scratch, scratch_bytes, image, stream);
}

int pcc_view_visibility(const int32_t* coords, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front, int32_t u_min,
                        int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size, int32_t H, int32_t W, void* scratch,
                        int64_t scratch_bytes, int32_t accumulate, int32_t* behind, int32_t* won, void* stream) {
    if (int rc = check_view("pcc_view_visibility", right, up, front, scale, point_size, H, W, n)) return rc;
    return look_back("pcc_view_visibility", make_view(right, up, front, u_min, v_max, ox, oy, scale, point_size, H, W), coords, n, scratch,
                     scratch_bytes, accumulate, behind, won, nullptr, stream);
}

int pcc_render_camera(const int32_t* coords, const uint8_t* rgb8, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q,
                      int32_t near_q, int32_t H, int32_t W, int32_t ps_q, const uint8_t* background, void* scratch, int64_t scratch_bytes,
                      uint8_t* image, void* stream) {
    if (int rc = check_camera("pcc_render_camera", pos_q, axes_q, focal_q, near_q, ps_q, H, W, n)) return rc;
    return draw("pcc_render_camera", make_camera(pos_q, axes_q, focal_q, near_q, ps_q, H, W), coords, rgb8, n, background, scratch,
                scratch_bytes, image, stream);
}

int pcc_camera_visibility(const int32_t* coords, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q, int32_t near_q,
                          int32_t H, int32_t W, int32_t ps_q, void* scratch, int64_t scratch_bytes, int32_t accumulate, int32_t* behind,
                          int32_t* won, int32_t* depth, void* stream) {
    if (int rc = check_camera("pcc_camera_visibility", pos_q, axes_q, focal_q, near_q, ps_q, H, W, n)) return rc;
    return look_back("pcc_camera_visibility", make_camera(pos_q, axes_q, focal_q, near_q, ps_q, H, W), coords, n, scratch, scratch_bytes,
                     accumulate, behind, won, depth, stream);
}

int pcc_view_buffers(const int32_t* coords, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front, int32_t u_min,
                     int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size, int32_t H, int32_t W, void* scratch,
                     int64_t scratch_bytes, int32_t* index, int32_t* depth, void* stream) {
    if (int rc = check_view("pcc_view_buffers", right, up, front, scale, point_size, H, W, n)) return rc;
    return show_buffers("pcc_view_buffers", make_view(right, up, front, u_min, v_max, ox, oy, scale, point_size, H, W), coords, n, scratch,
                        scratch_bytes, index, depth, stream);
}

int pcc_camera_buffers(const int32_t* coords, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q, int32_t near_q,
                       int32_t H, int32_t W, int32_t ps_q, void* scratch, int64_t scratch_bytes, int32_t* index, int32_t* depth,
                       void* stream) {
    if (int rc = check_camera("pcc_camera_buffers", pos_q, axes_q, focal_q, near_q, ps_q, H, W, n)) return rc;
    return show_buffers("pcc_camera_buffers", make_camera(pos_q, axes_q, focal_q, near_q, ps_q, H, W), coords, n, scratch, scratch_bytes,
                        index, depth, stream);
}

int pcc_view_sample(const int32_t* coords, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front, int32_t u_min,
                    int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size, int32_t H, int32_t W, void* scratch,
                    int64_t scratch_bytes, int32_t accumulate, const int32_t* image, int32_t channels, int32_t tolerance, int64_t* total,
                    int32_t* count, int32_t* peak, void* stream) {
    if (int rc = check_view("pcc_view_sample", right, up, front, scale, point_size, H, W, n)) return rc;
    return sample_back("pcc_view_sample", make_view(right, up, front, u_min, v_max, ox, oy, scale, point_size, H, W), coords, n, scratch,
                       scratch_bytes, accumulate, image, channels, tolerance, total, count, peak, stream);
}

int pcc_camera_sample(const int32_t* coords, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q, int32_t near_q,
                      int32_t H, int32_t W, int32_t ps_q, void* scratch, int64_t scratch_bytes, int32_t accumulate, const int32_t* image,
                      int32_t channels, int32_t tolerance, int64_t* total, int32_t* count, int32_t* peak, void* stream) {
    if (int rc = check_camera("pcc_camera_sample", pos_q, axes_q, focal_q, near_q, ps_q, H, W, n)) return rc;
    return sample_back("pcc_camera_sample", make_camera(pos_q, axes_q, focal_q, near_q, ps_q, H, W), coords, n, scratch, scratch_bytes,
                       accumulate, image, channels, tolerance, total, count, peak, stream);
}

int32_t pcc_image_compare_tile(void) { return IC_TILE; }

int64_t pcc_image_compare_scratch_bytes(int32_t H, int32_t W) {
    if (H < IC_WIN || W < IC_WIN || H > RENDER_MAX_DIM || W > RENDER_MAX_DIM) return 0;
    return (int64_t)((H + IC_TILE - 1) / IC_TILE) * ((W + IC_TILE - 1) / IC_TILE) * 8 * (int64_t)sizeof(double);
}

int pcc_image_compare(const uint8_t* ref, const uint8_t* img, int32_t H, int32_t W, void* scratch, int64_t scratch_bytes, double* out,
                      void* stream) {
    return compare_images("pcc_image_compare", ref, img, nullptr, H, W, scratch, scratch_bytes, out, stream);
}

int pcc_image_compare_masked(const uint8_t* ref, const uint8_t* img, const uint8_t* mask, int32_t H, int32_t W, void* scratch,
                             int64_t scratch_bytes, double* out, void* stream) {
    PCC_REQUIRE(mask, "pcc_image_compare_masked: mask required");
    return compare_images("pcc_image_compare_masked", ref, img, mask, H, W, scratch, scratch_bytes, out, stream);
}

}  // extern "C"
