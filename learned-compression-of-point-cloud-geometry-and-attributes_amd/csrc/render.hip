// View rendering and view PSNR / SSIM for the view-dependent evaluation (evaluate_view_dep.py:102-305).
//
// pcc_render_view replaces render_pointviews (evaluate_view_dep.py:308-348: an open3d OpenGL window, which is neither
// available without a display nor reproducible pixel for pixel) by an exact integer projection of a voxelised cloud: an
// orthographic z-buffer splat along a signed coordinate axis — every view the reference uses is one
// (evaluate_view_dep.py:46-57).
//
//   u = right . p, v = up . p, d = front . p              (front points from the object to the camera, as open3d's set_front)
//   the point covers columns (u - u_min) scale + ox + i and rows (v_max - v) scale + oy + j,  i, j in [0, point_size)
//   pixels outside the image are dropped one by one; the pixel shows the point with the largest d and, among equal d,
//   the lowest row index; untouched pixels show the background
//
// Three kernels: the z-buffer is cleared to 0; one thread per point does point_size^2 64-bit atomicMax of the word
// ((d + 2^18) << 32) | (0xFFFFFFFF - row); one thread per four pixels resolves the words to colours.  A maximum does not depend
// on the order its operands arrive in, so the image is bitwise reproducible although the splat is atomic.  |d| <= COORD_LIMIT
// < 2^18, so d + 2^18 is positive and the word of a drawn pixel is never 0; a row with a coordinate outside the range draws
// nothing.  Atomic bound: n point_size^2 64-bit atomics on H W words.
//
// pcc_view_visibility is the way back from the pixels to the points: the same clear and splat, then one thread per point walks
// its splat again and reads how far the point lies behind the z-buffer front (`behind`, the minimum over its pixels) and how
// many pixels it owns (`won`).  No image is resolved.
//
// pcc_render_camera and pcc_camera_visibility are the same two operators for a pinhole camera at a position: a perspective
// projection in int64 (camera_project below) between the shared clear and resolve kernels, and a walk back that also
// returns each point's depth.
//
// pcc_image_compare replaces rgb2yuv +peak_signal_noise_ratio + structural_similarity (evaluate_view_dep.py:196-204) by
// their raw sums in float64: one workgroup per IC_TILE x IC_TILE tile converts the tile and its 6-pixel apron to YUV one
// channel at a time into LDS, adds the squared differences of the pixels it owns and the SSIM map values of the 7 x 7
// windows whose top-left pixel it owns, reduces them over a fixed tree and stores its eight partials; a second kernel
// adds the partials in ascending workgroup order.  No float atomics: the result is bitwise reproducible.  Separate
// multiplies and adds throughout (the library is built with -ffp-contract=off).
#include "common.h"

namespace pcc {

constexpr int RENDER_DEPTH_BIAS = 1 << 18;
constexpr int RENDER_MAX_DIM = 8192;

struct RenderView {
    int32_t r[3], u[3], f[3];
    int32_t u_min, v_max, ox, oy, scale, point_size, H, W;
};

__global__ __launch_bounds__(256) void render_clear_kernel(uint64_t* __restrict__ zbuf, int64_t npix) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npix) zbuf[i] = 0ull;
}

__global__ __launch_bounds__(256) void render_splat_kernel(const int32_t* __restrict__ coords, int64_t n, RenderView a,
                                                           uint64_t* __restrict__ zbuf) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];                  // (batch, x, y, z): the batch is ignored
    if (!coord_in_range(0, c.y, c.z, c.w)) return;
    const int u = a.r[0] * c.y + a.r[1] * c.z + a.r[2] * c.w;
    const int v = a.u[0] * c.y + a.u[1] * c.z + a.u[2] * c.w;
    const int d = a.f[0] * c.y + a.f[1] * c.z + a.f[2] * c.w;
    const uint64_t word = ((uint64_t)(uint32_t)(d + RENDER_DEPTH_BIAS) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)row);
    // 64-bit positions: (u - u_min) * scale stays below 2^19 * 64, but u_min / ox / oy are the caller's
    const int64_t px0 = ((int64_t)u - a.u_min) * a.scale + a.ox, py0 = ((int64_t)a.v_max - v) * a.scale + a.oy;
    for (int j = 0; j < a.point_size; ++j) {
        const int64_t py = py0 + j;
        if (py < 0 || py >= a.H) continue;
        for (int i = 0; i < a.point_size; ++i) {
            const int64_t px = px0 + i;
            if (px < 0 || px >= a.W) continue;
            atomicMax(reinterpret_cast<unsigned long long*>(zbuf) + (py * a.W + px), (unsigned long long)word);
        }
    }
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
// (d of the pixel's winner) - (d of this point) over its pixels inside the image, won = the pixels whose word is this row's own.
// Every pixel of the splat holds a word of depth >= d (this row took part in its maximum), so behind >= 0, and it is 0 exactly
// where the front depth of a pixel is this point's; the tie to the lowest row decides only `won`.  A thread owns its row's two
// outputs: no atomics, and `accumulate` is a plain read-modify-write (min of behind, sum of won).
__global__ __launch_bounds__(256) void visibility_gather_kernel(const int32_t* __restrict__ coords, int64_t n, RenderView a,
                                                                const uint64_t* __restrict__ zbuf, int accumulate,
                                                                int32_t* __restrict__ behind, int32_t* __restrict__ won) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];
    int32_t best = PCC_VIS_OFFSCREEN, count = 0;
    if (coord_in_range(0, c.y, c.z, c.w)) {
        const int u = a.r[0] * c.y + a.r[1] * c.z + a.r[2] * c.w;
        const int v = a.u[0] * c.y + a.u[1] * c.z + a.u[2] * c.w;
        const int d = a.f[0] * c.y + a.f[1] * c.z + a.f[2] * c.w;
        const uint64_t own = ((uint64_t)(uint32_t)(d + RENDER_DEPTH_BIAS) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)row);
        const int64_t px0 = ((int64_t)u - a.u_min) * a.scale + a.ox, py0 = ((int64_t)a.v_max - v) * a.scale + a.oy;
        for (int j = 0; j < a.point_size; ++j) {
            const int64_t py = py0 + j;
            if (py < 0 || py >= a.H) continue;
            for (int i = 0; i < a.point_size; ++i) {
                const int64_t px = px0 + i;
                if (px < 0 || px >= a.W) continue;
                const uint64_t word = zbuf[py * a.W + px];
                const int32_t gap = (int32_t)(uint32_t)(word >> 32) - RENDER_DEPTH_BIAS - d;     // 0 .. 2 COORD_LIMIT
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
}

// ---- pinhole camera: perspective splat and walk back, all int64 ----
// The camera crosses the ABI as integers only (pcc_hip.h): pos in 1/16 voxel, the three axes in 2^-14, focal in 1/16 pixel,
// near in 1/16 voxel, the voxel edge ps in 1/16 voxel.  For a row p:
//   e = 16 p - pos;  U = right . e, V = up . e, D = -(front . e)   (2^-18 voxel; front points from the scene to the camera)
//   drawn <=> D >= near 2^14;  X = floor(focal U / D), Y = floor(focal V / D)   (1/16 pixel from the principal point)
//   s = clamp(ceil(focal ps 2^10 / D), 1, 16);  col0 = floor((8 W + X - 8 s) / 16), row0 = floor((8 H - Y - 8 s) / 16)
//   depth key dk = D >> 10 (1/256 voxel); the z-buffer word is ((0x7FFFFFFF - dk) << 32) | (0xFFFFFFFF - row)
// Bounds, which the host entry re-derives from the arguments it is given (camera_check): |e_k| <= |pos_k| + 16 COORD_LIMIT <
// 2^24 + 2^21, an axis row has entries of at most 2^14, so |U|, |V|, |D| < 3 2^14 (2^24 + 2^21) < 2^40, |focal U| < 2^60, dk <
// 2^30 and dk >= 16 near >= 16: the high half of a drawn pixel's word is in (2^30, 2^31) and never 0.  The clear and resolve
// kernels above are shared with the orthographic view: the word layout is theirs, the larger word is the nearer point and,
// among equal dk, the lower row.
struct CameraView {
    int32_t pos[3], ax[3][3];
    int32_t focal, near, ps, H, W;
};

struct CameraSplat {                 // the splat of one point clipped to the image: rows r0 .. r1 - 1, columns c0 .. c1 - 1
    int32_t r0, r1, c0, c1;
    uint32_t dk;
};

// floor(a / b) for b > 0, through one unsigned division (C++'s `/` truncates towards zero)
__device__ __forceinline__ int64_t camera_floordiv(int64_t a, uint64_t b) {
    return a >= 0 ? (int64_t)((uint64_t)a / b) : -(int64_t)(((uint64_t)(-a) + b - 1) / b);
}

// false when the row draws nothing: a coordinate out of range, or in front of the near plane (behind the camera included)
__device__ __forceinline__ bool camera_project(const int4 c, const CameraView& a, CameraSplat& out) {
    if (!coord_in_range(0, c.y, c.z, c.w)) return false;
    const int64_t e0 = 16 * (int64_t)c.y - a.pos[0], e1 = 16 * (int64_t)c.z - a.pos[1], e2 = 16 * (int64_t)c.w - a.pos[2];
    const int64_t U = a.ax[0][0] * e0 + a.ax[0][1] * e1 + a.ax[0][2] * e2;
    const int64_t V = a.ax[1][0] * e0 + a.ax[1][1] * e1 + a.ax[1][2] * e2;
    const int64_t D = -(a.ax[2][0] * e0 + a.ax[2][1] * e1 + a.ax[2][2] * e2);
    if (D < ((int64_t)a.near << 14)) return false;
    const uint64_t d = (uint64_t)D;
    const int64_t X = camera_floordiv((int64_t)a.focal * U, d), Y = camera_floordiv((int64_t)a.focal * V, d);
    const uint64_t edge = ((((uint64_t)a.focal * (uint64_t)a.ps) << 10) + d - 1) / d;
    const int64_t s = edge < 1 ? 1 : (edge > 16 ? 16 : (int64_t)edge);
    const int64_t col0 = (8 * (int64_t)a.W + X - 8 * s) >> 4, row0 = (8 * (int64_t)a.H - Y - 8 * s) >> 4;   // >> floors
    const int64_t c0 = col0 < 0 ? 0 : col0, c1 = col0 + s > a.W ? a.W : col0 + s;
    const int64_t r0 = row0 < 0 ? 0 : row0, r1 = row0 + s > a.H ? a.H : row0 + s;
    out.dk = (uint32_t)(d >> 10);
    // an empty range is stored as 0 .. 0: the clipped bounds of a splat far outside the image do not fit 32 bits
    const bool inside = c0 < c1 && r0 < r1;
    out.c0 = inside ? (int32_t)c0 : 0; out.c1 = inside ? (int32_t)c1 : 0;
    out.r0 = inside ? (int32_t)r0 : 0; out.r1 = inside ? (int32_t)r1 : 0;
    return true;
}

__device__ __forceinline__ uint64_t camera_word(uint32_t dk, int64_t row) {
    return ((uint64_t)(0x7FFFFFFFu - dk) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)row);
}

// one thread per point, at most 16 x 16 atomics each
__global__ __launch_bounds__(256) void camera_splat_kernel(const int32_t* __restrict__ coords, int64_t n, CameraView a,
                                                           uint64_t* __restrict__ zbuf) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];                  // (batch, x, y, z): the batch is ignored
    CameraSplat sp;
    if (!camera_project(c, a, sp)) return;
    const uint64_t word = camera_word(sp.dk, row);
    for (int32_t py = sp.r0; py < sp.r1; ++py)
        for (int32_t px = sp.c0; px < sp.c1; ++px)
            atomicMax(reinterpret_cast<unsigned long long*>(zbuf) + ((int64_t)py * a.W + px), (unsigned long long)word);
}

// the way back, as visibility_gather_kernel: behind in whole voxels (dk differences >> 8), won, and the point's own depth key
__global__ __launch_bounds__(256) void camera_gather_kernel(const int32_t* __restrict__ coords, int64_t n, CameraView a,
                                                            const uint64_t* __restrict__ zbuf, int accumulate,
                                                            int32_t* __restrict__ behind, int32_t* __restrict__ won,
                                                            int32_t* __restrict__ depth) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[row];
    int32_t best = PCC_VIS_OFFSCREEN, count = 0, dist = PCC_VIS_OFFSCREEN;
    CameraSplat sp;
    if (camera_project(c, a, sp) && sp.r0 < sp.r1) {
        const uint64_t own = camera_word(sp.dk, row);
        dist = (int32_t)sp.dk;
        for (int32_t py = sp.r0; py < sp.r1; ++py) {
            for (int32_t px = sp.c0; px < sp.c1; ++px) {
                const uint64_t word = zbuf[(int64_t)py * a.W + px];
                const uint32_t dk_front = 0x7FFFFFFFu - (uint32_t)(word >> 32);     // <= dk: this row took part in the maximum
                const int32_t gap = (int32_t)((sp.dk - dk_front) >> 8);
                best = gap < best ? gap : best;
                count += word == own;
            }
        }
    }
    if (accumulate) {
        const int32_t old_b = behind[row], old_d = depth[row];
        best = old_b < best ? old_b : best;
        dist = old_d < dist ? old_d : dist;
        count += won[row];
    }
    behind[row] = best;
    won[row] = count;
    depth[row] = dist;
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

__global__ __launch_bounds__(IC_THREADS) void image_compare_tile_kernel(const uint8_t* __restrict__ ref, const uint8_t* __restrict__ img,
                                                                        int H, int W, int tiles_x, double* __restrict__ partials) {
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
                    const double diff = x - y;
                    sse[ch] = sse[ch] + diff * diff;
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
    PCC_REQUIRE(H >= 1 && H <= RENDER_MAX_DIM && W >= 1 && W <= RENDER_MAX_DIM, "%s: H and W must be 1 .. %d (got %d x %d)", who,
                RENDER_MAX_DIM, H, W);
    PCC_REQUIRE(n >= 0 && n <= 0xFFFFFFFEll, "%s: 0 .. 2^32 - 2 points", who);
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
    PCC_REQUIRE(H >= 1 && H <= RENDER_MAX_DIM && W >= 1 && W <= RENDER_MAX_DIM, "%s: H and W must be 1 .. %d (got %d x %d)", who,
                RENDER_MAX_DIM, H, W);
    PCC_REQUIRE(n >= 0 && n <= 0xFFFFFFFEll, "%s: 0 .. 2^32 - 2 points", who);
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

}  // namespace pcc

using namespace pcc;

extern "C" {

int64_t pcc_render_scratch_bytes(int32_t H, int32_t W) {
    if (H < 1 || W < 1 || H > RENDER_MAX_DIM || W > RENDER_MAX_DIM) return 0;
    return (int64_t)H * W * 8;
}

int pcc_render_view(const int32_t* coords, const uint8_t* rgb8, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front,
                    int32_t u_min, int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size, int32_t H, int32_t W,
                    const uint8_t* background, void* scratch, int64_t scratch_bytes, uint8_t* image, void* stream) {
    if (int rc = check_view("pcc_render_view", right, up, front, scale, point_size, H, W, n)) return rc;
    PCC_REQUIRE(background, "pcc_render_view: background required");
    PCC_REQUIRE(n == 0 || (coords && rgb8), "pcc_render_view: null cloud with n > 0");
    PCC_REQUIRE(scratch && image, "pcc_render_view: z-buffer and image required");
    PCC_REQUIRE(scratch_bytes >= pcc_render_scratch_bytes(H, W), "pcc_render_view: scratch too small");
    const RenderView a = make_view(right, up, front, u_min, v_max, ox, oy, scale, point_size, H, W);
    const int64_t npix = (int64_t)H * W;
    const uint32_t bg = (uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16);
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    if (n > 0) hipLaunchKernelGGL(render_splat_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    hipLaunchKernelGGL(render_resolve_kernel, dim3(blocks_for((npix + 3) / 4, 256)), dim3(256), 0, st, zbuf, rgb8, bg, npix, image);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int64_t pcc_visibility_scratch_bytes(int32_t H, int32_t W) { return pcc_render_scratch_bytes(H, W); }

int pcc_view_visibility(const int32_t* coords, int64_t n, const int32_t* right, const int32_t* up, const int32_t* front, int32_t u_min,
                        int32_t v_max, int32_t ox, int32_t oy, int32_t scale, int32_t point_size, int32_t H, int32_t W, void* scratch,
                        int64_t scratch_bytes, int32_t accumulate, int32_t* behind, int32_t* won, void* stream) {
    if (int rc = check_view("pcc_view_visibility", right, up, front, scale, point_size, H, W, n)) return rc;
    PCC_REQUIRE(n == 0 || (coords && behind && won), "pcc_view_visibility: null cloud or outputs with n > 0");
    PCC_REQUIRE(scratch, "pcc_view_visibility: z-buffer required");
    PCC_REQUIRE(scratch_bytes >= pcc_visibility_scratch_bytes(H, W), "pcc_view_visibility: scratch too small");
    if (n == 0) return PCC_OK;                                // nothing to write, and the z-buffer is scratch: nothing to launch
    const RenderView a = make_view(right, up, front, u_min, v_max, ox, oy, scale, point_size, H, W);
    const int64_t npix = (int64_t)H * W;
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    hipLaunchKernelGGL(render_splat_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    hipLaunchKernelGGL(visibility_gather_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf, accumulate != 0, behind, won);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_render_camera(const int32_t* coords, const uint8_t* rgb8, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q,
                      int32_t near_q, int32_t H, int32_t W, int32_t ps_q, const uint8_t* background, void* scratch, int64_t scratch_bytes,
                      uint8_t* image, void* stream) {
    if (int rc = check_camera("pcc_render_camera", pos_q, axes_q, focal_q, near_q, ps_q, H, W, n)) return rc;
    PCC_REQUIRE(background, "pcc_render_camera: background required");
    PCC_REQUIRE(n == 0 || (coords && rgb8), "pcc_render_camera: null cloud with n > 0");
    PCC_REQUIRE(scratch && image, "pcc_render_camera: z-buffer and image required");
    PCC_REQUIRE(scratch_bytes >= pcc_render_scratch_bytes(H, W), "pcc_render_camera: scratch too small");
    const CameraView a = make_camera(pos_q, axes_q, focal_q, near_q, ps_q, H, W);
    const int64_t npix = (int64_t)H * W;
    const uint32_t bg = (uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16);
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    if (n > 0) hipLaunchKernelGGL(camera_splat_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    hipLaunchKernelGGL(render_resolve_kernel, dim3(blocks_for((npix + 3) / 4, 256)), dim3(256), 0, st, zbuf, rgb8, bg, npix, image);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_camera_visibility(const int32_t* coords, int64_t n, const int32_t* pos_q, const int32_t* axes_q, int32_t focal_q, int32_t near_q,
                          int32_t H, int32_t W, int32_t ps_q, void* scratch, int64_t scratch_bytes, int32_t accumulate, int32_t* behind,
                          int32_t* won, int32_t* depth, void* stream) {
    if (int rc = check_camera("pcc_camera_visibility", pos_q, axes_q, focal_q, near_q, ps_q, H, W, n)) return rc;
    PCC_REQUIRE(n == 0 || (coords && behind && won && depth), "pcc_camera_visibility: null cloud or outputs with n > 0");
    PCC_REQUIRE(scratch, "pcc_camera_visibility: z-buffer required");
    PCC_REQUIRE(scratch_bytes >= pcc_render_scratch_bytes(H, W), "pcc_camera_visibility: scratch too small");
    if (n == 0) return PCC_OK;                                // nothing to write, and the z-buffer is scratch: nothing to launch
    const CameraView a = make_camera(pos_q, axes_q, focal_q, near_q, ps_q, H, W);
    const int64_t npix = (int64_t)H * W;
    hipStream_t st = as_stream(stream);
    uint64_t* zbuf = reinterpret_cast<uint64_t*>(scratch);
    hipLaunchKernelGGL(render_clear_kernel, dim3(blocks_for(npix, 256)), dim3(256), 0, st, zbuf, npix);
    hipLaunchKernelGGL(camera_splat_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf);
    hipLaunchKernelGGL(camera_gather_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, coords, n, a, zbuf, accumulate != 0, behind, won,
                       depth);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int32_t pcc_image_compare_tile(void) { return IC_TILE; }

int64_t pcc_image_compare_scratch_bytes(int32_t H, int32_t W) {
    if (H < IC_WIN || W < IC_WIN || H > RENDER_MAX_DIM || W > RENDER_MAX_DIM) return 0;
    return (int64_t)((H + IC_TILE - 1) / IC_TILE) * ((W + IC_TILE - 1) / IC_TILE) * 8 * (int64_t)sizeof(double);
}

int pcc_image_compare(const uint8_t* ref, const uint8_t* img, int32_t H, int32_t W, void* scratch, int64_t scratch_bytes, double* out,
                      void* stream) {
    PCC_REQUIRE(H >= IC_WIN && W >= IC_WIN, "pcc_image_compare: images must be at least 7 x 7 (got %d x %d)", H, W);
    PCC_REQUIRE(H <= RENDER_MAX_DIM && W <= RENDER_MAX_DIM, "pcc_image_compare: H and W must be at most %d (got %d x %d)", RENDER_MAX_DIM, H, W);
    PCC_REQUIRE(ref && img && scratch && out, "pcc_image_compare: null pointer");
    PCC_REQUIRE(scratch_bytes >= pcc_image_compare_scratch_bytes(H, W), "pcc_image_compare: scratch too small");
    const int tiles_x = (W + IC_TILE - 1) / IC_TILE, tiles = tiles_x * ((H + IC_TILE - 1) / IC_TILE);
    hipStream_t st = as_stream(stream);
    double* partials = reinterpret_cast<double*>(scratch);
    hipLaunchKernelGGL(image_compare_tile_kernel, dim3(tiles), dim3(IC_THREADS), 0, st, ref, img, H, W, tiles_x, partials);
    hipLaunchKernelGGL(image_compare_sum_kernel, dim3(1), dim3(64), 0, st, partials, tiles, out);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
