// Surface normals of a voxelised point cloud (point-to-plane / D2 PSNR, facing quality maps).
//
// Replaces open3d's estimate_normals (evaluate_view_dep.py:354-376: a KD-tree radius search and a covariance
// eigen-decomposition per point).  On an integer grid the neighbourhood of a point p is the set of occupied voxels q with
// d = q - p, d.d <= R^2 (p included), found by probing the cloud's own hashed-voxel table at every lattice offset of the
// ball.  The moments are exact integers: S1 = sum d, S2 = sum d d^T, M = count * S2 - S1 S1^T (count^2 times the
// covariance; |M| < 3e8 and its 2 x 2 minors < 2^63 for R <= 8).  A point is valid when count >= 3 and the three principal
// 2 x 2 minors of M sum to > 0 (rank >= 2: the neighbours are not collinear), tested in int64; an invalid point gets the
// normal (0, 0, 0).  The normal of a valid point is the unit eigenvector of M's smallest eigenvalue, by a cyclic Jacobi
// iteration in float64 with a fixed pair order (0,1), (0,2), (1,2) and a fixed number of sweeps: the same input gives
// the same bits on every run.
//
// Latency bound like nn_search_kernel: one thread per point, 7 / 33 / 123 / 2,109 probes at R = 1 / 2 / 3 / 8.  The ball's
// moment loop and the Jacobi iteration live in ball_moments.h, which pcqm.hip shares.
#include "ball_moments.h"

namespace pcc {

__global__ __launch_bounds__(256) void estimate_normals_kernel(const int32_t* __restrict__ coords, int64_t n,
                                                               const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                               uint64_t mask, int shift, int radius, int orient_mode, double ox, double oy,
                                                               double oz, double* __restrict__ normals, int32_t* __restrict__ count,
                                                               int64_t* __restrict__ moments) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = coords[4 * i], x = coords[4 * i + 1], y = coords[4 * i + 2], z = coords[4 * i + 3];
    const BallMoments m = ball_moments(keys, vals, mask, shift, b, x, y, z, radius);
    if (count) count[i] = m.cnt;
    if (moments) {
        int64_t* o = moments + 6 * i;
        o[0] = m.xx; o[1] = m.xy; o[2] = m.xz; o[3] = m.yy; o[4] = m.yz; o[5] = m.zz;
    }
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (ball_spans_a_plane(m)) {
        smallest_eigenvector((double)m.xx, (double)m.xy, (double)m.xz, (double)m.yy, (double)m.yz, (double)m.zz, nx, ny, nz);
        double dot = 0.0;
        if (orient_mode == 1) dot = nx * ox + ny * oy + nz * oz;
        if (orient_mode == 2) dot = nx * (ox - (double)x) + ny * (oy - (double)y) + nz * (oz - (double)z);
        if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    }
    normals[3 * i] = nx; normals[3 * i + 1] = ny; normals[3 * i + 2] = nz;
}

}  // namespace pcc

using namespace pcc;

extern "C" {

int pcc_estimate_normals(const int32_t* coords, int64_t n, const uint64_t* keys, const int32_t* vals, int64_t cap, int32_t tensor_stride,
                         int32_t radius, int32_t orient_mode, const double* orient, double* normals, int32_t* count, int64_t* moments,
                         void* stream) {
    PCC_REQUIRE(cap >= 2 && (cap & (cap - 1)) == 0, "pcc_estimate_normals: table capacity must be a power of two");
    PCC_REQUIRE(radius >= 1 && radius <= NORMAL_MAX_RADIUS, "pcc_estimate_normals: radius must be 1 .. 8");
    PCC_REQUIRE(tensor_stride >= 1, "pcc_estimate_normals: tensor stride must be >= 1");
    PCC_REQUIRE(orient_mode >= 0 && orient_mode <= 2, "pcc_estimate_normals: orient_mode must be 0 (none), 1 (direction) or 2 (camera)");
    PCC_REQUIRE(orient_mode == 0 || orient != nullptr, "pcc_estimate_normals: orientation needs its 3 doubles");
    PCC_REQUIRE(normals != nullptr, "pcc_estimate_normals: output required");
    if (n <= 0) return PCC_OK;
    const double ox = orient_mode ? orient[0] : 0.0, oy = orient_mode ? orient[1] : 0.0, oz = orient_mode ? orient[2] : 0.0;
    hipLaunchKernelGGL(estimate_normals_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), coords, n, keys, vals,
                       (uint64_t)cap - 1, grid_shift_of(tensor_stride), radius, orient_mode, ox, oy, oz, normals, count, moments);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
