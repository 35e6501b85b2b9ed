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
// Latency bound like nn_search_kernel: one thread per point, 7 / 33 / 123 / 2,109 probes at R = 1 / 2 / 3 / 8.  The 3 x 3
// matrix and its eigenvectors are named scalars — an indexed array would live in scratch memory.
#include "common.h"

namespace pcc {

constexpr int NORMAL_SWEEPS = 12;
constexpr int NORMAL_MAX_RADIUS = 8;

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix; r is the third index.  app, aqq, apq: the pair's
// entries; apr, aqr: their couplings to r; (v0p, v0q), (v1p, v1q), (v2p, v2q): columns p and q of the eigenvector matrix.
__host__ __device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p,
                                                       double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));      // the smaller root: |angle| <= pi/4
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double pr = apr, qr = aqr;
    apr = c * pr - s * qr;
    aqr = s * pr + c * qr;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx xy xz; xy yy yz; xz yz zz).  Equal smallest
// diagonal entries resolve to the lowest column.
__host__ __device__ __forceinline__ void smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22,
                                                              double& nx, double& ny, double& nz) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < NORMAL_SWEEPS; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
    double lo = a00;
    nx = v00; ny = v10; nz = v20;
    if (a11 < lo) { lo = a11; nx = v01; ny = v11; nz = v21; }
    if (a22 < lo) { nx = v02; ny = v12; nz = v22; }
    const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
    nx *= inv; ny *= inv; nz *= inv;
}

__global__ __launch_bounds__(256) void estimate_normals_kernel(const int32_t* __restrict__ coords, int64_t n,
                                                               const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                               uint64_t mask, int shift, int radius, int orient_mode, double ox, double oy,
                                                               double oz, double* __restrict__ normals, int32_t* __restrict__ count,
                                                               int64_t* __restrict__ moments) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = coords[4 * i], x = coords[4 * i + 1], y = coords[4 * i + 2], z = coords[4 * i + 3];
    const int r2 = radius * radius;
    int cnt = 0, sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    for (int dx = -radius; dx <= radius; ++dx) {
        for (int dy = -radius; dy <= radius; ++dy) {
            const int rest = r2 - dx * dx - dy * dy;
            if (rest < 0) continue;
            for (int dz = -radius; dz <= radius; ++dz) {
                if (dz * dz > rest) continue;
                // a coordinate below zero (or past the cloud) packs to a key no row holds: the probe misses
                if (table_find(keys, vals, mask, shift, pack_key(b, x + dx, y + dy, z + dz)) < 0) continue;
                ++cnt;
                sx += dx; sy += dy; sz += dz;
                sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
                syy += dy * dy; syz += dy * dz; szz += dz * dz;
            }
        }
    }
    const int64_t c = cnt;
    const int64_t mxx = c * sxx - (int64_t)sx * sx, mxy = c * sxy - (int64_t)sx * sy, mxz = c * sxz - (int64_t)sx * sz;
    const int64_t myy = c * syy - (int64_t)sy * sy, myz = c * syz - (int64_t)sy * sz, mzz = c * szz - (int64_t)sz * sz;
    if (count) count[i] = cnt;
    if (moments) {
        int64_t* m = moments + 6 * i;
        m[0] = mxx; m[1] = mxy; m[2] = mxz; m[3] = myy; m[4] = myz; m[5] = mzz;
    }
    const int64_t minors = (mxx * myy - mxy * mxy) + (mxx * mzz - mxz * mxz) + (myy * mzz - myz * myz);
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (cnt >= 3 && minors > 0) {
        smallest_eigenvector((double)mxx, (double)mxy, (double)mxz, (double)myy, (double)myz, (double)mzz, nx, ny, nz);
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
