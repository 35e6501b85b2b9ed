// The radius-R ball of a voxel and the eigen-decomposition of its moments, shared by the surface normals (normals.hip) and
// the surface variation of the perceptual metric (pcqm.hip).
//
// The neighbourhood of a point p is the set of occupied voxels q of its batch item with d = q - p, d.d <= R^2 (p included),
// found by probing the cloud's own hashed-voxel table at every lattice offset of the ball.  The moments are exact integers:
// S1 = sum d, S2 = sum d d^T, M = count * S2 - S1 S1^T (count^2 times the covariance; |M| < 3e8 and its 2 x 2 minors < 2^63
// for R <= 8).  The eigen-decomposition is a cyclic Jacobi iteration in float64 with a fixed pair order (0,1), (0,2), (1,2)
// and a fixed number of sweeps: the same input gives the same bits on every run.  The 3 x 3 matrix and its eigenvectors are
// named scalars — an indexed array would live in scratch memory.
#pragma once
#include "common.h"

namespace pcc {

constexpr int NORMAL_SWEEPS = 12;
constexpr int NORMAL_MAX_RADIUS = 8;

// count and the upper triangle of M of one ball
struct BallMoments {
    int cnt;
    int64_t xx, xy, xz, yy, yz, zz;
};

__device__ __forceinline__ BallMoments ball_moments(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals, uint64_t mask,
                                                    int shift, int b, int x, int y, int z, int radius) {
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
    BallMoments m;
    m.cnt = cnt;
    m.xx = c * sxx - (int64_t)sx * sx; m.xy = c * sxy - (int64_t)sx * sy; m.xz = c * sxz - (int64_t)sx * sz;
    m.yy = c * syy - (int64_t)sy * sy; m.yz = c * syz - (int64_t)sy * sz; m.zz = c * szz - (int64_t)sz * sz;
    return m;
}

// at least 3 neighbours that are not collinear: the three principal 2 x 2 minors of M sum to > 0 (rank >= 2), in int64
__host__ __device__ __forceinline__ bool ball_spans_a_plane(const BallMoments& m) {
    const int64_t minors = (m.xx * m.yy - m.xy * m.xy) + (m.xx * m.zz - m.xz * m.xz) + (m.yy * m.zz - m.yz * m.yz);
    return m.cnt >= 3 && minors > 0;
}

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

// The fixed-order sweeps on the symmetric matrix (a00 a01 a02; a01 a11 a12; a02 a12 a22): on return its diagonal holds the
// eigenvalues and column k of (v00 v01 v02; v10 v11 v12; v20 v21 v22), which enters as the identity, the eigenvector of akk.
__host__ __device__ __forceinline__ void jacobi_sweeps(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22,
                                                       double& v00, double& v01, double& v02, double& v10, double& v11, double& v12,
                                                       double& v20, double& v21, double& v22) {
#pragma unroll 1
    for (int sweep = 0; sweep < NORMAL_SWEEPS; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
        jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
        jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
    }
}

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx xy xz; xy yy yz; xz yz zz).  Equal smallest
// diagonal entries resolve to the lowest column.
__host__ __device__ __forceinline__ void smallest_eigenvector(double a00, double a01, double a02, double a11, double a12, double a22,
                                                              double& nx, double& ny, double& nz) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    jacobi_sweeps(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    double lo = a00;
    nx = v00; ny = v10; nz = v20;
    if (a11 < lo) { lo = a11; nx = v01; ny = v11; nz = v21; }
    if (a22 < lo) { nx = v02; ny = v12; nz = v22; }
    const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
    nx *= inv; ny *= inv; nz *= inv;
}

// Surface variation l0 / (l0 + l1 + l2) of the same matrix, l0 its smallest eigenvalue: 0 on a plane, 1/3 where the
// neighbours spread evenly in space.  M is positive semi-definite, so an l0 that the rotations left below zero counts as 0.
__host__ __device__ __forceinline__ double surface_variation_of(double a00, double a01, double a02, double a11, double a12, double a22) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    jacobi_sweeps(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    double lo = a00;
    if (a11 < lo) lo = a11;
    if (a22 < lo) lo = a22;
    if (lo < 0.0) lo = 0.0;
    return lo / ((a00 + a11) + a22);
}

}  // namespace pcc
