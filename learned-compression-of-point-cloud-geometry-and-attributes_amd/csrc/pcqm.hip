// A PCQM-style perceptual quality metric on a voxel grid ("pcqm_voxel"): per-point local statistics of lightness, chroma,
// hue and curvature of a reference cloud R and a distorted cloud D, compared feature by feature and pooled.
//
// The reference's sweep scores PCQM with an external binary (utils.py:290-344: `PCQM ... -fq -r 0.004 -knn 20 -rx 2.0`).  This
// follows PCQM's published structure (Meynet, Nehme, Digne, Lavoue, QoMEX 2020) on an integer grid and does NOT reproduce that
// binary's numbers: the colour space is plain CIELAB (made by the caller), the curvature is the surface variation
// l0 / (l0 + l1 + l2) of the radius-r ball instead of a fitted quadric's mean curvature, and a point of R corresponds to its
// nearest voxel of D instead of its projection onto a fitted quadric.
//
// pcc_surface_variation: kappa per point from the exact integer moments and the fixed-order Jacobi of ball_moments.h (shared
// with normals.hip); 0 where pcc_estimate_normals gives no normal.
//
// pcc_pcqm_features: for a point p of R with centre attributes x(p) and its nearest D voxel p^ = D[nn[p]], both balls of radius
// h are walked once, in ascending (dx, dy, dz) with dz innermost (the table's slots are coherent along z).  A neighbour at
// squared distance d2 has the weight w[d2] of the caller's table: no transcendental function runs here.  Sums are SHIFTED by
// the centre's attributes, u = x_R(q) - x_R(p) over N_R(p) and v = x_D(.) - x_D(p^) on the D side, so that one pass gives
// means and second moments without cancellation against the attribute's magnitude:
//     mean = x(centre) + S[u] / W,   variance = S[u u] / W - (S[u] / W)^2,
//     cross = S[u v'] / W_R - (S[u] / W_R)(S[v'] / W_R),  v' = x_D(D[nn[q]]) - x_D(p^) paired over q in N_R(p)
// (sum w (u - E u)(v' - m) = sum w u v' - E[u] sum w v' for ANY m, because sum w (u - E u) = 0: the D-side mean drops out).
// The 20 accumulators are named scalars: no scratch memory, no spills (checked at build time).
//
// Launch shape: one thread per point, like normals.hip.  Spreading a point's ball over 2, 4 or 8 lanes of a wave (columns dealt
// round-robin, sums folded in a fixed order) was measured on the 850,824-point frame and lost at every width: 49.6 ms with one
// lane against 54.2 / 57.4 / 65.9 ms with 2 / 4 / 8 at h = 8, and 7.2 against 8.4 / 10.2 / 13.2 ms at h = 4 — a frame has thousands
// of waves either way, and neighbouring threads of one wave already walk neighbouring voxels through the same table lines.
//
// Pooling uses no float atomics: every workgroup adds its points' features in a fixed tree and stores the 8 partial sums at
// its own index; a second launch adds the partials in ascending workgroup order.
#include "ball_moments.h"

namespace pcc {

constexpr int PCQM_THREADS = 256;
constexpr int PCQM_MAX_RADIUS = NORMAL_MAX_RADIUS;
constexpr int PCQM_ATTRS = 5;           // L, c, a, b, kappa
constexpr int PCQM_STATS = 18;
constexpr int PCQM_FEATURES = 8;

__global__ __launch_bounds__(256) void surface_variation_kernel(const int32_t* __restrict__ coords, int64_t n,
                                                                const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                                uint64_t mask, int shift, int radius, double* __restrict__ kappa) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = coords[4 * i], x = coords[4 * i + 1], y = coords[4 * i + 2], z = coords[4 * i + 3];
    const BallMoments m = ball_moments(keys, vals, mask, shift, b, x, y, z, radius);
    double k = 0.0;
    if (ball_spans_a_plane(m)) k = surface_variation_of((double)m.xx, (double)m.xy, (double)m.xz, (double)m.yy, (double)m.yz, (double)m.zz);
    kappa[i] = k;
}

struct PcqmArgs {
    const int32_t* coords_r; const uint64_t* keys_r; const int32_t* vals_r; uint64_t mask_r;
    const int32_t* coords_d; const uint64_t* keys_d; const int32_t* vals_d; uint64_t mask_d;
    int64_t n_r, n_d;
    const int32_t* nn;
    const double* attrs_r; const double* attrs_d; const double* w;
    int shift, h;
    double k_l, k_kappa, c_chroma, c_hue;
    double* stats; double* features; double* partials;
};

// |a - b| / (max(a, b) + k)
__device__ __forceinline__ double pcqm_contrast(double a, double b, double k) { return fabs(a - b) / ((a > b ? a : b) + k); }

// the sum of `v` over the workgroup, added in a fixed tree; every thread calls it
__device__ __forceinline__ double pcqm_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = PCQM_THREADS >> 1; s > 0; s >>= 1) {
        if (t < s) red[t] = red[t] + red[t + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(PCQM_THREADS) void pcqm_features_kernel(const PcqmArgs a) {
    __shared__ double red[PCQM_THREADS];
    const int64_t i = (int64_t)blockIdx.x * PCQM_THREADS + threadIdx.x;
    double f1 = 0.0, f2 = 0.0, f3 = 0.0, f4 = 0.0, f5 = 0.0, f6 = 0.0, f7 = 0.0, f8 = 0.0;
    if (i < a.n_r) {
        const int h = a.h, h2 = h * h;
        const double nan = __builtin_nan("");
        const int j = a.nn[i];
        const bool j_ok = (uint32_t)j < (uint32_t)a.n_d;
        const int64_t jc = j_ok ? j : 0;
        const double* cr = a.attrs_r + PCQM_ATTRS * i;
        const double* cd = a.attrs_d + PCQM_ATTRS * jc;
        const double rL = cr[0], rC = cr[1], rA = cr[2], rB = cr[3], rK = cr[4];
        const double dL = cd[0], dC = cd[1], dA = cd[2], dB = cd[3], dK = cd[4];
        // ---- the ball of p in R, each neighbour paired with its own nearest D voxel
        double wr = j_ok ? 0.0 : nan, sL = 0.0, sC = 0.0, sA = 0.0, sB = 0.0, sK = 0.0, sLL = 0.0, sKK = 0.0;
        double tL = 0.0, tK = 0.0, xL = 0.0, xK = 0.0;
        {
            const int b = a.coords_r[4 * i], x = a.coords_r[4 * i + 1], y = a.coords_r[4 * i + 2], z = a.coords_r[4 * i + 3];
            for (int dx = -h; dx <= h; ++dx) {
                for (int dy = -h; dy <= h; ++dy) {
                    const int rest = h2 - dx * dx - dy * dy;
                    if (rest < 0) continue;
                    for (int dz = -h; dz <= h; ++dz) {
                        if (dz * dz > rest) continue;
                        const int q = table_find(a.keys_r, a.vals_r, a.mask_r, a.shift, pack_key(b, x + dx, y + dy, z + dz));
                        if (q < 0) continue;
                        if ((uint32_t)q >= (uint32_t)a.n_r) { wr = nan; continue; }      // a table of another cloud: poison, never read past
                        const double w = a.w[h2 - rest + dz * dz];
                        const double* aq = a.attrs_r + PCQM_ATTRS * (int64_t)q;
                        const double uL = aq[0] - rL, uC = aq[1] - rC, uA = aq[2] - rA, uB = aq[3] - rB, uK = aq[4] - rK;
                        const int jq = a.nn[q];
                        const bool ok = (uint32_t)jq < (uint32_t)a.n_d;
                        const double* bq = a.attrs_d + PCQM_ATTRS * (int64_t)(ok ? jq : 0);
                        const double vL = ok ? bq[0] - dL : nan, vK = ok ? bq[4] - dK : nan;
                        const double wuL = w * uL, wuK = w * uK;
                        wr = wr + w;
                        sL = sL + wuL; sC = sC + w * uC; sA = sA + w * uA; sB = sB + w * uB; sK = sK + wuK;
                        sLL = sLL + wuL * uL; sKK = sKK + wuK * uK;
                        tL = tL + w * vL; tK = tK + w * vK;
                        xL = xL + wuL * vL; xK = xK + wuK * vK;
                    }
                }
            }
        }
        // ---- the ball of p^ in D
        double wd = 0.0, eL = 0.0, eC = 0.0, eA = 0.0, eB = 0.0, eK = 0.0, eLL = 0.0, eKK = 0.0;
        {
            const int b = a.coords_d[4 * jc], x = a.coords_d[4 * jc + 1], y = a.coords_d[4 * jc + 2], z = a.coords_d[4 * jc + 3];
            for (int dx = -h; dx <= h; ++dx) {
                for (int dy = -h; dy <= h; ++dy) {
                    const int rest = h2 - dx * dx - dy * dy;
                    if (rest < 0) continue;
                    for (int dz = -h; dz <= h; ++dz) {
                        if (dz * dz > rest) continue;
                        const int q = table_find(a.keys_d, a.vals_d, a.mask_d, a.shift, pack_key(b, x + dx, y + dy, z + dz));
                        if (q < 0) continue;
                        if ((uint32_t)q >= (uint32_t)a.n_d) { wd = nan; continue; }
                        const double w = a.w[h2 - rest + dz * dz];
                        const double* bq = a.attrs_d + PCQM_ATTRS * (int64_t)q;
                        const double vL = bq[0] - dL, vC = bq[1] - dC, vA = bq[2] - dA, vB = bq[3] - dB, vK = bq[4] - dK;
                        const double wvL = w * vL, wvK = w * vK;
                        wd = wd + w;
                        eL = eL + wvL; eC = eC + w * vC; eA = eA + w * vA; eB = eB + w * vB; eK = eK + wvK;
                        eLL = eLL + wvL * vL; eKK = eKK + wvK * vK;
                    }
                }
            }
        }
        // ---- statistics: the centres are members of their balls and w[0] > 0 in any sensible table, so wr, wd > 0
        const double mrL = sL / wr, mrK = sK / wr, mdL = eL / wd, mdK = eK / wd;
        const double muL = rL + mrL, muC = rC + sC / wr, muA = rA + sA / wr, muB = rB + sB / wr, muK = rK + mrK;
        const double nuL = dL + mdL, nuC = dC + eC / wd, nuA = dA + eA / wd, nuB = dB + eB / wd, nuK = dK + mdK;
        double vrL = sLL / wr - mrL * mrL, vdL = eLL / wd - mdL * mdL, vrK = sKK / wr - mrK * mrK, vdK = eKK / wd - mdK * mdK;
        vrL = vrL < 0.0 ? 0.0 : vrL; vdL = vdL < 0.0 ? 0.0 : vdL; vrK = vrK < 0.0 ? 0.0 : vrK; vdK = vdK < 0.0 ? 0.0 : vdK;
        const double cvL = xL / wr - mrL * (tL / wr), cvK = xK / wr - mrK * (tK / wr);
        if (a.stats) {
            double* s = a.stats + PCQM_STATS * i;
            s[0] = wr; s[1] = wd;
            s[2] = muL; s[3] = muC; s[4] = muA; s[5] = muB; s[6] = muK;
            s[7] = nuL; s[8] = nuC; s[9] = nuA; s[10] = nuB; s[11] = nuK;
            s[12] = vrL; s[13] = vdL; s[14] = cvL; s[15] = vrK; s[16] = vdK; s[17] = cvK;
        }
        // ---- features.  sigma sigma^ is sqrt(v v^), not sqrt(v) sqrt(v^): sqrt(v * v) == v exactly, so identical clouds score 0
        const double ssL = sqrt(vrL * vdL), ssK = sqrt(vrK * vdK);
        const double dc = muC - nuC, da = muA - nuA, db = muB - nuB;
        double dh = (da * da + db * db) - dc * dc;
        dh = dh < 0.0 ? 0.0 : dh;
        f1 = pcqm_contrast(muL, nuL, a.k_l);
        f2 = pcqm_contrast(sqrt(vrL), sqrt(vdL), a.k_l);
        f3 = fabs(ssL - cvL) / (ssL + a.k_l);
        f4 = 1.0 - 1.0 / (a.c_chroma * (dc * dc) + 1.0);
        f5 = 1.0 - 1.0 / (a.c_hue * dh + 1.0);
        f6 = pcqm_contrast(muK, nuK, a.k_kappa);
        f7 = pcqm_contrast(sqrt(vrK), sqrt(vdK), a.k_kappa);
        f8 = fabs(ssK - cvK) / (ssK + a.k_kappa);
        if (a.features) {
            double* f = a.features + PCQM_FEATURES * i;
            f[0] = f1; f[1] = f2; f[2] = f3; f[3] = f4; f[4] = f5; f[5] = f6; f[6] = f7; f[7] = f8;
        }
    }
    if (a.partials) {      // uniform over the launch: every thread reaches the barriers
        double* p = a.partials + PCQM_FEATURES * (int64_t)blockIdx.x;
        const double t1 = pcqm_block_sum(f1, red), t2 = pcqm_block_sum(f2, red), t3 = pcqm_block_sum(f3, red), t4 = pcqm_block_sum(f4, red);
        const double t5 = pcqm_block_sum(f5, red), t6 = pcqm_block_sum(f6, red), t7 = pcqm_block_sum(f7, red), t8 = pcqm_block_sum(f8, red);
        if (threadIdx.x == 0) { p[0] = t1; p[1] = t2; p[2] = t3; p[3] = t4; p[4] = t5; p[5] = t6; p[6] = t7; p[7] = t8; }
    }
}

// thread f adds feature f of every workgroup, in ascending workgroup order; no workgroups: zeros
__global__ __launch_bounds__(64) void pcqm_pool_kernel(const double* __restrict__ partials, int64_t blocks, double* __restrict__ sums) {
    const int f = threadIdx.x;
    if (f >= PCQM_FEATURES) return;
    double acc = 0.0;
    for (int64_t b = 0; b < blocks; ++b) acc = acc + partials[PCQM_FEATURES * b + f];
    sums[f] = acc;
}

static int64_t pcqm_blocks(int64_t n) { return (n + PCQM_THREADS - 1) / PCQM_THREADS; }

}  // namespace pcc

using namespace pcc;

extern "C" {

int pcc_surface_variation(const int32_t* coords, int64_t n, const uint64_t* keys, const int32_t* vals, int64_t cap, int32_t tensor_stride,
                          int32_t radius, double* kappa, void* stream) {
    PCC_REQUIRE(cap >= 2 && (cap & (cap - 1)) == 0, "pcc_surface_variation: table capacity (cap) must be a power of two");
    PCC_REQUIRE(radius >= 1 && radius <= PCQM_MAX_RADIUS, "pcc_surface_variation: radius must be 1 .. 8");
    PCC_REQUIRE(tensor_stride >= 1, "pcc_surface_variation: tensor_stride must be >= 1");
    PCC_REQUIRE(n >= 0, "pcc_surface_variation: n must be >= 0");
    PCC_REQUIRE(kappa != nullptr, "pcc_surface_variation: output kappa required");
    if (n == 0) return PCC_OK;
    PCC_REQUIRE(coords && keys && vals, "pcc_surface_variation: coords, keys and vals required");
    hipLaunchKernelGGL(surface_variation_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), coords, n, keys, vals,
                       (uint64_t)cap - 1, grid_shift_of(tensor_stride), radius, kappa);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int64_t pcc_pcqm_scratch_bytes(int64_t n) {
    if (n < 0 || n > 0x7ffffffe) return 0;
    const int64_t blocks = pcqm_blocks(n);
    return (blocks < 1 ? 1 : blocks) * PCQM_FEATURES * (int64_t)sizeof(double);
}

int pcc_pcqm_features(const int32_t* coords_r, int64_t n_r, const uint64_t* keys_r, const int32_t* vals_r, int64_t cap_r,
                      const int32_t* coords_d, int64_t n_d, const uint64_t* keys_d, const int32_t* vals_d, int64_t cap_d,
                      int32_t tensor_stride, const int32_t* nn, const double* attrs_r, const double* attrs_d, const double* w, int32_t h,
                      const double* constants, double* stats, double* features, double* sums, void* scratch, int64_t scratch_bytes,
                      void* stream) {
    PCC_REQUIRE(h >= 1 && h <= PCQM_MAX_RADIUS, "pcc_pcqm_features: h must be 1 .. 8");
    PCC_REQUIRE(cap_r >= 2 && (cap_r & (cap_r - 1)) == 0, "pcc_pcqm_features: table capacity cap_r must be a power of two");
    PCC_REQUIRE(cap_d >= 2 && (cap_d & (cap_d - 1)) == 0, "pcc_pcqm_features: table capacity cap_d must be a power of two");
    PCC_REQUIRE(tensor_stride >= 1, "pcc_pcqm_features: tensor_stride must be >= 1");
    PCC_REQUIRE(n_r >= 0 && n_r <= 0x7ffffffe, "pcc_pcqm_features: n_r must be 0 .. 2^31 - 2");
    PCC_REQUIRE(n_d >= 0 && n_d <= 0x7ffffffe, "pcc_pcqm_features: n_d must be 0 .. 2^31 - 2");
    PCC_REQUIRE(constants != nullptr, "pcc_pcqm_features: constants (k_L, k_kappa, c_chroma, c_hue) required");
    PCC_REQUIRE(stats || features || sums, "pcc_pcqm_features: one of the outputs stats, features, sums required");
    PCC_REQUIRE(!sums || scratch, "pcc_pcqm_features: sums needs scratch");
    PCC_REQUIRE(!sums || scratch_bytes >= pcc_pcqm_scratch_bytes(n_r), "pcc_pcqm_features: scratch too small for sums (pcc_pcqm_scratch_bytes)");
    hipStream_t st = as_stream(stream);
    if (n_r == 0) {
        if (sums) {
            hipLaunchKernelGGL(pcqm_pool_kernel, dim3(1), dim3(64), 0, st, (const double*)scratch, (int64_t)0, sums);
            PCC_LAUNCH_CHECK();
        }
        return PCC_OK;
    }
    PCC_REQUIRE(n_d >= 1, "pcc_pcqm_features: n_d must be >= 1 when n_r > 0 (every point needs a nearest neighbour)");
    PCC_REQUIRE(coords_r && keys_r && vals_r, "pcc_pcqm_features: coords_r, keys_r and vals_r required");
    PCC_REQUIRE(coords_d && keys_d && vals_d, "pcc_pcqm_features: coords_d, keys_d and vals_d required");
    PCC_REQUIRE(nn && attrs_r && attrs_d && w, "pcc_pcqm_features: nn, attrs_r, attrs_d and w required");
    PcqmArgs a;
    a.coords_r = coords_r; a.keys_r = keys_r; a.vals_r = vals_r; a.mask_r = (uint64_t)cap_r - 1;
    a.coords_d = coords_d; a.keys_d = keys_d; a.vals_d = vals_d; a.mask_d = (uint64_t)cap_d - 1;
    a.n_r = n_r; a.n_d = n_d; a.nn = nn; a.attrs_r = attrs_r; a.attrs_d = attrs_d; a.w = w;
    a.shift = grid_shift_of(tensor_stride); a.h = h;
    a.k_l = constants[0]; a.k_kappa = constants[1]; a.c_chroma = constants[2]; a.c_hue = constants[3];
    a.stats = stats; a.features = features; a.partials = sums ? (double*)scratch : nullptr;
    const int64_t blocks = pcqm_blocks(n_r);
    hipLaunchKernelGGL(pcqm_features_kernel, dim3((unsigned)blocks), dim3(PCQM_THREADS), 0, st, a);
    PCC_LAUNCH_CHECK();
    if (sums) {
        hipLaunchKernelGGL(pcqm_pool_kernel, dim3(1), dim3(64), 0, st, (const double*)scratch, blocks, sums);
        PCC_LAUNCH_CHECK();
    }
    return PCC_OK;
}

}  // extern "C"
