"""``pcqm_voxel``: a PCQM-style perceptual quality metric on a voxel grid (csrc/pcqm.hip).

The reference's sweep records PCQM as its headline quality axis (plot.py:17, evaluate.py:126) and gets it from an external binary
(utils.py:290-344: ``PCQM ... -fq -r 0.004 -knn 20 -rx 2.0``).  This module is a STAND-IN in the sense of the anchor codec and
D2: it follows PCQM's published structure (Meynet, Nehme, Digne, Lavoue: "PCQM: a full-reference quality metric for colored 3D
point clouds", QoMEX 2020) on an integer grid and does NOT reproduce the binary's numbers.  The result is called ``pcqm_voxel``,
never ``pcqm``: it must not be lined up against the ``pcqm`` column of the reference's results.  Three deviations:

1. colour space: plain CIELAB (sRGB -> linear -> XYZ D65 -> L*a*b*) instead of PCQM's LAB2000HL lookup table;
2. curvature: the surface variation l0 / (l0 + l1 + l2) of the radius-r ball (the eigenvalues of the exact integer moment matrix
   of ``estimate_normals``) instead of the mean curvature of a fitted quadric;
3. correspondence: a point of the source corresponds to its nearest voxel of the reconstruction (ties to the smallest (x, y, z),
   ``metrics.nearest_neighbours``) instead of its projection onto a fitted quadric.

Definition (float64 throughout).  R = source, D = reconstruction, duplicates dropped as ``PointCloudMetric`` drops them.  Every
row carries (L, c, a, b, kappa): CIELAB of the colour rounded to 8 bit, chroma c = sqrt(a^2 + b^2), and kappa of the radius-r
ball in its own cloud (0 where ``estimate_normals`` gives no normal).  For p in R with nearest D voxel p^: N_R(p) = {q in R: |q -
p|^2 <= h^2}, N_D(p^) likewise in D, centres included, a neighbour at squared distance d2 weighted exp(-d2 / (2 sigma^2)), sigma =
h / 3.  Weighted means mu_x / mu^_x of all five channels, weighted variances v_x / v^_x of L and kappa (clamped at 0) and the
cross terms s_x = sum_{q in N_R(p)} w (x_R(q) - mu_x)(x_D(q^) - mu^_x) / sum w, q^ the nearest D voxel of q, give

    f1 = |mu_L - mu^_L| / (max(mu_L, mu^_L) + k_L)              f2 = |sd_L - sd^_L| / (max(sd_L, sd^_L) + k_L)
    f3 = |S_L - s_L| / (S_L + k_L),  S_L = sqrt(v_L v^_L)        f4 = 1 - 1 / (c_chroma (mu_c - mu^_c)^2 + 1)
    f5 = 1 - 1 / (c_hue dH + 1),  dH = max(0, (mu_a - mu^_a)^2 + (mu_b - mu^_b)^2 - (mu_c - mu^_c)^2)
    f6, f7, f8 = f1, f2, f3 on kappa with k_kappa

(sd = sqrt(v); S = sd sd^ is taken as sqrt(v v^) so that identical clouds score exactly 0).  F_i = the mean of f_i over R and
``pcqm_voxel`` = sum_i weights_i F_i: 0 for identical clouds, larger is worse.

The default constants — k_L = k_kappa = 1, c_chroma = 0.002, c_hue = 0.1, weights (f3, f4, f6) = (0.0057, 0.9771, 0.0172) and 0
for the other features — are RECALLED from the PCQM release and the colour-image-difference measure it builds on; nothing in
this repository can check them.  They are keyword parameters for that reason.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import check, ptr
from .sparse import CoordMap

N_FEATURES = 8
N_STATS = 18
STAT_NAMES = ("sum_w_R", "sum_w_D", "mean_L_R", "mean_c_R", "mean_a_R", "mean_b_R", "mean_kappa_R", "mean_L_D", "mean_c_D", "mean_a_D",
              "mean_b_D", "mean_kappa_D", "var_L_R", "var_L_D", "cross_L", "var_kappa_R", "var_kappa_D", "cross_kappa")
# recalled from the PCQM release, not checkable here (module docstring)
DEFAULT_WEIGHTS = (0.0, 0.0, 0.0057, 0.9771, 0.0, 0.0172, 0.0, 0.0)
DEFAULT_K_L, DEFAULT_K_KAPPA, DEFAULT_C_CHROMA, DEFAULT_C_HUE = 1.0, 1.0, 0.002, 0.1

_RGB_TO_XYZ = ((0.4124564, 0.3575761, 0.1804375), (0.2126729, 0.7151522, 0.0721750), (0.0193339, 0.1191920, 0.9503041))


def lab_planes(rgb):
    """rgb float [N, 3] in [0, 1] -> float64 [N, 4]: (L, c, a, b) of the colour rounded to 8 bit (``metrics._round_to_8bit``):
    sRGB -> linear -> XYZ -> CIELAB against the white the matrix itself gives for (1, 1, 1), so white is (100, 0, 0, 0) and black
    (0, 0, 0, 0); L in [0, 100], c = sqrt(a^2 + b^2).  Elementwise torch code, on whatever device ``rgb`` is on."""
    from .metrics import _round_to_8bit
    c = _round_to_8bit(torch.as_tensor(rgb).to(torch.float64))
    lin = torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    f = []
    for row in _RGB_TO_XYZ:
        t = (row[0] * lin[:, 0] + row[1] * lin[:, 1] + row[2] * lin[:, 2]) / ((row[0] + row[1]) + row[2])
        f.append(torch.where(t > (6.0 / 29.0) ** 3, t.clamp_min(1e-300) ** (1.0 / 3.0), t / (3.0 * (6.0 / 29.0) ** 2) + 4.0 / 29.0))
    L, a, b = 116.0 * f[1] - 16.0, 500.0 * (f[0] - f[1]), 200.0 * (f[1] - f[2])
    return torch.stack([L, torch.sqrt(a * a + b * b), a, b], dim=1)


def surface_variation(coords, radius, coord_map=None):
    """kappa float64 [N] of the int32 [N, 4] coordinate tensor (batch, x, y, z) on the GPU: l0 / (l0 + l1 + l2) of the moment
    matrix of the radius-``radius`` ball (1 .. 8 voxels), 0 where ``estimate_normals`` gives no normal.  ``coord_map``: the
    CoordMap built on ``coords`` (built here when missing)."""
    if not (torch.is_tensor(coords) and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4 and coords.is_cuda):
        raise ValueError("surface_variation: coords is an int32 [N, 4] tensor (batch, x, y, z) on the GPU")
    coords = coords.contiguous()
    if coord_map is None:
        coord_map = CoordMap(coords, 1)
    elif coords.device != coord_map.device:
        raise ValueError("surface_variation: coordinates and coord_map are on different devices")
    n = int(coords.shape[0])
    kappa = torch.empty(n, dtype=torch.float64, device=coords.device)
    with torch.cuda.device(coords.device):
        keys, vals, cap = coord_map.table()
        check(_lib.lib().pcc_surface_variation(ptr(coords), n, ptr(keys), ptr(vals), cap, coord_map.stride, int(radius), ptr(kappa),
                                               _lib.stream()))
    return kappa


def default_radii(coords):
    """(radius, neighbourhood) the reference's call implies (-r 0.004, -rx 2.0): radius = clamp(round(0.004 * the largest side of
    the bounding box), 1, 4) voxels and neighbourhood = 2 radius.  coords: int [N, 4]"""
    if coords.shape[0] == 0:
        return 1, 2
    xyz = coords[:, 1:4]
    side = int((xyz.max(dim=0).values - xyz.min(dim=0).values).max())
    r = min(4, max(1, int(round(0.004 * side))))
    return r, 2 * r


def gaussian_weights(neighbourhood):
    """the weight table of pcc_pcqm_features: w[d2] = exp(-d2 / (2 sigma^2)), sigma = h / 3, for d2 = 0 .. h^2 (host floats)"""
    h = int(neighbourhood)
    sigma = h / 3.0
    return [math.exp(-d2 / (2.0 * sigma * sigma)) for d2 in range(h * h + 1)]


def pcqm_features(coords_r, map_r, attrs_r, coords_d, map_d, attrs_d, nn, neighbourhood, weight_table=None, k_L=DEFAULT_K_L,
                  k_kappa=DEFAULT_K_KAPPA, c_chroma=DEFAULT_C_CHROMA, c_hue=DEFAULT_C_HUE, want_stats=False, want_features=True):
    """The feature kernel on prepared inputs -> (stats [N_R, 18] or None, features [N_R, 8] or None, sums [8]), float64 on the
    GPU.  coords_* int32 [N, 4] with their CoordMaps, attrs_* float64 [N, 5] = (L, c, a, b, kappa), nn int32 [N_R] = the row of
    every R point's nearest D voxel, ``weight_table``: h^2 + 1 floats (default ``gaussian_weights``).  STAT_NAMES names the
    columns of ``stats``."""
    h = int(neighbourhood)
    dev = coords_r.device
    n_r, n_d = int(coords_r.shape[0]), int(coords_d.shape[0])
    in_range = 1 <= h <= 8                                   # out of range: the library refuses the call and names h
    table = [float(v) for v in weight_table] if weight_table is not None else (gaussian_weights(h) if in_range else [])
    if in_range and len(table) != h * h + 1:
        raise ValueError(f"pcqm_features: the weight table holds h^2 + 1 = {h * h + 1} values, got {len(table)}")
    if attrs_r.shape != (n_r, 5) or attrs_d.shape != (n_d, 5) or attrs_r.dtype != torch.float64 or attrs_d.dtype != torch.float64:
        raise ValueError("pcqm_features: attribute planes are float64 [N, 5]")
    if nn.shape != (n_r,) or nn.dtype != torch.int32:
        raise ValueError("pcqm_features: nn is int32 [N_R]")
    if map_r.stride != map_d.stride:
        raise ValueError("pcqm_features: the two clouds live on different tensor strides")
    coords_r, coords_d, attrs_r, attrs_d, nn = (t.contiguous() for t in (coords_r, coords_d, attrs_r, attrs_d, nn))
    L = _lib.lib()
    with torch.cuda.device(dev):
        w = torch.tensor(table if table else [1.0], dtype=torch.float64, device=dev)
        stats = torch.empty((n_r, N_STATS), dtype=torch.float64, device=dev) if want_stats else None
        features = torch.empty((n_r, N_FEATURES), dtype=torch.float64, device=dev) if want_features else None
        sums = torch.empty(N_FEATURES, dtype=torch.float64, device=dev)
        nbytes = int(L.pcc_pcqm_scratch_bytes(n_r))
        scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        constants = (ctypes.c_double * 4)(float(k_L), float(k_kappa), float(c_chroma), float(c_hue))
        keys_r, vals_r, cap_r = map_r.table()
        keys_d, vals_d, cap_d = map_d.table()
        check(L.pcc_pcqm_features(ptr(coords_r), n_r, ptr(keys_r), ptr(vals_r), cap_r, ptr(coords_d), n_d, ptr(keys_d), ptr(vals_d), cap_d,
                                  map_r.stride, ptr(nn), ptr(attrs_r), ptr(attrs_d), ptr(w), h, ctypes.addressof(constants), ptr(stats),
                                  ptr(features), ptr(sums), ptr(scratch), nbytes, _lib.stream()))
    return stats, features, sums


def _attribute_planes(coords, rgb, coord_map, radius):
    return torch.cat([lab_planes(rgb), surface_variation(coords, radius, coord_map).unsqueeze(1)], dim=1).contiguous()


def _score(sc, srgb, smap, rc, rrgb, rmap, nn, radius, neighbourhood, weights, k_L, k_kappa, c_chroma, c_hue, return_features):
    """the metric on de-duplicated clouds, their maps and the source -> reconstruction association"""
    if sc.shape[0] == 0 or rc.shape[0] == 0:
        raise ValueError("pcqm_voxel: empty cloud")
    radius = default_radii(sc)[0] if radius is None else int(radius)
    neighbourhood = min(8, 2 * radius) if neighbourhood is None else int(neighbourhood)
    weights = [float(v) for v in weights]
    if len(weights) != N_FEATURES:
        raise ValueError("pcqm_voxel: weights are 8 numbers, one per feature")
    attrs_r = _attribute_planes(sc, srgb, smap, radius)
    attrs_d = _attribute_planes(rc, rrgb, rmap, radius)
    _, features, sums = pcqm_features(sc, smap, attrs_r, rc, rmap, attrs_d, nn, neighbourhood, k_L=k_L, k_kappa=k_kappa,
                                      c_chroma=c_chroma, c_hue=c_hue, want_features=return_features)
    pooled = [s / sc.shape[0] for s in sums.tolist()]
    score = 0.0
    for wgt, F in zip(weights, pooled):
        if wgt != 0.0:
            score += wgt * F
    out = {"pcqm_voxel": score, "radius": radius, "neighbourhood": neighbourhood}
    out.update({"pcqm_f%d" % (i + 1): F for i, F in enumerate(pooled)})
    if return_features:
        out["features"] = features
    return out


def pcqm_voxel(source, reconstruction, radius=None, neighbourhood=None, *, weights=DEFAULT_WEIGHTS, k_L=DEFAULT_K_L,
               k_kappa=DEFAULT_K_KAPPA, c_chroma=DEFAULT_C_CHROMA, c_hue=DEFAULT_C_HUE, return_features=False, device="cuda:0"):
    """The voxel-grid PCQM stand-in of two ``[N, 6]`` clouds (x, y, z voxel indices, r, g, b in [0, 1]; tensors or arrays) ->
    {"pcqm_voxel": the score (0 = identical, larger = worse), "pcqm_f1" .. "pcqm_f8": the pooled features, "radius",
    "neighbourhood": the radii used} and, with ``return_features``, "features": float64 [N_source, 8] on the GPU.

    ``radius`` (curvature, 1 .. 8 voxels) defaults to clamp(round(0.004 * largest side of the source's bounding box), 1, 4),
    ``neighbourhood`` (statistics, 1 .. 8) to twice the radius (8 at most).  NOT the number the PCQM binary prints; the constants' defaults are
    recalled from the PCQM release and cannot be checked here (module docstring)."""
    from .metrics import _as_cloud, _drop_duplicated_points, nearest_neighbours
    sc, srgb = _drop_duplicated_points(*_as_cloud(source, device))
    rc, rrgb = _drop_duplicated_points(*_as_cloud(reconstruction, device))
    with torch.cuda.device(sc.device):
        smap, rmap = CoordMap(sc, 1, nbatch=1), CoordMap(rc, 1, nbatch=1)
        if sc.shape[0] == 0 or rc.shape[0] == 0:
            raise ValueError("pcqm_voxel: empty cloud")
        nn = nearest_neighbours(sc, rmap)[0]
    return _score(sc, srgb, smap, rc, rrgb, rmap, nn, radius, neighbourhood, weights, k_L, k_kappa, c_chroma, c_hue, return_features)
