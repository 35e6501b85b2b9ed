"""Quality-map builders (mirror of /root/reference/data/q_map.py:143-291, class ``Q_Map``).

A quality map is a sparse tensor on the frame's coordinates with two channels ``[q_g, q_a]`` in
[0, 1] (geometry, attribute; order fixed by utils.py:439).  ``Q_Map(config)(geometry)`` draws, per
batch item, either a linear gradient along a random axis or a uniform map with random levels — the
reference's training-time generator, driven by Python's ``random`` like the reference so that a
seeded run draws the same maps — and returns it together with the lambda map used by the losses.
``uniform_map`` / ``gradient_map`` / ``view_dependent_map`` / ``roi_map`` build the fixed maps of the
evaluation scripts (utils.py:436-445, evaluate_view_dep.py:207-260); ``facing_map`` is the second half of the view-dependent
experiment (evaluate_view_dep.py:354-376): quality by the angle between a point's normal and the viewing ray; ``visibility_map`` goes one step further and scores a point
by what the judged views can show at all (render.visibility: how far it lies behind the z-buffer front); ``distance_map`` scores
it by how large a camera at a position sees it (render.camera_visibility's depth); ``image_map`` scores it by an IMAGE in the
judged view (a box, a mask, a gaze point: ``box_image`` / ``gaze_image``) that render.sample_views carried back to the points.  Elementwise work
on [N, 2] tensors; plain torch.
"""
import math
import random

import torch

from .sparse import SparseTensor


def uniform_map(coords_map, q_g, q_a):
    n = coords_map.n
    f = torch.empty((n, 2), dtype=torch.float32, device=coords_map.device)
    f[:, 0] = float(q_g)
    f[:, 1] = float(q_a)
    return SparseTensor(f, coordinate_map=coords_map)


def gradient_map(coords_map, axis, lo=0.0, hi=1.0):
    """q rises linearly from ``lo`` to ``hi`` along coordinate axis 1..3 (both channels)."""
    c = coords_map.coords[:, axis].to(torch.float32)
    t = torch.clamp((c - c.min()) / (c.max() - c.min() + 1e-10), 0, 1)
    q = lo + (hi - lo) * t
    return SparseTensor(q.unsqueeze(1).repeat(1, 2).contiguous(), coordinate_map=coords_map)


def view_dependent_map(coords_map, q_g, q_a, axis, lo, hi):
    """evaluate_view_dep.py:207-215: quality falls off along a viewing axis — score = clip((p[axis] - lo) /
    (hi - lo), 0, 1), channels [q_g * score, q_a * score]"""
    c = coords_map.coords[:, axis].to(torch.float32)
    score = torch.clamp((c - float(lo)) / (float(hi) - float(lo)), 0, 1)
    return SparseTensor(torch.stack([float(q_g) * score, float(q_a) * score], dim=1).contiguous(), coordinate_map=coords_map)


def roi_map(coords_map, q_g, q_a, axis, plane):
    """evaluate_view_dep.py:254-260: region of interest — full quality where p[axis] >= plane, zero below"""
    score = (coords_map.coords[:, axis] >= plane).to(torch.float32)
    return SparseTensor(torch.stack([float(q_g) * score, float(q_a) * score], dim=1).contiguous(), coordinate_map=coords_map)


def facing_score(points, normals, camera=None, direction=None, floor=0.0):
    """float64 [N]: floor + (1 - floor) * |n . v| with v the unit vector from the point to ``camera`` or the fixed unit
    ``direction``; a point without a normal (zero) scores 1"""
    if (camera is None) == (direction is None):
        raise ValueError("facing map: give a camera position or a direction (one of them)")
    p, n = points.to(torch.float64), normals.to(torch.float64)
    v = torch.as_tensor(camera if camera is not None else direction, dtype=torch.float64, device=p.device).reshape(1, 3)
    if camera is not None:
        v = v - p
    v = v / torch.linalg.vector_norm(v, dim=1, keepdim=True).clamp_min(1e-300)
    score = float(floor) + (1.0 - float(floor)) * (n * v).sum(dim=1).abs()
    return torch.where((n != 0).any(dim=1), score, torch.ones_like(score))


def facing_map(coords_map, normals, q_g, q_a, camera=None, direction=None, floor=0.0):
    """quality by how squarely a surface faces the viewer: score = floor + (1 - floor) * |n . v| (facing_score), channels
    [q_g * score, q_a * score]; ``normals``: float64 [N, 3] of normals.estimate_normals on the map's coordinates"""
    score = facing_score(coords_map.coords[:, 1:4], normals, camera, direction, floor)
    return SparseTensor(torch.stack([float(q_g) * score, float(q_a) * score], dim=1).to(torch.float32).contiguous(), coordinate_map=coords_map)


def visibility_score(behind, tolerance=2, falloff=8, floor=0.0):
    """float64 [N]: floor + (1 - floor) * w from ``behind`` (integers: render.visibility's first result, voxels behind the
    z-buffer front).  With hidden = max(behind - tolerance, 0): w = 1 where hidden == 0; w = max(0, 1 - hidden / falloff) where
    hidden > 0 (0 when falloff == 0); w = 0 wherever behind == render.OFFSCREEN.  Float64 arithmetic on the integer input.

    ``tolerance`` keeps the few voxels just under the visible surface (they shape what the decoder puts on the front),
    ``falloff`` is the depth over which quality then runs out.  The defaults (2 and 8) are starting values read off a
    prototype on the synthetic shell, NOT tuned against rate or quality."""
    from .render import OFFSCREEN
    tolerance, falloff, floor = float(tolerance), float(falloff), float(floor)
    if not (tolerance >= 0 and falloff >= 0):
        raise ValueError("visibility score: tolerance and falloff are non-negative (got %r, %r)" % (tolerance, falloff))
    if not 0.0 <= floor <= 1.0:
        raise ValueError("visibility score: floor is in [0, 1] (got %r)" % floor)
    behind = torch.as_tensor(behind)
    if behind.is_floating_point() or behind.is_complex() or behind.dtype == torch.bool or behind.dim() != 1:
        raise ValueError("visibility score: behind is a one-dimensional integer tensor (render.visibility's first result)")
    b = behind.to(torch.int64)
    hidden = torch.clamp(b.to(torch.float64) - tolerance, min=0.0)
    if falloff > 0:
        w = torch.clamp(1.0 - hidden / falloff, min=0.0)
    else:
        w = (hidden == 0).to(torch.float64)
    w = torch.where(b == OFFSCREEN, torch.zeros_like(w), w)
    return floor + (1.0 - floor) * w


def visibility_map(coords_map, behind, q_g, q_a, tolerance=2, falloff=8, floor=0.0):
    """quality by what the judged views can show: score = visibility_score(behind, ...), channels [q_g * score, q_a * score]
    (float64 products, cast to float32 — as facing_map).  ``behind`` must be in the row order of ``coords_map.coords``: compute
    it on those rows, ``behind, _ = render.visibility(coords_map.coords[:, 1:4], views, H, W)``."""
    score = visibility_score(behind, tolerance, falloff, floor)
    if score.shape[0] != coords_map.n:
        raise ValueError("visibility map: %d scores for %d coordinates" % (score.shape[0], coords_map.n))
    score = score.to(coords_map.device)
    return SparseTensor(torch.stack([float(q_g) * score, float(q_a) * score], dim=1).to(torch.float32).contiguous(), coordinate_map=coords_map)


def distance_score(depth, focal, full=1.0, floor=0.0):
    """float64 [N]: clip((focal * 256 / depth) / full, floor, 1) from ``depth`` (integers: render.camera_visibility's third
    result, the distance along the viewing direction in 1/256 voxel) and the camera's ``focal`` in pixels.  focal * 256 / depth
    is the edge of the projected voxel in pixels: a voxel that covers ``full`` pixels or more gets full quality, a smaller one
    proportionally less, never below ``floor``.  0 wherever depth == render.OFFSCREEN (the camera does not draw the point).
    Float64 arithmetic on the integer input.

    The defaults (a full pixel, no floor) are starting values, NOT tuned against rate or quality."""
    from .render import OFFSCREEN
    focal, full, floor = float(focal), float(full), float(floor)
    if not (focal > 0 and math.isfinite(focal) and full > 0 and math.isfinite(full)):
        raise ValueError("distance score: focal and full are positive (got %r, %r)" % (focal, full))
    if not 0.0 <= floor <= 1.0:
        raise ValueError("distance score: floor is in [0, 1] (got %r)" % floor)
    depth = torch.as_tensor(depth)
    if depth.is_floating_point() or depth.is_complex() or depth.dtype == torch.bool or depth.dim() != 1:
        raise ValueError("distance score: depth is a one-dimensional integer tensor (render.camera_visibility's third result)")
    d = depth.to(torch.int64)
    if bool((d <= 0).any()):
        raise ValueError("distance score: depths are positive (a drawn point lies beyond the near plane)")
    score = torch.clamp(((focal * 256.0) / d.to(torch.float64)) / full, min=floor, max=1.0)
    return torch.where(d == OFFSCREEN, torch.zeros_like(score), score)


def distance_map(coords_map, depth, focal, q_g, q_a, full=1.0, floor=0.0):
    """quality by how large the camera sees a voxel: score = distance_score(depth, focal, ...), channels [q_g * score,
    q_a * score] (float64 products, cast to float32 — as visibility_map).  ``depth`` must be in the row order of
    ``coords_map.coords``: ``_, _, depth = render.camera_visibility(coords_map.coords[:, 1:4], [camera])``, ``focal`` is
    ``camera.focal``."""
    score = distance_score(depth, focal, full, floor)
    if score.shape[0] != coords_map.n:
        raise ValueError("distance map: %d scores for %d coordinates" % (score.shape[0], coords_map.n))
    score = score.to(coords_map.device)
    return SparseTensor(torch.stack([float(q_g) * score, float(q_a) * score], dim=1).to(torch.float32).contiguous(), coordinate_map=coords_map)


def image_score(total, count, peak, reduce="max", channel=0, scale=255, floor=0.0):
    """float64 [N]: floor + (1 - floor) * clip(v / scale, 0, 1) from what render.sample_views / sample_cameras bring back from an
    image (``total`` int64 [N, C], ``count`` int32 [N], ``peak`` int32 [N, C]): v = peak[:, channel] for ``reduce="max"`` (the
    brightest pixel that looks at the point), total[:, channel] / count for ``reduce="mean"``.  A point no pixel counted for
    (count == 0) scores ``floor``.  ``scale`` is the image value that means full quality (255 for a byte image).  Float64
    arithmetic on the integer inputs."""
    if reduce not in ("max", "mean"):
        raise ValueError("image score: reduce is 'max' or 'mean' (got %r)" % (reduce,))
    scale, floor = float(scale), float(floor)
    if not (scale > 0 and math.isfinite(scale)):
        raise ValueError("image score: scale is positive (got %r)" % scale)
    if not 0.0 <= floor <= 1.0:
        raise ValueError("image score: floor is in [0, 1] (got %r)" % floor)
    total, count, peak = torch.as_tensor(total), torch.as_tensor(count), torch.as_tensor(peak)
    if any(t.is_floating_point() or t.is_complex() or t.dtype == torch.bool for t in (total, count, peak)):
        raise ValueError("image score: total, count and peak are integer tensors (render.sample_views' results)")
    if count.dim() != 1 or total.dim() != 2 or peak.shape != total.shape or total.shape[0] != count.shape[0]:
        raise ValueError("image score: total and peak are [N, C], count is [N]")
    if not 0 <= int(channel) < total.shape[1]:
        raise ValueError("image score: channel %r of %d" % (channel, total.shape[1]))
    seen = count > 0
    if reduce == "max":
        v = peak[:, int(channel)].to(torch.float64)
    else:
        v = total[:, int(channel)].to(torch.float64) / count.clamp_min(1).to(torch.float64)
    # a tensor divisor: dividing a GPU tensor by a Python number multiplies by its reciprocal, which is not the rounded quotient
    w = torch.clamp(v / torch.full_like(v, scale), min=0.0, max=1.0)
    w = torch.where(seen, w, torch.zeros_like(w))
    return floor + (1.0 - floor) * w


def image_map(coords_map, total, count, peak, q_g, q_a, reduce="max", channel=0, scale=255, floor=0.0):
    """a screen-space quality map: score = image_score(total, count, peak, ...), channels [q_g * score, q_a * score] (float64
    products, cast to float32 — as visibility_map).  The three tensors must be in the row order of ``coords_map.coords``:
    ``total, count, peak = render.sample_views(coords_map.coords[:, 1:4], views, images, H, W, tolerance=2)``."""
    score = image_score(total, count, peak, reduce, channel, scale, floor)
    if score.shape[0] != coords_map.n:
        raise ValueError("image map: %d scores for %d coordinates" % (score.shape[0], coords_map.n))
    score = score.to(coords_map.device)
    return SparseTensor(torch.stack([float(q_g) * score, float(q_a) * score], dim=1).to(torch.float32).contiguous(), coordinate_map=coords_map)


def _image_shape(H, W):
    if not (int(H) == H and int(W) == W and int(H) >= 1 and int(W) >= 1):
        raise ValueError("an image is H x W pixels, both at least 1 (got %r x %r)" % (H, W))
    return int(H), int(W)


def box_image(H, W, box):
    """uint8 [H, W] numpy array: 255 in rows r0 .. r1 - 1 and columns c0 .. c1 - 1 of ``box = (r0, r1, c0, c1)`` (clipped to the
    image), 0 elsewhere — a detector's box as an image for render.sample_views"""
    import numpy as np
    H, W = _image_shape(H, W)
    r0, r1, c0, c1 = (int(v) for v in box)
    img = np.zeros((H, W), dtype=np.uint8)
    img[max(r0, 0):max(r1, 0), max(c0, 0):max(c1, 0)] = 255
    return img


def gaze_image(H, W, gaze, radius, falloff):
    """uint8 [H, W] numpy array: 255 within ``radius`` pixels of the gaze point ``gaze = (row, col)``, running linearly to 0 over
    ``falloff`` further pixels: rint(255 * clip(1 - (dist - radius) / falloff, 0, 1)) in float64, dist the Euclidean distance of
    the pixel's (row, col) from the gaze point; with falloff == 0 a hard disc"""
    import numpy as np
    H, W = _image_shape(H, W)
    row, col = (float(v) for v in gaze)
    radius, falloff = float(radius), float(falloff)
    if not (radius >= 0 and falloff >= 0 and math.isfinite(radius) and math.isfinite(falloff)):
        raise ValueError("gaze image: radius and falloff are non-negative (got %r, %r)" % (radius, falloff))
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dist = np.sqrt((rr - row) * (rr - row) + (cc - col) * (cc - col))
    if falloff > 0:
        w = np.clip(1.0 - (dist - radius) / falloff, 0.0, 1.0)
    else:
        w = (dist <= radius).astype(np.float64)
    return np.rint(255.0 * w).astype(np.uint8)


class Q_Map:
    def __init__(self, config):
        self.mode = config["mode"]
        if self.mode == "exponential":
            self.a_A = math.log2(config["lambda_A_max"] + config["lambda_A_min"])
            self.b_A = config["lambda_A_min"] - 1
            self.a_G = math.log2(config["lambda_G_max"] + config["lambda_G_min"])
            self.b_G = config["lambda_G_min"] - 1
        elif self.mode == "quadratic":
            self.a_A = config["lambda_A_max"] - config["lambda_A_min"]
            self.b_A = config["lambda_A_min"]
            self.a_G = config["lambda_G_max"] - config["lambda_G_min"]
            self.b_G = config["lambda_G_min"]
        else:
            raise ValueError("Unknown Q_map mode")

    def __call__(self, geometry):
        """geometry: SparseTensor -> (q_map, lambda_map), both on geometry's coordinate map"""
        coords = geometry.C
        feats = torch.zeros((coords.shape[0], 2), dtype=torch.float32, device=coords.device)
        for b in torch.unique(coords[:, 0]).tolist():
            mask = coords[:, 0] == b
            feats[mask] = self.random_q_map(coords[mask])
        q_map = SparseTensor(feats, coordinate_map=geometry.map)
        return q_map, self.scale_q_map(q_map)

    def scale_q_map(self, q_map):
        f = q_map.F.clone()
        if self.mode == "exponential":
            f[:, 0] = 2 ** (f[:, 0] * self.a_G) + self.b_G
            f[:, 1] = 2 ** (f[:, 1] * self.a_A) + self.b_A
        else:
            f[:, 0] = f[:, 0] ** 2 * self.a_G + self.b_G
            f[:, 1] = f[:, 1] ** 2 * self.a_A + self.b_A
        return SparseTensor(f, coordinate_map=q_map.map)

    def random_q_map(self, coordinates):
        return self.gradient(coordinates) if random.choice(range(2)) == 0 else self.uniform(coordinates)

    @staticmethod
    def gradient(coordinates):
        direction = random.randint(1, 3)
        c = coordinates[:, direction].to(torch.float32)
        q = torch.clamp((c - c.min()) / (c.max() - c.min() + 1e-10), 0, 1)
        return q.unsqueeze(1).repeat(1, 2)

    @staticmethod
    def uniform(coordinates):
        scale_geometry = random.uniform(0, 1)
        scale_attribute = random.uniform(0, 1)
        q = torch.ones((coordinates.shape[0], 2), dtype=torch.float32, device=coordinates.device)
        q[:, 0] *= scale_geometry
        q[:, 1] *= scale_attribute
        return q
