"""View rendering and view PSNR / SSIM: the evaluation half of the view-dependent and region-of-interest experiment
(the reference's evaluate_view_dep.py:102-305: ``render_pointviews``, then ``rgb2yuv``, ``peak_signal_noise_ratio`` and
``structural_similarity`` on the rendered images).

The reference renders through open3d's OpenGL window (evaluate_view_dep.py:308-348), which needs a display and is not
reproducible pixel for pixel.  Every view it uses is a signed coordinate axis (evaluate_view_dep.py:46-57), so the
renderer here is an exact integer projection of a voxelised cloud — an orthographic z-buffer splat (csrc/render.hip,
``pcc_render_view``) — the same move metrics.py makes for the KD-tree:

    u = right . p,  v = up . p,  d = front . p          (front points from the object to the camera: open3d's set_front)
    a point covers columns (u - u_min) * scale + ox + i and rows (v_max - v) * scale + oy + j,  i, j in [0, point_size)

A pixel shows the point with the largest d; among equal d the lowest row wins, and rows are put in canonical (x, y, z)
order before the call, so for a duplicate-free cloud the tie goes to the smaller (x, y, z) whatever the input order.
What differs from open3d: no perspective (the reference narrows the field of view to its minimum, :340, which is close to
orthographic), square integer splats instead of round anti-aliased GL points, an integer ``scale`` in place of ``zoom``.

``visibility`` is the way back from such an image to the points (``pcc_view_visibility``): per point, how many voxels it lies
behind the z-buffer front of the given views and how many pixels show it — what q_map.visibility_map builds its quality map from.

``Camera``, ``render_camera`` and ``camera_visibility`` are the same two operators for a viewer who stands at a point: a pinhole
camera quantised to integers on the host, a perspective projection in int64 on the device (``pcc_render_camera``,
``pcc_camera_visibility``), and per point also its depth, which q_map.distance_map turns into a quality map.

``view_buffers`` / ``camera_buffers`` return the z-buffer itself (the row and the depth every pixel shows), and ``sample_views``
/ ``sample_cameras`` carry an IMAGE back to the points (``pcc_view_sample``, ``pcc_camera_sample``): per point the sum, the
number and the maximum of an integer image over the pixels that look at it — what q_map.image_map builds a screen-space
quality map from (a detector's box, a painted mask, a gaze point).

``view_metrics`` restates scikit-image's formulas in float64 (``pcc_image_compare``).  scikit-image is no dependency of
this project and was not at hand: the ``yuv_from_rgb`` coefficients, the SSIM constants (K1 = 0.01, K2 = 0.03, 7 x 7
uniform window, sample covariance, crop of 3) and the data-range rule of ``peak_signal_noise_ratio`` are recalled from its
source, not pinned against it.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

# named views as data, (front, up): evaluate_view_dep.py:49-50 (the 8iVFB bodies) and :54-55 (MVUB)
VIEWS = {"front": ((0, 0, 1), (0, 1, 0)), "side": ((-1, 0, 0), (0, 1, 0))}
VIEWS_MVUB = {"front": ((0, -1, 0), (0, 0, 1)), "side": ((-1, 0, 0), (0, 0, 1))}

COORD_LIMIT = _lib.PCC.COORD_LIMIT
OFFSCREEN = _lib.PCC.VIS_OFFSCREEN             # ``visibility``'s ``behind`` of a point no pixel of whose splat is inside the image
SAMPLE_OWN = _lib.PCC.SAMPLE_OWN               # ``sample_views``' tolerance that means "the pixels that show the point"
SAMPLE_NONE = _lib.PCC.SAMPLE_NONE             # ``peak`` of a point no pixel counted for
SAMPLE_MAX_CHANNELS = _lib.PCC.SAMPLE_MAX_CHANNELS
MAX_DIM = 8192                                 # the largest image side the renderer takes (csrc/render.hip, RENDER_MAX_DIM)


def _axis(v, name):
    try:
        a = [int(x) for x in v]
        exact = len(a) == 3 and all(float(x) == float(y) for x, y in zip(a, v))
    except (TypeError, ValueError):
        exact = False
    if not exact or sorted(abs(x) for x in a) != [0, 0, 1]:
        raise ValueError("%s must be a signed unit coordinate axis such as (0, 0, 1) or (-1, 0, 0), got %r" % (name, v))
    return tuple(a)


def view_axes(front, up):
    """-> (right, up, front) as integer triples, right = up x front.  ValueError unless front and up are orthogonal signed
    coordinate axes."""
    f, u = _axis(front, "front"), _axis(up, "up")
    if sum(a * b for a, b in zip(f, u)) != 0:
        raise ValueError("front %r and up %r are not orthogonal" % (front, up))
    r = (u[1] * f[2] - u[2] * f[1], u[2] * f[0] - u[0] * f[2], u[0] * f[1] - u[1] * f[0])
    return r, u, f


def _view(view):
    """a preset name or a (front, up) pair -> (front, up)"""
    if isinstance(view, str):
        if view not in VIEWS:
            raise ValueError("unknown view %r: one of %s or a (front, up) pair" % (view, sorted(VIEWS)))
        return VIEWS[view]
    front, up = view
    return front, up


def _int_xyz(cloud):
    """[N, >= 3] tensor or array -> its xyz columns as an int32 tensor (on the cloud's device); ValueError unless integers"""
    if not torch.is_tensor(cloud):
        cloud = torch.as_tensor(np.asarray(cloud))
    if cloud.dim() != 2 or cloud.shape[1] < 3:
        raise ValueError("a cloud is a [N, 6] array: x, y, z, r, g, b")
    xyz = cloud[:, :3]
    ixyz = torch.round(xyz.double()).to(torch.int32)
    if not torch.equal(ixyz.to(xyz.dtype), xyz):
        raise ValueError("views are rendered from voxelised clouds: coordinates must be integers")
    return cloud, ixyz


def view_frame(cloud, front, up, H, W, scale=None):
    """The framing (u_min, u_max, v_min, v_max, scale, ox, oy) that centres ``cloud``'s bounding box in an H x W image:
    ox = (W - (u_max - u_min + 1) * scale) // 2, oy likewise with v and H.  ``scale=None`` picks the largest integer scale at
    which the box fits, at least 1.  An empty cloud is framed like the single voxel (0, 0, 0)."""
    r, u, _ = view_axes(front, up)
    _, xyz = _int_xyz(cloud)
    if xyz.shape[0] == 0:
        u_min = u_max = v_min = v_max = 0
    else:
        lo, hi = xyz.amin(dim=0).tolist(), xyz.amax(dim=0).tolist()

        def span(axis):                       # a signed unit axis picks one coordinate, possibly negated
            k = [abs(a) for a in axis].index(1)
            return (lo[k], hi[k]) if axis[k] > 0 else (-hi[k], -lo[k])

        (u_min, u_max), (v_min, v_max) = span(r), span(u)
    wu, wv = u_max - u_min + 1, v_max - v_min + 1
    if scale is None:
        scale = max(1, min(int(W) // wu, int(H) // wv))
    scale = int(scale)
    return u_min, u_max, v_min, v_max, scale, (int(W) - wu * scale) // 2, (int(H) - wv * scale) // 2


def colours_to_bytes(rgb):
    """clamp(rint(float32(c) * 255), 0, 255) as uint8"""
    return torch.clamp(torch.round(rgb.to(torch.float32) * 255.0), 0.0, 255.0).to(torch.uint8)


def _cloud(who, cloud, device, colours=False):
    """What every operator ``who`` checks first -> (cloud, xyz, n, dev): the cloud as a tensor, its integer xyz columns, its row
    count and the GPU the call runs on (``device``, else the cloud's, else cuda:0)"""
    cloud, xyz = _int_xyz(cloud)
    if colours and cloud.shape[1] < 6:
        raise ValueError("a cloud is a [N, 6] array: x, y, z, r, g, b")
    dev = torch.device(device) if device is not None else (cloud.device if cloud.is_cuda else torch.device("cuda:0"))
    if dev.type != "cuda":
        raise ValueError("%s runs on the GPU: got device %s" % (who, dev))
    n = int(cloud.shape[0])
    if n and int(xyz.abs().max()) > COORD_LIMIT:
        raise ValueError("%s: coordinates beyond +-%d" % (who, COORD_LIMIT))
    return cloud, xyz, n, dev


def _background(background):
    bg = np.asarray(background)
    if bg.shape != (3,) or bg.min() < 0 or bg.max() > 255:
        raise ValueError("background is three bytes")
    return bg.astype(np.uint8)


def _sorted_rows(L, cloud, xyz, dev, colours):
    """-> (coords, rgb8, perm): the (batch 0, x, y, z) int32 rows on ``dev`` in canonical (x, y, z) order — the tie rule's
    "lowest row" —, the colours of ``cloud`` as bytes in that order (None unless ``colours``) and the permutation that put them
    there (None for fewer than two rows)"""
    n = int(xyz.shape[0])
    coords = torch.cat([torch.zeros((n, 1), dtype=torch.int32, device=dev), xyz.to(dev)], dim=1).contiguous()
    rgb8 = colours_to_bytes(cloud[:, 3:6].to(dev)).contiguous() if colours else None
    if n < 2:
        return coords, rgb8, None
    nbytes = L.pcc_sort_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    check(L.pcc_sort_coords(ptr(coords), n, ptr(perm), ptr(scratch), nbytes, _lib.stream()))
    perm = perm.long()
    return coords[perm].contiguous(), rgb8[perm].contiguous() if colours else None, perm


def _zbuffer(L, dev, sizes):
    """-> (zbuf, zbytes): one z-buffer on ``dev`` large enough for every (H, W) of ``sizes`` (0 bytes for a size the entries refuse)"""
    zbytes = max(L.pcc_render_scratch_bytes(H, W) for H, W in sizes)
    return torch.empty(max(zbytes, 8), dtype=torch.uint8, device=dev), zbytes


def _input_order(perm, *outs):
    """per-row outputs of canonically sorted rows -> the same in the input's row order"""
    return outs if perm is None else tuple(torch.empty_like(t).index_copy_(0, perm, t) for t in outs)


def render_view(cloud, front, up, H, W, frame=None, point_size=None, background=(255, 255, 255), device=None):
    """Render ``cloud`` ([N, 6]: integer x, y, z and r, g, b in [0, 1]; one batch item) from the signed axis ``front`` with
    ``up`` upwards -> uint8 [H, W, 3] tensor on the cloud's device (``device`` for an array; a GPU: there is no CPU renderer).

    ``frame``: a ``view_frame`` result (of this or of another cloud — reconstructions are rendered in their source's
    frame); None frames the cloud itself.  ``point_size=None`` means the frame's scale: adjacent voxels tile the image
    without gaps or overlap."""
    r, u, f = view_axes(front, up)
    cloud, xyz, n, dev = _cloud("render_view", cloud, device, colours=True)
    if frame is None:
        frame = view_frame(xyz, f, u, H, W)
    u_min, _, _, v_max, scale, ox, oy = (int(v) for v in frame)
    point_size = scale if point_size is None else int(point_size)
    bg = _background(background)
    H, W = int(H), int(W)
    L = _lib.lib()
    with torch.cuda.device(dev):
        coords, rgb8, _ = _sorted_rows(L, cloud, xyz, dev, colours=True)
        zbuf, zbytes = _zbuffer(L, dev, [(H, W)])
        image = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if zbytes else None
        axes = [np.asarray(a, dtype=np.int32) for a in (r, u, f)]
        check(L.pcc_render_view(ptr(coords) if n else None, ptr(rgb8) if n else None, n, ptr(axes[0]), ptr(axes[1]), ptr(axes[2]),
                                u_min, v_max, ox, oy, scale, point_size, H, W, ptr(bg), ptr(zbuf), zbytes, ptr(image), _lib.stream()))
    return image


def _views(views):
    """a non-empty list of preset names / (front, up) pairs -> [(right, up, front), ...]; ValueError otherwise"""
    if isinstance(views, str) or not isinstance(views, (list, tuple)):
        raise ValueError("views is a list of preset names of %s or (front, up) pairs, got %r" % (sorted(VIEWS), views))
    if len(views) == 0:
        raise ValueError("views is empty: visibility needs at least one view")
    out = []
    for view in views:
        try:
            front, up = _view(view)
        except TypeError:
            raise ValueError("a view is a preset name of %s or a (front, up) pair, got %r" % (sorted(VIEWS), view)) from None
        out.append(view_axes(front, up))
    return out


def visibility(cloud, views, H, W, frames=None, point_size=None, device=None):
    """Which points do the images of ``views`` show?  -> (behind, won): int32 [N] tensors on the GPU in the INPUT's row order
    (csrc/render.hip, ``pcc_view_visibility``).

    For one view, with the geometry, clipping and winner rule of ``render_view`` at H x W: ``behind[i]`` is the minimum, over
    the pixels of point i's splat that lie inside the image, of (the largest d splatted onto the pixel) - d_i: 0 exactly when
    the point is on the z-buffer front in at least one pixel, otherwise how many voxels deep it lies behind what the view
    shows; ``OFFSCREEN`` when no pixel of its splat is inside the image.  ``won[i]`` is the number of pixels that show point i
    (rows are put in canonical (x, y, z) order before the call, as in ``render_view``, so ties between equal depths go to the
    smaller (x, y, z) whatever the input order; ``behind`` does not depend on ties).  Over several views ``behind`` is the
    minimum and ``won`` the sum.  All integer and bitwise reproducible.

    ``cloud``: [N, >= 3] with integer coordinates (colours are not needed).  ``views``: a non-empty list of preset names of
    ``VIEWS`` or (front, up) pairs.  ``frames``: None (every view frames the cloud itself at H x W) or one ``view_frame`` result
    per view (a reconstruction is analysed in its source's frames).  ``point_size=None`` means each frame's scale.  Not a
    camera: orthographic, axis views only, square splats."""
    axes = _views(views)
    if frames is not None:
        if not isinstance(frames, (list, tuple)) or len(frames) != len(axes):
            raise ValueError("frames is None or one view_frame result per view (%d views)" % len(axes))
        if any(not isinstance(fr, (list, tuple)) or len(fr) != 7 for fr in frames):
            raise ValueError("a frame is a view_frame result: (u_min, u_max, v_min, v_max, scale, ox, oy)")
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError("H and W must be 1 .. %d (got %d x %d)" % (MAX_DIM, H, W))
    cloud, xyz, n, dev = _cloud("visibility", cloud, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        behind, won = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        if n == 0:                                     # nothing to frame and nothing to ask
            return behind, won
        xyz = xyz.to(dev)
        coords, _, perm = _sorted_rows(L, cloud, xyz, dev, colours=False)
        zbuf, zbytes = _zbuffer(L, dev, [(H, W)])
        for k, (r, u, f) in enumerate(axes):
            frame = view_frame(xyz, f, u, H, W) if frames is None else frames[k]
            u_min, _, _, v_max, scale, ox, oy = (int(v) for v in frame)
            size = scale if point_size is None else int(point_size)
            vecs = [np.asarray(a, dtype=np.int32) for a in (r, u, f)]
            check(L.pcc_view_visibility(ptr(coords), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, size, H, W,
                                        ptr(zbuf), zbytes, int(k > 0), ptr(behind), ptr(won), _lib.stream()))
        return _input_order(perm, behind, won)


CameraInts = collections.namedtuple("CameraInts", "pos_q axes_q focal_q near_q H W")
POS_Q_MAX, AXIS_ONE, FOCAL_Q_MAX = 1 << 24, 1 << 14, 1 << 20            # the limits of include/pcc_hip.h's camera table


def _vec3(v, name):
    a = np.asarray(v, dtype=np.float64)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError("%s must be three finite numbers, got %r" % (name, v))
    return a


def _unit(a, name):
    length = float(np.sqrt((a * a).sum()))
    if not length > 0.0:
        raise ValueError("%s has no direction (zero length)" % name)
    return a / length


class Camera:
    """A pinhole camera at a position, built in float64 and then QUANTISED: only the integers of ``quantised()`` reach the
    library (include/pcc_hip.h, ``pcc_render_camera``), so two cameras with equal integers render equal bytes.

    ``front`` points from the scene to the camera (the convention of ``view_axes`` and open3d's ``set_front``); with ``look_at``
    it is normalise(position - look_at).  right = normalise(up x front), up' = front x right.  ``focal`` is in pixels; with
    ``fov_y`` (degrees, the full vertical angle) focal = (H / 2) / tan(fov_y / 2).  Exactly one of ``look_at`` / ``front`` and
    exactly one of ``fov_y`` / ``focal``; ``near`` is the distance of the near plane in voxels.  The principal point is the
    image centre (W / 2, H / 2).

    Quantisation: pos_q = rint(16 position) (1/16 voxel, |position| <= 2^20), axes_q = rint(2^14 [right; up'; front]) (an
    axis-aligned camera is exact), focal_q = rint(16 focal) in 1 .. 2^20, near_q = rint(16 near) >= 1, H and W in 1 .. 8192.
    ValueError for anything outside, and for an ``up`` parallel to ``front``."""

    def __init__(self, position, look_at=None, front=None, up=(0, 1, 0), fov_y=None, focal=None, H=None, W=None, near=1.0):
        if (look_at is None) == (front is None):
            raise ValueError("camera: give look_at or front (exactly one of them)")
        if (fov_y is None) == (focal is None):
            raise ValueError("camera: give fov_y or focal (exactly one of them)")
        if H is None or W is None:
            raise ValueError("camera: the image size H, W is required")
        H, W = _image_size(H, W)
        position = _vec3(position, "position")
        f = _unit(position - _vec3(look_at, "look_at") if look_at is not None else _vec3(front, "front"), "front")
        right = np.cross(_unit(_vec3(up, "up"), "up"), f)
        if not float(np.sqrt((right * right).sum())) > 1e-9:
            raise ValueError("camera: up %r is parallel to front %r" % (up, tuple(f.tolist())))
        right = _unit(right, "up x front")
        up2 = np.cross(f, right)
        if fov_y is not None:
            fov_y = float(fov_y)
            if not 0.0 < fov_y < 180.0:
                raise ValueError("camera: fov_y is an angle in (0, 180) degrees, got %r" % fov_y)
            focal = (H / 2.0) / math.tan(math.radians(fov_y) / 2.0)
        focal, near = float(focal), float(near)
        if not (math.isfinite(focal) and math.isfinite(near)):
            raise ValueError("camera: focal and near must be finite")
        axes = np.stack([right, up2, f])
        self._set(position, axes, focal, near, H, W,
                  np.rint(16.0 * position), np.rint(float(AXIS_ONE) * axes), np.rint(16.0 * focal), np.rint(16.0 * near))

    def _set(self, position, axes, focal, near, H, W, pos_q, axes_q, focal_q, near_q):
        pos_q = tuple(int(v) for v in np.asarray(pos_q).reshape(3))
        axes_q = tuple(tuple(int(v) for v in row) for row in np.asarray(axes_q).reshape(3, 3))
        focal_q, near_q = int(focal_q), int(near_q)
        if max(abs(v) for v in pos_q) > POS_Q_MAX:
            raise ValueError("camera: position beyond +-2^20 voxels")
        if max(abs(v) for row in axes_q for v in row) > AXIS_ONE:
            raise ValueError("camera: an axis entry beyond +-2^14")
        if not 1 <= focal_q <= FOCAL_Q_MAX:
            raise ValueError("camera: focal must quantise to 1 .. 2^20 sixteenths of a pixel (got %d)" % focal_q)
        if not 1 <= near_q <= 0x7FFFFFFF:
            raise ValueError("camera: near must quantise to at least one sixteenth of a voxel (got %d)" % near_q)
        self.position, self.focal, self.near, self.H, self.W = np.asarray(position, dtype=np.float64), float(focal), float(near), H, W
        self.right, self.up, self.front = (np.asarray(a, dtype=np.float64) for a in axes)
        self._ints = CameraInts(pos_q, axes_q, focal_q, near_q, H, W)

    def quantised(self):
        """-> CameraInts(pos_q (3 ints), axes_q (3 x 3 ints: right, up', front), focal_q, near_q, H, W)"""
        return self._ints

    @classmethod
    def from_quantised(cls, pos_q, axes_q, focal_q, near_q, H, W):
        """the camera with exactly these integers (``Camera.from_quantised(*camera.quantised())`` is ``camera`` again)"""
        H, W = _image_size(H, W)
        try:
            p, a = np.asarray(pos_q), np.asarray(axes_q)
            exact = (p.shape == (3,) and a.shape == (3, 3) and all(int(v) == v for v in p.tolist() + a.reshape(-1).tolist())
                     and int(focal_q) == focal_q and int(near_q) == near_q)
        except (TypeError, ValueError):
            exact = False
        if not exact:
            raise ValueError("camera: from_quantised takes integers: pos_q[3], axes_q[3][3], focal_q, near_q, H, W")
        self = cls.__new__(cls)
        self._set(p.astype(np.float64) / 16.0, a.astype(np.float64) / float(AXIS_ONE), focal_q / 16.0, near_q / 16.0, H, W, p, a,
                  focal_q, near_q)
        return self

    def __repr__(self):
        return "Camera.from_quantised(%r, %r, %d, %d, %d, %d)" % tuple(self._ints)


def _image_size(H, W):
    try:
        h, w = int(H), int(W)
        ok = h == H and w == W and 1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("H and W must be integers in 1 .. %d (got %r x %r)" % (MAX_DIM, H, W))
    return h, w


def _ps_q(point_size):
    """rint(16 point_size) for point_size in (0, 16]: the voxel's edge in 1/16 voxel, 1 .. 256"""
    try:
        ps = float(point_size)
    except (TypeError, ValueError):
        ps = float("nan")
    q = int(np.rint(16.0 * ps)) if math.isfinite(ps) else 0
    if not (0.0 < ps <= 16.0 and 1 <= q <= 256):
        raise ValueError("point_size is a voxel edge in (0, 16] voxels (got %r)" % (point_size,))
    return q


def _camera_args(camera):
    q = camera.quantised()
    return np.asarray(q.pos_q, dtype=np.int32), np.asarray(q.axes_q, dtype=np.int32).reshape(9), q


def render_camera(cloud, camera, point_size=1.0, background=(255, 255, 255), device=None):
    """Render ``cloud`` ([N, 6]: integer x, y, z and r, g, b in [0, 1]) as ``camera`` (a ``Camera``) sees it -> uint8 [H, W, 3]
    tensor on the cloud's device (``device`` for an array; a GPU), H and W the camera's (``pcc_render_camera``).

    Perspective, in integers (include/pcc_hip.h states the projection): a voxel is a square splat of its projected edge
    ``focal * point_size / depth`` pixels, rounded up and clamped to 1 .. 16, centred on its projection; points nearer than
    ``camera.near`` (or behind the camera) are not drawn.  A pixel shows the point with the smallest depth key (1/256 voxel);
    among equal keys the lowest row wins, and rows are put in canonical (x, y, z) order first, so the image does not depend on
    the input's row order.  ``point_size`` is the voxel's edge in voxels, in (0, 16].  Not a lens: square splats, no
    anti-aliasing, and holes open between voxels once one projects beyond 16 pixels."""
    if not isinstance(camera, Camera):
        raise ValueError("render_camera: camera is a render.Camera, got %r" % (camera,))
    ps_q = _ps_q(point_size)
    cloud, xyz, n, dev = _cloud("render_camera", cloud, device, colours=True)
    bg = _background(background)
    pos, axes, q = _camera_args(camera)
    L = _lib.lib()
    with torch.cuda.device(dev):
        coords, rgb8, _ = _sorted_rows(L, cloud, xyz, dev, colours=True)
        zbuf, zbytes = _zbuffer(L, dev, [(q.H, q.W)])
        image = torch.empty((q.H, q.W, 3), dtype=torch.uint8, device=dev)
        check(L.pcc_render_camera(ptr(coords) if n else None, ptr(rgb8) if n else None, n, ptr(pos), ptr(axes), q.focal_q, q.near_q,
                                  q.H, q.W, ps_q, ptr(bg), ptr(zbuf), zbytes, ptr(image), _lib.stream()))
    return image


def camera_visibility(cloud, cameras, point_size=1.0, device=None):
    """Which points do ``cameras`` (a non-empty list of ``Camera``) show?  -> (behind, won, depth): int32 [N] tensors on the GPU
    in the INPUT's row order (``pcc_camera_visibility``).

    For one camera, with the projection, clipping and winner rule of ``render_camera``: ``behind[i]`` is the minimum over the
    pixels of point i's splat inside the image of (its depth key - the pixel's front depth key) >> 8: whole voxels behind what
    the camera sees, 0 within one voxel of the front; ``won[i]`` the number of pixels that show point i; ``depth[i]`` its depth
    key, the distance along the viewing direction in 1/256 voxel (what q_map.distance_score reads).  A point that is not drawn
    (nearer than ``near``, behind the camera) or whose splat lies wholly outside the image has behind = depth = ``OFFSCREEN``
    and won = 0.  Over several cameras: minimum, sum, minimum.  ``behind`` feeds q_map.visibility_score / visibility_map as
    ``visibility``'s does.  All integer and bitwise reproducible."""
    if isinstance(cameras, Camera) or not isinstance(cameras, (list, tuple)):
        raise ValueError("cameras is a list of render.Camera, got %r" % (cameras,))
    if len(cameras) == 0:
        raise ValueError("cameras is empty: camera_visibility needs at least one camera")
    if any(not isinstance(c, Camera) for c in cameras):
        raise ValueError("cameras is a list of render.Camera, got %r" % (cameras,))
    ps_q = _ps_q(point_size)
    cloud, xyz, n, dev = _cloud("camera_visibility", cloud, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        behind, won, depth = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        if n == 0:
            return behind, won, depth
        coords, _, perm = _sorted_rows(L, cloud, xyz, dev, colours=False)
        zbuf, zbytes = _zbuffer(L, dev, [(c.H, c.W) for c in cameras])
        for k, camera in enumerate(cameras):
            pos, axes, q = _camera_args(camera)
            check(L.pcc_camera_visibility(ptr(coords), n, ptr(pos), ptr(axes), q.focal_q, q.near_q, q.H, q.W, ps_q, ptr(zbuf), zbytes,
                                          int(k > 0), ptr(behind), ptr(won), ptr(depth), _lib.stream()))
        return _input_order(perm, behind, won, depth)


def _frames(frames, n_views):
    if frames is not None:
        if not isinstance(frames, (list, tuple)) or len(frames) != n_views:
            raise ValueError("frames is None or one view_frame result per view (%d views)" % n_views)
        if any(not isinstance(fr, (list, tuple)) or len(fr) != 7 for fr in frames):
            raise ValueError("a frame is a view_frame result: (u_min, u_max, v_min, v_max, scale, ox, oy)")


def _cameras(who, cameras):
    if isinstance(cameras, Camera) or not isinstance(cameras, (list, tuple)):
        raise ValueError("cameras is a list of render.Camera, got %r" % (cameras,))
    if len(cameras) == 0:
        raise ValueError("cameras is empty: %s needs at least one camera" % who)
    if any(not isinstance(c, Camera) for c in cameras):
        raise ValueError("cameras is a list of render.Camera, got %r" % (cameras,))


def _row_index(index, perm):
    """a plane of canonically sorted row numbers (-1: background) -> the same in the input's row numbers"""
    if perm is None:
        return index
    shown = index >= 0
    return torch.where(shown, perm.to(torch.int32)[index.clamp_min(0).long()], index)


def view_buffers(cloud, front, up, H, W, frame=None, point_size=None, device=None):
    """The z-buffer ``render_view`` resolves its image from -> (index, depth): int32 [H, W] tensors on the GPU
    (``pcc_view_buffers``).  ``index`` is the row of ``cloud`` (in the INPUT's row order) every pixel shows under the renderer's
    full winner rule, -1 for background: ``render_view``'s image is ``rgb8[index]`` with the background where index < 0.
    ``depth`` is d = front . p of that row, ``OFFSCREEN`` for background.  The arguments are ``render_view``'s; colours are not
    needed.  An empty cloud gives all background."""
    r, u, f = view_axes(front, up)
    cloud, xyz, n, dev = _cloud("view_buffers", cloud, device)
    H, W = _image_size(H, W)
    if frame is None:
        frame = view_frame(xyz, f, u, H, W)
    u_min, _, _, v_max, scale, ox, oy = (int(v) for v in frame)
    point_size = scale if point_size is None else int(point_size)
    L = _lib.lib()
    with torch.cuda.device(dev):
        coords, _, perm = _sorted_rows(L, cloud, xyz, dev, colours=False)
        zbuf, zbytes = _zbuffer(L, dev, [(H, W)])
        index, depth = (torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(2))
        axes = [np.asarray(a, dtype=np.int32) for a in (r, u, f)]
        check(L.pcc_view_buffers(ptr(coords) if n else None, n, ptr(axes[0]), ptr(axes[1]), ptr(axes[2]), u_min, v_max, ox, oy, scale,
                                 point_size, H, W, ptr(zbuf), zbytes, ptr(index), ptr(depth), _lib.stream()))
        return _row_index(index, perm), depth


def camera_buffers(cloud, camera, point_size=1.0, device=None):
    """``view_buffers`` for a ``Camera`` -> (index, depth): int32 [H, W] (the camera's size) on the GPU (``pcc_camera_buffers``).
    ``depth`` is the shown row's depth key (1/256 voxel along the viewing direction), ``OFFSCREEN`` for background."""
    if not isinstance(camera, Camera):
        raise ValueError("camera_buffers: camera is a render.Camera, got %r" % (camera,))
    ps_q = _ps_q(point_size)
    cloud, xyz, n, dev = _cloud("camera_buffers", cloud, device)
    pos, axes, q = _camera_args(camera)
    L = _lib.lib()
    with torch.cuda.device(dev):
        coords, _, perm = _sorted_rows(L, cloud, xyz, dev, colours=False)
        zbuf, zbytes = _zbuffer(L, dev, [(q.H, q.W)])
        index, depth = (torch.empty((q.H, q.W), dtype=torch.int32, device=dev) for _ in range(2))
        check(L.pcc_camera_buffers(ptr(coords) if n else None, n, ptr(pos), ptr(axes), q.focal_q, q.near_q, q.H, q.W, ps_q, ptr(zbuf),
                                   zbytes, ptr(index), ptr(depth), _lib.stream()))
        return _row_index(index, perm), depth


def _sample_images(who, images, sizes):
    """one integer / bool [H, W] or [H, W, C] array or tensor per view -> ([H, W, C] int32 tensors (on their own devices), C);
    ValueError for anything else, before the GPU is touched"""
    if torch.is_tensor(images) or isinstance(images, np.ndarray) or not isinstance(images, (list, tuple)) or len(images) != len(sizes):
        raise ValueError("%s: images is a list of one image per view (%d views)" % (who, len(sizes)))
    out, channels = [], None
    for image, (H, W) in zip(images, sizes):
        t = image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image))
        if t.is_floating_point() or t.is_complex():
            raise ValueError("%s: an image holds integers or bools (the operator is exact: quantise a float image first), got %s" % (who, t.dtype))
        if t.dim() == 2:
            t = t.unsqueeze(2)
        if t.dim() != 3 or (int(t.shape[0]), int(t.shape[1])) != (H, W):
            raise ValueError("%s: an image is [H, W] or [H, W, C] of its view's size %d x %d, got %s" % (who, H, W, tuple(image.shape)))
        if not 1 <= int(t.shape[2]) <= SAMPLE_MAX_CHANNELS:
            raise ValueError("%s: an image has 1 .. %d channels, got %d" % (who, SAMPLE_MAX_CHANNELS, int(t.shape[2])))
        if channels is not None and int(t.shape[2]) != channels:
            raise ValueError("%s: every image has the same number of channels" % who)
        channels = int(t.shape[2])
        narrow = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32)
        if t.dtype not in narrow and t.numel() and not (int(t.min()) >= -0x80000000 and int(t.max()) <= 0x7FFFFFFF):
            raise ValueError("%s: image values must fit int32" % who)
        out.append(t.to(torch.int32))
    return out, channels


def _tolerance(who, tolerance):
    if tolerance is None:
        return SAMPLE_OWN
    try:
        t = int(tolerance)
        ok = t == tolerance and 0 <= t <= 0x7FFFFFFF
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s: tolerance is None (the pixels that show the point) or a whole number of voxels >= 0, got %r" % (who, tolerance))
    return t


def _sample_outputs(n, channels, dev):
    return (torch.zeros((n, channels), dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
            torch.full((n, channels), SAMPLE_NONE, dtype=torch.int32, device=dev))


def sample_views(cloud, views, images, H, W, frames=None, point_size=None, tolerance=None, device=None):
    """Carry ``images`` back to the points through ``views`` -> (total, count, peak): int64 [N, C], int32 [N], int32 [N, C]
    tensors on the GPU in the INPUT's row order (csrc/render.hip, ``pcc_view_sample``).

    For one view, with the geometry, clipping and winner rule of ``render_view`` at H x W: a pixel of point i's splat COUNTS for
    the point when it shows the point (``tolerance=None``: ``count`` is ``visibility``'s ``won``), or when the z-buffer front of the
    pixel is at most ``tolerance`` voxels in front of the point (``tolerance >= 0``: the quantity whose minimum is ``behind``, so
    count > 0 exactly where behind <= tolerance).  ``total`` is the sum of the image over the counted pixels, ``count`` their
    number, ``peak`` the maximum (``SAMPLE_NONE`` when nothing counted).  Over several views: sum, sum, maximum.  All integer and
    bitwise reproducible; the operator is exact, so callers quantise (a float image is a ValueError).

    ``images``: one integer or bool array or tensor per view, [H, W] or [H, W, C] with C <= 4.  ``views``, ``frames`` and
    ``point_size`` as in ``visibility``.  No sub-pixel sampling: a point reads whole pixels of its own splat."""
    axes = _views(views)
    _frames(frames, len(axes))
    H, W = _image_size(H, W)
    tol = _tolerance("sample_views", tolerance)
    images, channels = _sample_images("sample_views", images, [(H, W)] * len(axes))
    cloud, xyz, n, dev = _cloud("sample_views", cloud, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        total, count, peak = _sample_outputs(n, channels, dev)
        if n == 0:
            return total, count, peak
        xyz = xyz.to(dev)
        coords, _, perm = _sorted_rows(L, cloud, xyz, dev, colours=False)
        zbuf, zbytes = _zbuffer(L, dev, [(H, W)])
        for k, (r, u, f) in enumerate(axes):
            frame = view_frame(xyz, f, u, H, W) if frames is None else frames[k]
            u_min, _, _, v_max, scale, ox, oy = (int(v) for v in frame)
            size = scale if point_size is None else int(point_size)
            vecs = [np.asarray(a, dtype=np.int32) for a in (r, u, f)]
            image = images[k].to(dev).contiguous()
            check(L.pcc_view_sample(ptr(coords), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, size, H, W,
                                    ptr(zbuf), zbytes, int(k > 0), ptr(image), channels, tol, ptr(total), ptr(count), ptr(peak),
                                    _lib.stream()))
        return _input_order(perm, total, count, peak)


def sample_cameras(cloud, cameras, images, point_size=1.0, tolerance=None, device=None):
    """``sample_views`` for a non-empty list of ``Camera`` (``pcc_camera_sample``): every image has its camera's size, and
    ``tolerance`` counts whole voxels of depth as ``camera_visibility``'s ``behind`` does."""
    _cameras("sample_cameras", cameras)
    ps_q = _ps_q(point_size)
    tol = _tolerance("sample_cameras", tolerance)
    images, channels = _sample_images("sample_cameras", images, [(c.H, c.W) for c in cameras])
    cloud, xyz, n, dev = _cloud("sample_cameras", cloud, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        total, count, peak = _sample_outputs(n, channels, dev)
        if n == 0:
            return total, count, peak
        coords, _, perm = _sorted_rows(L, cloud, xyz, dev, colours=False)
        zbuf, zbytes = _zbuffer(L, dev, [(c.H, c.W) for c in cameras])
        for k, camera in enumerate(cameras):
            pos, axes, q = _camera_args(camera)
            image = images[k].to(dev).contiguous()
            check(L.pcc_camera_sample(ptr(coords), n, ptr(pos), ptr(axes), q.focal_q, q.near_q, q.H, q.W, ps_q, ptr(zbuf), zbytes,
                                      int(k > 0), ptr(image), channels, tol, ptr(total), ptr(count), ptr(peak), _lib.stream()))
        return _input_order(perm, total, count, peak)


def data_range_of(ref_min):
    """scikit-image's rule for float images when ``peak_signal_noise_ratio`` is given no data_range: 1 if the reference
    image's smallest value is >= 0, else 2 (the range of [-1, 1]) — what evaluate_view_dep.py:203 gets, since U and V are
    signed"""
    return 1.0 if ref_min >= 0 else 2.0


def _mask(who, mask, H, W, dev):
    """a bool or integer [H, W] array or tensor -> uint8 [H, W] on ``dev``, 1 where it is nonzero"""
    t = mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask))
    if t.dim() != 2 or (int(t.shape[0]), int(t.shape[1])) != (H, W):
        raise ValueError("%s: the mask is [H, W] of the images' size %d x %d, got %s" % (who, H, W, tuple(t.shape)))
    return (t.to(dev) != 0).to(torch.uint8).contiguous()


def image_compare(ref_img, img, mask=None):
    """The raw sums of ``pcc_image_compare`` for two uint8 [H, W, 3] GPU images -> eight floats: per-channel (Y, U, V) sums
    of squared differences, per-channel sums of the SSIM map over its (H - 6) x (W - 6) crop, smallest and largest YUV value
    of ``ref_img``.  Bitwise reproducible.  ``mask`` ([H, W], nonzero = inside; ``pcc_image_compare_masked``): the squared
    differences of the masked pixels only and the SSIM values of the windows whose centre pixel is masked; the last two stay
    over the whole image."""
    L = _lib.lib()
    if not (torch.is_tensor(ref_img) and torch.is_tensor(img)):
        raise ValueError("image_compare: images are uint8 [H, W, 3] tensors on the GPU")
    if ref_img.dtype != torch.uint8 or img.dtype != torch.uint8 or ref_img.dim() != 3 or ref_img.shape[2] != 3 or ref_img.shape != img.shape:
        raise ValueError("image_compare: two uint8 [H, W, 3] images of one size")
    if not ref_img.is_cuda:
        raise ValueError("image_compare runs on the GPU: got device %s" % ref_img.device)
    dev = ref_img.device
    H, W = int(ref_img.shape[0]), int(ref_img.shape[1])
    with torch.cuda.device(dev):
        a, b = ref_img.contiguous(), img.to(dev).contiguous()
        nbytes = L.pcc_image_compare_scratch_bytes(H, W)
        scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        out = torch.empty(8, dtype=torch.float64, device=dev)
        if mask is None:
            check(L.pcc_image_compare(ptr(a), ptr(b), H, W, ptr(scratch), nbytes, ptr(out), _lib.stream()))
        else:
            m = _mask("image_compare", mask, H, W, dev)
            check(L.pcc_image_compare_masked(ptr(a), ptr(b), ptr(m), H, W, ptr(scratch), nbytes, ptr(out), _lib.stream()))
        return out.tolist()


def metrics_from_sums(sums, H, W, data_range=None, pixels=None, windows=None):
    """the numbers of ``view_metrics`` from the eight raw sums of an H x W pair; ``pixels`` / ``windows``: the numbers of masked
    pixels and masked windows the sums ran over (None: all of them).  A mean over an empty set is nan."""
    n = float(H * W) if pixels is None else float(pixels)
    nan = float("nan")
    y_mse, u_mse, v_mse = ((s / n if n > 0 else nan) for s in sums[0:3])
    mse = (sums[0] + sums[1] + sums[2]) / (3.0 * n) if n > 0 else nan
    if data_range is None:
        data_range = data_range_of(sums[6])
    crop = float((H - 6) * (W - 6)) if windows is None else float(windows)
    ssim = (sums[3] / crop + sums[4] / crop + sums[5] / crop) / 3.0 if crop > 0 else nan
    if math.isnan(mse):
        psnr = nan
    else:
        psnr = math.inf if mse <= 0 else 10.0 * math.log10(float(data_range) ** 2 / mse)
    return {"psnr": psnr, "ssim": ssim, "y_mse": y_mse, "u_mse": u_mse, "v_mse": v_mse}


def view_metrics(ref_img, img, data_range=None, mask=None):
    """PSNR and SSIM of a rendered view against the reference view, in YUV as evaluate_view_dep.py:196-204 takes them ->
    {"psnr", "ssim", "y_mse", "u_mse", "v_mse"}.  PSNR = 10 log10(data_range^2 / mse), mse over all 3 H W values (inf at 0);
    ``data_range=None`` follows ``data_range_of``.  SSIM is the mean of the three channels' mean SSIM
    (structural_similarity(channel_axis=2, data_range=1.0), 7 x 7 uniform window).

    ``mask`` ([H, W], nonzero = inside) restricts the judgement to a region: the mean squared errors run over the masked pixels,
    the SSIM over the windows of its crop whose centre pixel is masked; the data-range rule still reads the whole reference.  A
    metric over an empty set (no masked pixel, or none away from the 3-pixel border) is nan.  ``mask=None`` is the whole image."""
    H, W = int(ref_img.shape[0]), int(ref_img.shape[1])
    if mask is None:
        return metrics_from_sums(image_compare(ref_img, img), H, W, data_range)
    sums = image_compare(ref_img, img, mask)
    m = _mask("view_metrics", mask, H, W, ref_img.device)
    return metrics_from_sums(sums, H, W, data_range, pixels=int(m.sum()), windows=int(m[3:H - 3, 3:W - 3].sum()))
