"""Plain restatement of the z-buffer planes and of the back-projection of images onto points (render.view_buffers,
camera_buffers, sample_views, sample_cameras): what tests/test_sample_reference.py, tests/test_view_buffers.py,
tests/test_view_sample.py and tests/test_screen_map.py hold the operators to.  Written from the specification, not from the
kernel: Python integers, a painter's loop, no packed words, no atomics.  Built on the projections and framings of
tests/_view_reference.py and tests/_camera_reference.py.

Both kinds of view are reduced to one list of BOXES, one per row in canonical order: None for a row that draws nothing inside the
image, else (r0, r1, c0, c1, near) with the splat clipped to the image and ``near`` an integer that is larger for the nearer
point: d = front . p for the orthographic view, -dk for the camera.  The gap between a pixel's front and a point is then
(near_front - near_point) >> shift, shift 0 for the view (whole voxels) and 8 for the camera (dk is in 1/256 voxel).

The back-projection is written twice, and tests/test_sample_reference.py holds the two equal:
  per point (``sample_per_point``): paint the front and the winner of every pixel far to near, then walk every row's box;
  per pixel (``sample_per_pixel``): for every pixel collect the rows whose box covers it, take its front and its winner as a
  maximum over that list, and scatter the pixel's value to the rows of the list that count."""
import numpy as np

import _camera_reference as cref
from _view_reference import axes, frame_of

OFFSCREEN = 2147483647
NONE = -2147483648
COORD_LIMIT = 130000
VIEW_SHIFT, CAMERA_SHIFT = 0, 8


def canonical_order(xyz):
    xyz = np.asarray(xyz)
    return np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0]))


def view_boxes(xyz, front, up, H, W, frame, point_size=None):
    """rows AS GIVEN -> boxes of the orthographic view"""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    r, u, f = axes(front, up)
    u_min, _, _, v_max, scale, ox, oy = (int(v) for v in frame)
    ps = scale if point_size is None else int(point_size)
    out = []
    for p in xyz:
        p = [int(v) for v in p]
        if any(abs(v) > COORD_LIMIT for v in p):
            out.append(None)
            continue
        uu, vv, dd = (sum(int(a[k]) * p[k] for k in range(3)) for a in (r, u, f))
        c0, r0 = (uu - u_min) * scale + ox, (v_max - vv) * scale + oy
        box = (max(r0, 0), min(r0 + ps, H), max(c0, 0), min(c0 + ps, W), dd)
        out.append(box if box[0] < box[1] and box[2] < box[3] else None)
    return out


def camera_boxes(xyz, cam, ps_q=16):
    """rows AS GIVEN -> boxes of the camera (a tuple of _camera_reference.quantise)"""
    H, W = cam[4], cam[5]
    out = []
    for p in np.asarray(xyz, dtype=np.int64).reshape(-1, 3):
        pr = cref.project(p, cam, ps_q)
        if pr is None:
            out.append(None)
            continue
        col0, row0, s, dk = pr[:4]
        box = (max(row0, 0), min(row0 + s, H), max(col0, 0), min(col0 + s, W), -dk)
        out.append(box if box[0] < box[1] and box[2] < box[3] else None)
    return out


def paint(boxes, H, W):
    """painter's loop: far to near and, among equal depth, the higher row first -> (winner [H, W] with -1 for background,
    near [H, W] (0 where winner is -1))"""
    winner = np.full((H, W), -1, dtype=np.int64)
    near = np.zeros((H, W), dtype=np.int64)
    drawn = [i for i, b in enumerate(boxes) if b is not None]
    for i in sorted(drawn, key=lambda i: (boxes[i][4], -i)):
        r0, r1, c0, c1, nk = boxes[i]
        winner[r0:r1, c0:c1] = i
        near[r0:r1, c0:c1] = nk
    return winner, near


def buffers(boxes, H, W, camera):
    """-> (index, depth) int64 [H, W] as pcc_view_buffers (camera=False: depth = d) / pcc_camera_buffers (True: depth = dk)"""
    winner, near = paint(boxes, H, W)
    depth = np.where(winner >= 0, -near if camera else near, OFFSCREEN)
    return winner, depth


def _image(image, H, W):
    img = np.asarray(image)
    img = img[:, :, None] if img.ndim == 2 else img
    assert img.shape[:2] == (H, W) and img.dtype.kind in "biu"
    return img.astype(np.int64)


def _empty(n, C):
    return np.zeros((n, C), dtype=np.int64), np.zeros(n, dtype=np.int64), np.full((n, C), NONE, dtype=np.int64)


def sample_per_point(boxes, image, H, W, shift, tolerance):
    """(total [n, C], count [n], peak [n, C]) int64 for ONE view: every row walks its own box over the painted planes.
    tolerance None: the pixels whose winner is the row; else the pixels with (front - own) >> shift <= tolerance."""
    img = _image(image, H, W)
    winner, near = paint(boxes, H, W)
    total, count, peak = _empty(len(boxes), img.shape[2])
    for i, b in enumerate(boxes):
        if b is None:
            continue
        r0, r1, c0, c1, nk = b
        if tolerance is None:
            counts = winner[r0:r1, c0:c1] == i
        else:
            counts = ((near[r0:r1, c0:c1] - nk) >> shift) <= tolerance
        if counts.any():
            values = img[r0:r1, c0:c1][counts]
            count[i], total[i], peak[i] = values.shape[0], values.sum(axis=0), values.max(axis=0)
    return total, count, peak


def sample_per_pixel(boxes, image, H, W, shift, tolerance):
    """the same three arrays, pixel by pixel: the rows that cover a pixel, its front and winner as a maximum over them, then a
    scatter of the pixel's value"""
    img = _image(image, H, W)
    total, count, peak = _empty(len(boxes), img.shape[2])
    cover = {}
    for i, b in enumerate(boxes):
        if b is None:
            continue
        for y in range(b[0], b[1]):
            for x in range(b[2], b[3]):
                cover.setdefault((y, x), []).append(i)
    for (y, x), rows in cover.items():
        front, win = max((boxes[i][4], -i) for i in rows)
        for i in rows:
            counts = i == -win if tolerance is None else ((front - boxes[i][4]) >> shift) <= tolerance
            if counts:
                count[i] += 1
                total[i] += img[y, x]
                peak[i] = np.maximum(peak[i], img[y, x])
    return total, count, peak


def fold(results):
    """single-view results -> their fold over the views: sum, sum, maximum"""
    total, count, peak = (np.array(a) for a in results[0])
    for t, c, p in results[1:]:
        total, count, peak = total + t, count + c, np.maximum(peak, p)
    return total, count, peak


def _back(order, arrays):
    out = []
    for a in arrays:
        o = np.empty_like(a)
        o[order] = a
        out.append(o)
    return tuple(out)


def _frame(rows, front, up, H, W):
    if len(rows):
        return frame_of(rows, front, up, H, W)
    s = max(1, min(W, H))
    return 0, 0, 0, 0, s, (W - s) // 2, (H - s) // 2


def sample_views(xyz, views, images, H, W, frames=None, point_size=None, tolerance=None, formulation=sample_per_point):
    """render.sample_views for integer [N, 3] rows in ANY order (duplicate-free) and (front, up) pairs, in the input's row order"""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    order = canonical_order(xyz)
    rows, res = xyz[order], []
    for k, (front, up) in enumerate(views):
        frame = frames[k] if frames is not None else _frame(rows, front, up, H, W)
        res.append(formulation(view_boxes(rows, front, up, H, W, frame, point_size), images[k], H, W, VIEW_SHIFT, tolerance))
    return _back(order, fold(res))


def sample_cameras(xyz, cams, images, point_size=1.0, tolerance=None, formulation=sample_per_point):
    """render.sample_cameras likewise; a camera is _camera_reference's tuple of integers"""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    order = canonical_order(xyz)
    rows = xyz[order]
    res = [formulation(camera_boxes(rows, cam, cref.ps_q_of(point_size)), images[k], cam[4], cam[5], CAMERA_SHIFT, tolerance)
           for k, cam in enumerate(cams)]
    return _back(order, fold(res))


def _index_back(winner, order):
    return np.where(winner >= 0, np.asarray(order)[np.maximum(winner, 0)], -1)


def view_buffers(xyz, front, up, H, W, frame=None, point_size=None):
    """render.view_buffers for rows in ANY order -> (index in the input's row numbers, depth)"""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    order = canonical_order(xyz)
    rows = xyz[order]
    winner, depth = buffers(view_boxes(rows, front, up, H, W, _frame(rows, front, up, H, W) if frame is None else frame, point_size), H, W, False)
    return _index_back(winner, order), depth


def camera_buffers(xyz, cam, point_size=1.0):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    order = canonical_order(xyz)
    winner, depth = buffers(camera_boxes(xyz[order], cam, cref.ps_q_of(point_size)), cam[4], cam[5], True)
    return _index_back(winner, order), depth


def tallies(count):
    """(rows with count > 0, rows with count == 0): what every GPU case pins as constants before it compares"""
    count = np.asarray(count)
    return int((count > 0).sum()), int((count == 0).sum())


# ---- image score and image makers (q_map.image_score, box_image, gaze_image) in numpy float64 ----
def image_score(total, count, peak, reduce="max", channel=0, scale=255, floor=0.0):
    total, count, peak = (np.asarray(a, dtype=np.int64) for a in (total, count, peak))
    if reduce == "max":
        v = peak[:, channel].astype(np.float64)
    else:
        v = total[:, channel].astype(np.float64) / np.maximum(count, 1).astype(np.float64)
    w = np.where(count > 0, np.clip(v / float(scale), 0.0, 1.0), 0.0)
    return float(floor) + (1.0 - float(floor)) * w


def box_image(H, W, box):
    r0, r1, c0, c1 = box
    img = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            if r0 <= y < r1 and c0 <= x < c1:
                img[y, x] = 255
    return img


def gaze_image(H, W, gaze, radius, falloff):
    img = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            dist = np.sqrt(np.float64((y - gaze[0]) * (y - gaze[0]) + (x - gaze[1]) * (x - gaze[1])))
            w = min(max(1.0 - (dist - radius) / falloff, 0.0), 1.0) if falloff > 0 else float(dist <= radius)
            img[y, x] = int(np.rint(255.0 * w))
    return img


# ---- masked view metrics ----
def masked_metrics(ref_img, img, mask, data_range=None):
    """render.view_metrics(mask=...) in numpy: the errors over the masked pixels, the SSIM over the windows whose centre is masked"""
    import math
    from _view_reference import ssim_map, yuv
    a, b = yuv(np.asarray(ref_img)), yuv(np.asarray(img))
    m = np.asarray(mask) != 0
    H, W = m.shape
    nan = float("nan")
    err = (a - b) ** 2
    chan = [float(err[..., k][m].mean()) if m.any() else nan for k in range(3)]
    mse = float(err[m].mean()) if m.any() else nan
    if data_range is None:
        data_range = 1.0 if a.min() >= 0 else 2.0
    centre = m[3:H - 3, 3:W - 3]
    ssim = float(np.mean([ssim_map(a[..., k], b[..., k])[centre].mean() for k in range(3)])) if centre.any() else nan
    psnr = nan if math.isnan(mse) else (math.inf if mse == 0 else 10.0 * math.log10(data_range ** 2 / mse))
    return {"psnr": psnr, "ssim": ssim, "y_mse": chan[0], "u_mse": chan[1], "v_mse": chan[2]}


# ---- the inputs of the GPU cases (tests/test_view_sample.py); tests/test_sample_reference.py holds the two formulations equal on them ----
FRONT, SIDE = ((0, 0, 1), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0))
TOLERANCES = (None, 0, 3, 2 ** 31 - 2)
BIG = 2 ** 31 - 1


def random_image(H, W, C, seed, extreme=False):
    """int32 [H, W, C]: values in +-1000, or every value one of +-(2^31 - 1)"""
    rng = np.random.default_rng(seed)
    if extreme:
        return np.where(rng.integers(0, 2, size=(H, W, C)) == 1, BIG, -BIG).astype(np.int32)
    return rng.integers(-1000, 1001, size=(H, W, C)).astype(np.int32)


def cases():
    """name -> {"kind": "camera" | "view", "xyz", "cam" | ("view", "H", "W", "frame", "point_size"), "point_size"}"""
    out = {}
    xyz, cam, _ = cref.clip_case()
    out["clip"] = dict(kind="camera", xyz=xyz, cam=cam, point_size=1.0)
    xyz, cam = cref.tie_case()
    out["tie"] = dict(kind="camera", xyz=xyz, cam=cam, point_size=1.0)
    xyz, cam = cref.oblique_case(n=700)
    xyz = xyz[(np.abs(xyz) <= COORD_LIMIT).all(axis=1)]              # the Python entry points refuse rows beyond the range
    out["off_screen"] = dict(kind="camera", xyz=xyz, cam=cam, point_size=1.0)
    out["near_plane"] = dict(kind="camera", xyz=cref.exactly(600, cref.BOX, 77), cam=cref.inside_camera(), point_size=2.0)
    out["camera_1x1"] = dict(kind="camera", xyz=cref.exactly(300, cref.BOX, 78), cam=cref.axis_camera((0, 0, 1), (0, 1, 0), 60.0, 2.0, 1, 1),
                             point_size=1.0)
    box = cref.exactly(1000, 24, 79)
    out["view_size_1"] = dict(kind="view", xyz=box, view=FRONT, H=81, W=76, frame=frame_of(box, *FRONT, 81, 76, scale=3), point_size=1)
    out["view_size_16"] = dict(kind="view", xyz=box, view=SIDE, H=57, W=52, frame=frame_of(box, *SIDE, 57, 52, scale=2), point_size=16)
    out["view_off_screen"] = dict(kind="view", xyz=box, view=FRONT, H=100, W=90, frame=(0, 23, 0, 23, 3, -30, 40), point_size=5)
    out["view_1x1"] = dict(kind="view", xyz=box, view=FRONT, H=1, W=1, frame=(0, 23, 0, 23, 1, -11, -12), point_size=3)
    return out


def case_size(case):
    return (case["cam"][4], case["cam"][5]) if case["kind"] == "camera" else (case["H"], case["W"])


def case_sample(case, image, tolerance, formulation=sample_per_point):
    """the reference's (total, count, peak) of a case, in the input's row order"""
    if case["kind"] == "camera":
        return sample_cameras(case["xyz"], [case["cam"]], [image], point_size=case["point_size"], tolerance=tolerance, formulation=formulation)
    return sample_views(case["xyz"], [case["view"]], [image], case["H"], case["W"], frames=[case["frame"]], point_size=case["point_size"],
                        tolerance=tolerance, formulation=formulation)
