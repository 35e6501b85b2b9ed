"""Plain restatement of the pinhole-camera views (render.Camera, render_camera, camera_visibility, q_map.distance_score): what
tests/test_camera_reference.py, tests/test_camera.py and tests/test_camera_harness.py hold the operators to.  Written from the
specification, not from the kernel: Python integers throughout (no width to overflow), a painter's loop that paints a depth-key
buffer and a winner buffer far to near (among equal keys the higher row first, so the lowest row is what stays), then a second
walk over every splat.  No packed words, no atomics.

A camera is the tuple of integers that crosses the C interface: (pos_q[3], axes_q[3][3] = right, up, front, focal_q, near_q, H, W)."""
import math

import numpy as np

OFFSCREEN = 2147483647
COORD_LIMIT = 130000


def quantise(position, look_at=None, front=None, up=(0, 1, 0), fov_y=None, focal=None, H=None, W=None, near=1.0):
    """the specification's camera in float64 -> its integers"""
    position = np.asarray(position, dtype=np.float64)
    f = position - np.asarray(look_at, dtype=np.float64) if look_at is not None else np.asarray(front, dtype=np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(np.asarray(up, dtype=np.float64), f)
    r = r / np.linalg.norm(r)
    u = np.cross(f, r)
    if fov_y is not None:
        focal = (H / 2.0) / math.tan(math.radians(fov_y) / 2.0)
    pos_q = tuple(int(v) for v in np.rint(16.0 * position))
    axes_q = tuple(tuple(int(v) for v in np.rint(16384.0 * a)) for a in (r, u, f))
    return pos_q, axes_q, int(np.rint(16.0 * focal)), int(np.rint(16.0 * near)), int(H), int(W)


def ps_q_of(point_size):
    return int(np.rint(16.0 * float(point_size)))


def project(p, cam, ps_q=16):
    """one point -> None when it draws nothing, else (col0, row0, s, dk, X, Y, D).  Python's // rounds towards -inf."""
    pos_q, (right, up, front), focal_q, near_q, H, W = cam
    p = [int(v) for v in p]
    if any(abs(v) > COORD_LIMIT for v in p):
        return None
    e = [16 * p[k] - int(pos_q[k]) for k in range(3)]
    U = sum(int(right[k]) * e[k] for k in range(3))
    V = sum(int(up[k]) * e[k] for k in range(3))
    D = -sum(int(front[k]) * e[k] for k in range(3))
    if D < near_q * 2 ** 14:
        return None
    X, Y = (focal_q * U) // D, (focal_q * V) // D
    s = min(max(-((-(focal_q * ps_q * 2 ** 10)) // D), 1), 16)
    col0, row0 = (8 * W + X - 8 * s) // 16, (8 * H - Y - 8 * s) // 16
    return col0, row0, s, D >> 10, X, Y, D


def canonical_order(xyz):
    xyz = np.asarray(xyz)
    return np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0]))


def paint(xyz, cam, ps_q=16):
    """rows AS GIVEN (the row index is the tie rule's) -> (key [H, W] with -1 where nothing was drawn, winner [H, W] with -1,
    behind, won, depth) for ONE camera"""
    H, W = cam[4], cam[5]
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    n = xyz.shape[0]
    boxes = []
    for i in range(n):
        pr = project(xyz[i], cam, ps_q)
        if pr is None:
            boxes.append(None)
            continue
        col0, row0, s, dk = pr[:4]
        r0, r1, c0, c1 = max(row0, 0), min(row0 + s, H), max(col0, 0), min(col0 + s, W)
        boxes.append((r0, r1, c0, c1, dk) if r0 < r1 and c0 < c1 else None)
    key = np.full((H, W), -1, dtype=np.int64)
    winner = np.full((H, W), -1, dtype=np.int64)
    drawn = [i for i in range(n) if boxes[i] is not None]
    for i in sorted(drawn, key=lambda i: (-boxes[i][4], -i)):          # far to near; among equal keys descending row
        r0, r1, c0, c1, dk = boxes[i]
        key[r0:r1, c0:c1] = dk
        winner[r0:r1, c0:c1] = i
    behind, won, depth = np.full(n, OFFSCREEN, dtype=np.int64), np.zeros(n, dtype=np.int64), np.full(n, OFFSCREEN, dtype=np.int64)
    for i in drawn:
        r0, r1, c0, c1, dk = boxes[i]
        behind[i] = int(((dk - key[r0:r1, c0:c1]) >> 8).min())
        won[i] = int((winner[r0:r1, c0:c1] == i).sum())
        depth[i] = dk
    return key, winner, behind, won, depth


def image_of(winner, rgb8, background=(255, 255, 255)):
    img = np.empty(winner.shape + (3,), dtype=np.uint8)
    img[:] = np.asarray(background, dtype=np.uint8)
    shown = winner >= 0
    img[shown] = np.asarray(rgb8, dtype=np.uint8).reshape(-1, 3)[winner[shown]]
    return img


def colours_to_bytes(rgb):
    return np.clip(np.rint(np.asarray(rgb, dtype=np.float32) * np.float32(255.0)), 0, 255).astype(np.uint8)


def render_camera(cloud, cam, point_size=1.0, background=(255, 255, 255)):
    """render.render_camera for [N, 6] rows in ANY order (duplicate-free) -> uint8 [H, W, 3]"""
    cloud = np.asarray(cloud).reshape(-1, 6)
    xyz = np.rint(cloud[:, :3]).astype(np.int64)
    order = canonical_order(xyz)
    _, winner, _, _, _ = paint(xyz[order], cam, ps_q_of(point_size))
    return image_of(winner, colours_to_bytes(cloud[order, 3:6]), background)


def camera_visibility(xyz, cams, point_size=1.0):
    """render.camera_visibility for integer [N, 3] rows in ANY order (duplicate-free) -> (behind, won, depth) in the input's
    row order: minimum / sum / minimum over the cameras"""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    order = canonical_order(xyz)
    n = xyz.shape[0]
    behind, won, depth = np.full(n, OFFSCREEN, dtype=np.int64), np.zeros(n, dtype=np.int64), np.full(n, OFFSCREEN, dtype=np.int64)
    for cam in cams:
        _, _, b, w, d = paint(xyz[order], cam, ps_q_of(point_size))
        behind, won, depth = np.minimum(behind, b), won + w, np.minimum(depth, d)
    out = [np.empty_like(a) for a in (behind, won, depth)]
    for o, a in zip(out, (behind, won, depth)):
        o[order] = a
    return tuple(out)


def distance_score(depth, focal, full=1.0, floor=0.0):
    """q_map.distance_score in numpy float64"""
    d = np.asarray(depth, dtype=np.int64)
    score = np.clip(((float(focal) * 256.0) / d.astype(np.float64)) / float(full), float(floor), 1.0)
    return np.where(d == OFFSCREEN, 0.0, score)


# ---- the inputs of the GPU cases (tests/test_camera.py); tests/test_camera_reference.py asserts what they must exercise ----
BOX = 24
CENTRE = (11.5, 11.5, 11.5)


def exactly(n, grid, seed):
    """n distinct voxels of a grid^3 box in random row order"""
    rng = np.random.default_rng(seed)
    xyz = np.unique(rng.integers(0, grid, size=(2 * n + 8, 3)), axis=0)
    rng.shuffle(xyz)
    assert xyz.shape[0] >= n
    return xyz[:n].astype(np.int64)


def axis_camera(front, up, distance, focal, H, W, near=1.0):
    """a camera on the axis ``front`` through the box centre, ``distance`` voxels from it: exact integers"""
    pos = tuple(c + distance * f for c, f in zip(CENTRE, front))
    return quantise(pos, front=front, up=up, focal=focal, H=H, W=W, near=near)


AXIS_VIEWS = [((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)), ((1, 0, 0), (0, 1, 0)), ((-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)),
              ((0, -1, 0), (1, 0, 0))]


def oblique_camera(H=128, W=96):
    return quantise((300, -200, 500), look_at=CENTRE, fov_y=40, H=H, W=W)


def oblique_case(n=1000, seed=2000):
    """n voxels of the box, four voxels far to the sides (in range, outside the image) and two rows beyond the coordinate range,
    in shuffled order, seen by the oblique camera at 128 x 96 -> (rows [n + 6, 3], camera)"""
    extra = np.array([[-2000, 11, 11], [11, 3000, 11], [11, 11, -4000], [2500, 2500, 0], [0, 0, COORD_LIMIT + 1], [-COORD_LIMIT - 1, 5, 5]],
                     dtype=np.int64)
    rows = np.concatenate([exactly(n, BOX, seed), extra])
    np.random.default_rng(seed + 1).shuffle(rows)
    return rows, oblique_camera()


def inside_camera(H=30, W=28):
    """in the middle of the box, looking along -z: rows on both sides of the near plane"""
    return quantise((11.5, 11.5, 11.5), front=(0, 0, 1), up=(0, 1, 0), focal=20.0, H=H, W=W, near=2.0)


def far_camera(H=30, W=28):
    """so far away that every voxel projects to less than a pixel: every s = 1"""
    return quantise((11.5, 11.5, 20000.0), front=(0, 0, 1), up=(0, 1, 0), focal=4000.0, H=H, W=W)


def near_camera(H=128, W=96):
    """so near that every voxel projects beyond 16 pixels: every s clamps at 16"""
    return quantise((11.5, 11.5, 40.0), front=(0, 0, 1), up=(0, 1, 0), focal=1000.0, H=H, W=W)


def clip_case():
    """the solid 8 x 8 x 24 core of the box under the near camera: every voxel 16 pixels wide, the core far wider than the image
    -> (xyz, camera, {name: mask of the rows whose splat is cut at that edge or corner and still partly inside})"""
    xyz = np.stack(np.meshgrid(np.arange(8, 16), np.arange(8, 16), np.arange(BOX), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    np.random.default_rng(31).shuffle(xyz)
    cam = near_camera()
    H, W = cam[4], cam[5]
    pr = [project(p, cam) for p in xyz]
    col, row, s = (np.array([p[k] for p in pr]) for k in range(3))
    left, right, top, bottom = (col < 0) & (col + s > 0), (col < W) & (col + s > W), (row < 0) & (row + s > 0), (row < H) & (row + s > H)
    in_rows, in_cols = (row + s > 0) & (row < H), (col + s > 0) & (col < W)
    cuts = {"left": left & in_rows, "right": right & in_rows, "top": top & in_cols, "bottom": bottom & in_cols, "top left": left & top,
            "top right": right & top, "bottom left": left & bottom, "bottom right": right & bottom}
    return xyz, cam, cuts


def tie_case():
    """voxels mirrored about the optical axis of an axis-aligned camera: equal depth keys, overlapping splats (rows 0 and 1 share
    columns on the same image rows), and one voxel behind them"""
    xyz = np.array([[11, 11, 5], [12, 11, 5], [11, 12, 5], [12, 12, 5], [11, 11, 2]], dtype=np.int64)
    cam = quantise((11.5, 11.5, 30.0), front=(0, 0, 1), up=(0, 1, 0), focal=120.0, H=30, W=28)
    return xyz, cam
