"""Plain numpy restatement of render.visibility and q_map.visibility_score: what tests/test_visibility_reference.py,
tests/test_visibility.py and tests/test_visibility_harness.py hold the operators to.  Written from the specification, not
from the kernel: a painter's loop that paints a depth buffer and a winner buffer (far to near; among equal depth the
higher row first, so the lowest row is what stays), then a second walk over every splat.  No atomics, no packed words."""
import numpy as np

from _view_reference import axes, frame_of

OFFSCREEN = 2147483647
COORD_LIMIT = 130000


def canonical_order(xyz):
    """the permutation that puts integer [N, 3] rows in ascending (x, y, z) order"""
    xyz = np.asarray(xyz)
    return np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0]))


def view_visibility(xyz, front, up, H, W, frame, point_size=None):
    """(behind, won), int64 [N] each, of rows given in canonical order for ONE view.  A row with a coordinate beyond
    COORD_LIMIT paints nothing and gets (OFFSCREEN, 0)."""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    r, u, f = axes(front, up)
    u_min, _, _, v_max, scale, ox, oy = frame
    ps = scale if point_size is None else point_size
    n = xyz.shape[0]
    behind, won = np.full(n, OFFSCREEN, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if n == 0:
        return behind, won
    uu, vv, dd = xyz @ r, xyz @ u, xyz @ f
    drawn = (np.abs(xyz) <= COORD_LIMIT).all(axis=1)

    def box(i):                                          # the splat clipped to the image: rows r0:r1, columns c0:c1 (maybe empty)
        c0, r0 = (int(uu[i]) - u_min) * scale + ox, (v_max - int(vv[i])) * scale + oy
        return max(r0, 0), min(r0 + ps, H), max(c0, 0), min(c0 + ps, W)

    depth = np.zeros((H, W), dtype=np.int64)
    winner = np.full((H, W), -1, dtype=np.int64)
    for i in np.lexsort((-np.arange(n), dd)):            # ascending depth; among equal depth descending row
        if not drawn[i]:
            continue
        r0, r1, c0, c1 = box(i)
        if r0 < r1 and c0 < c1:
            depth[r0:r1, c0:c1] = dd[i]
            winner[r0:r1, c0:c1] = i
    for i in range(n):
        if not drawn[i]:
            continue
        r0, r1, c0, c1 = box(i)
        if r0 < r1 and c0 < c1:
            behind[i] = int((depth[r0:r1, c0:c1] - dd[i]).min())
            won[i] = int((winner[r0:r1, c0:c1] == i).sum())
    return behind, won


def visibility(xyz, views, H, W, frames=None, point_size=None):
    """render.visibility for integer [N, 3] rows in ANY order (duplicate-free) and a list of (front, up) pairs ->
    (behind, won) in the input's row order: the minimum / the sum over the views; frames=None frames the cloud itself"""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    order = canonical_order(xyz)
    rows = xyz[order]
    behind, won = np.full(len(rows), OFFSCREEN, dtype=np.int64), np.zeros(len(rows), dtype=np.int64)
    for k, (front, up) in enumerate(views):
        if frames is not None:
            frame = frames[k]
        elif len(rows):
            frame = frame_of(rows, front, up, H, W)
        else:
            frame = (0, 0, 0, 0, max(1, min(W, H)), (W - max(1, min(W, H))) // 2, (H - max(1, min(W, H))) // 2)
        b, w = view_visibility(rows, front, up, H, W, frame, point_size)
        behind, won = np.minimum(behind, b), won + w
    out_b, out_w = np.empty_like(behind), np.empty_like(won)
    out_b[order], out_w[order] = behind, won
    return out_b, out_w


def score(behind, tolerance=2, falloff=8, floor=0.0):
    """q_map.visibility_score in numpy float64"""
    b = np.asarray(behind, dtype=np.int64)
    hidden = np.maximum(b.astype(np.float64) - float(tolerance), 0.0)
    if falloff > 0:
        w = np.maximum(1.0 - hidden / float(falloff), 0.0)
    else:
        w = (hidden == 0).astype(np.float64)
    w = np.where(b == OFFSCREEN, 0.0, w)
    return float(floor) + (1.0 - float(floor)) * w
