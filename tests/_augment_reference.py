"""numpy restatements of the training augmentations (pcc_augment_rotate, pcc_color_jitter; include/pcc_hip.h) and the inputs
the GPU tests share.

Rotate: float32 operations in the stated order (every product and sum rounded separately), np.rint, first occurrence through
np.unique(axis=0, return_index=True): the kernel must EQUAL it.

Jitter: torchvision's functional ops on float images, once in float64 and once in float32.  The GPU is held to the float64
evaluation within JITTER_TOL, which tests/test_augment_reference.py measures as four times the largest deviation of the
float32 restatement from the float64 one over the GPU tests' inputs — never against the kernel.
"""
import functools
import itertools

import numpy as np

COORD_LIMIT = 130000
COUNT_ERR_RANGE = -2

# Largest |float32 restatement - float64 restatement| over jitter_cases() (every input of tests/test_color_jitter.py),
# measured by tests/test_augment_reference.py::test_measured_jitter_tolerance, and the bound the kernel is held to: four
# times that, which covers an equally valid order of the fp32 operations and another shape of the mean's sum.
JITTER_F32_DEVIATION = 1.1882312994093702e-06      # the measured value itself
JITTER_TOL = 4 * JITTER_F32_DEVIATION


# ---------------------------------------------------------------------------------------------
# rotate
# ---------------------------------------------------------------------------------------------
def rotate_reference(coords, rot, half):
    """coords int32 [n,4], rot float32 [B,9], half -> (out_coords int32 [m,4], out_src int32 [m]) or COUNT_ERR_RANGE"""
    coords = np.asarray(coords, dtype=np.int32).reshape(-1, 4)
    rot = np.asarray(rot, dtype=np.float32).reshape(-1, 9)
    n = coords.shape[0]
    if n == 0:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int32)
    b = coords[:, 0]
    if b.min() < 0 or b.max() >= rot.shape[0]:
        return COUNT_ERR_RANGE
    h = np.float32(half)
    d = coords[:, 1:].astype(np.float32) - h                    # [n,3] float32
    R = rot[b]                                                  # [n,9]
    with np.errstate(all="ignore"):
        cols = []
        for r in range(3):
            v = (d[:, 0] * R[:, 3 * r] + d[:, 1] * R[:, 3 * r + 1]).astype(np.float32)
            v = (v + d[:, 2] * R[:, 3 * r + 2]).astype(np.float32)
            cols.append(np.rint((v + h).astype(np.float32)))
    f = np.stack(cols, axis=1)
    assert f.dtype == np.float32
    if not np.all(np.isfinite(f)) or np.any(np.abs(f) > COORD_LIMIT):
        return COUNT_ERR_RANGE
    out = np.concatenate([b[:, None], f.astype(np.int32)], axis=1).astype(np.int32)
    _, first = np.unique(out, axis=0, return_index=True)
    first = np.sort(first)
    return out[first], first.astype(np.int32)


def angle_matrix(phi, theta):
    """R_y(theta) @ R_x(phi), float32 [9] (independent of pcc_amd.augment.rotation_matrices: a plain matrix product)"""
    cp, sp, ct, st = np.cos(phi), np.sin(phi), np.cos(theta), np.sin(theta)
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], dtype=np.float64)
    Ry = np.array([[ct, 0, st], [0, 1, 0], [-st, 0, ct]], dtype=np.float64)
    return (Ry @ Rx).astype(np.float32).reshape(9)


def signed_permutations():
    """the 24 proper rotations of the cube: axis permutations with sign flips of determinant +1, float32 [24,9]"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3))
            for r in range(3):
                M[r, perm[r]] = signs[r]
            if round(np.linalg.det(M)) == 1:
                out.append(M.astype(np.float32).reshape(9))
    assert len(out) == 24
    return np.stack(out)


# entries of 0.5: with half = 63.5, x' = (x + y) / 2 exactly — .5 ties on both sides of zero — and y', z' = y/2, z/2 + 31.75
HALF_MATRIX = np.array([0.5, 0.5, 0, 0, 0.5, 0, 0, 0, 0.5], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def cube_shell(edge=128, seed=0):
    """the surface of a sphere inside an edge^3 block, about 40 k voxels for edge 128, shuffled: int32 [n,3]"""
    g = np.arange(edge, dtype=np.float64) - (edge - 1) / 2.0
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    pts = np.argwhere(np.abs(r - 0.45 * edge) < 0.5).astype(np.int32)
    return pts[np.random.default_rng(seed).permutation(pts.shape[0])].copy()


def rows_of(xyz, b=0):
    xyz = np.asarray(xyz).reshape(-1, 3)
    return np.concatenate([np.full((xyz.shape[0], 1), b), xyz], axis=1).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# jitter
# ---------------------------------------------------------------------------------------------
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def _gray(c, dt):
    return (dt(0.2989) * c[:, 0] + dt(0.587) * c[:, 1] + dt(0.114) * c[:, 2]).astype(dt)


def _blend(a, b, f, dt):
    return np.clip((f * a + (dt(1.0) - f) * b).astype(dt), dt(0.0), dt(1.0))


def _hue(c, f, dt):
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    maxc, minc = c.max(axis=1), c.min(axis=1)
    eqc = maxc == minc
    cr = maxc - minc
    ones = np.ones_like(maxc)
    s = cr / np.where(eqc, ones, maxc)
    div = np.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (dt(2.0) + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (dt(4.0) + gc - rc)
    h = np.fmod((hr + hg + hb) / dt(6.0) + dt(1.0), dt(1.0))
    h = np.mod(h + f, dt(1.0)).astype(dt)
    v = maxc
    i = np.floor(h * dt(6.0))
    t = h * dt(6.0) - i
    i = i.astype(np.int32) % 6
    one = dt(1.0)
    p = np.clip(v * (one - s), 0, 1)
    q = np.clip(v * (one - s * t), 0, 1)
    u = np.clip(v * (one - s * (one - t)), 0, 1)
    table = [(v, u, p), (q, v, p), (p, v, u), (p, q, v), (u, p, v), (v, p, q)]
    out = np.empty_like(c)
    for ch in range(3):
        out[:, ch] = np.choose(i, [table[k][ch] for k in range(6)])
    assert out.dtype == dt
    return out


def jitter_item(rgb, params, order, dtype=np.float64):
    """one item: rgb [n,3] in [0,1], params (b, c, s, h), order a permutation of 0..3 -> [n,3] of ``dtype``"""
    dt = np.dtype(dtype).type
    c = np.asarray(rgb, dtype=np.float32).astype(dt)
    par = [dt(np.float32(p)) for p in params]
    if c.shape[0] == 0:
        return c
    for op in order:
        f = par[op]
        if op == BRIGHTNESS:
            c = _blend(c, np.zeros_like(c), f, dt)
        elif op == CONTRAST:
            m = dt(np.mean(_gray(c, dt), dtype=dt))
            c = _blend(c, np.full_like(c, m), f, dt)
        elif op == SATURATION:
            c = _blend(c, _gray(c, dt)[:, None], f, dt)
        elif op == HUE:
            c = _hue(c, f, dt)
        else:
            raise ValueError(op)
        assert c.dtype == dt
    return c


def jitter_reference(rgb, offsets, params, order, dtype=np.float64):
    rgb = np.asarray(rgb, dtype=np.float32)
    out = np.empty(rgb.shape, dtype=dtype)
    for i in range(len(offsets) - 1):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        out[lo:hi] = jitter_item(rgb[lo:hi], params[i], order[i], dtype)
    return out


ORDERS = [list(p) for p in itertools.permutations(range(4))]
JITTER_CHUNK = 1024                                         # pcc_color_jitter_chunk(): the GPU test asserts it
ITEM_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)


def special_colours():
    """gray points (cr = 0), black, white, the pure primaries and secondaries, and ties of the maximum and of the minimum"""
    return np.array([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [0, 0, 0], [1, 1, 1],
                     [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1],
                     [0.75, 0.75, 0.25], [0.25, 0.75, 0.75], [0.75, 0.25, 0.75],      # r = g > b, g = b > r, r = b > g
                     [0.75, 0.25, 0.25], [0.25, 0.75, 0.25], [0.25, 0.25, 0.75],      # two equal minima
                     [1.0, 0.999999, 0.0], [0.1, 0.1000001, 0.1]], dtype=np.float32)


def _colours(n, rng):
    c = rng.random((n, 3), dtype=np.float32)
    sp = special_colours()
    k = min(n, sp.shape[0])
    c[:k] = sp[:k]
    return c


@functools.lru_cache(maxsize=None)
def jitter_cases():
    """name -> (rgb float32 [n,3], offsets int64 [B+1], params float32 [B,4], order int32 [B,4]); every input of the GPU test"""
    rng = np.random.default_rng(2024)
    cases = {}

    def add(name, sizes, params, orders):
        sizes = list(sizes)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        rgb = _colours(int(off[-1]), rng)
        cases[name] = (rgb, off, np.asarray(params, dtype=np.float32).reshape(len(sizes), 4),
                       np.asarray(orders, dtype=np.int32).reshape(len(sizes), 4))

    def draw(k):
        par = np.stack([rng.uniform(0.7, 1.3, k), rng.uniform(0.7, 1.3, k), rng.uniform(0.7, 1.3, k), rng.uniform(-0.3, 0.3, k)], 1)
        return par, [ORDERS[int(i)] for i in rng.integers(0, 24, k)]

    # the item sizes, one batch: 1, 63/64/65, 1023/1024/1025 (= the chunk +-1), two chunks +-1
    par, orders = draw(len(ITEM_SIZES))
    add("sizes", ITEM_SIZES, par, orders)
    # an empty item in the middle of a batch (and one at each end)
    par, orders = draw(5)
    add("empty", (0, 300, 0, 1500, 0), par, orders)
    # all 24 orders on one small item each
    par, _ = draw(24)
    add("orders", [40] * 24, par, ORDERS)
    # factor extremes, hue +-0.3 wrapping in both directions, contrast at each position
    ext = [(0.7, 0.7, 0.7, -0.3), (1.3, 1.3, 1.3, 0.3), (0.7, 1.3, 0.7, 0.3), (1.3, 0.7, 1.3, -0.3),
           (1.0, 1.0, 1.0, 0.0), (1.0, 1.0, 0.0, 0.0), (1.3, 1.3, 1.3, -0.3), (0.7, 0.7, 1.3, 0.3)]
    add("extremes", [200] * 8, ext, [ORDERS[0], ORDERS[23], ORDERS[9], ORDERS[14], ORDERS[0], ORDERS[5], ORDERS[17], ORDERS[20]])
    # a cube-sized item
    par, orders = draw(2)
    add("large", (40000, 5000), par, orders)
    return cases
