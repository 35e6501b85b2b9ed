"""RAHT restated in numpy float64, twice: the closed-form plan and step-by-step transform that include/pcc_hip.h specifies
(pcc_raht_plan / pcc_raht_transform; same operation order, so the GPU can be compared with it coefficient by coefficient), and,
separately, the textbook recursive definition over the octree (no plan, no steps: split the rows at the top key bit, transform the
halves, merge their DCs).  Also the quantiser, the per-context table choice of the PCR1 stream, and the clouds the tests share."""
import functools

import numpy as np

MAX_DEPTH = 17


def morton_keys(coords, origin, depth):
    """coords int [N,3] -> (uint64 keys, in_grid mask): bit 3b+2 = x's bit b, 3b+1 = y's, 3b = z's; 0 for a row outside the grid"""
    g = np.asarray(coords, dtype=np.int64) - np.asarray(origin, dtype=np.int64)
    ok = ((g >= 0) & (g < (1 << depth))).all(axis=1)
    g = np.where(ok[:, None], g, 0).astype(np.uint64)
    key = np.zeros(g.shape[0], dtype=np.uint64)
    for b in range(depth):
        for axis in range(3):
            key |= ((g[:, axis] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - axis)
    return key, ok


def default_origin_depth(coords):
    c = np.asarray(coords, dtype=np.int64)
    lo = c.min(axis=0)
    return lo, int((c.max(axis=0) - lo).max()).bit_length()


def plan(coords, origin=None, depth=None):
    """-> dict of int32 arrays perm, step, left, w0, w1, step_rows, step_offsets and status = [outside, duplicates], as
    pcc_raht_plan writes them"""
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    n = coords.shape[0]
    o, d = default_origin_depth(coords)
    origin = o if origin is None else origin
    depth = d if depth is None else depth
    key, ok = morton_keys(coords, origin, depth)
    perm = np.argsort(key, kind="stable")
    key = key[perm]
    step = np.full(n, -1, dtype=np.int64)
    left = np.arange(n, dtype=np.int64)
    w0 = np.zeros(n, dtype=np.int64)
    w1 = np.zeros(n, dtype=np.int64)
    duplicates = 0
    for i in range(1, n):
        diff = int(key[i]) ^ int(key[i - 1])
        if diff == 0:
            duplicates += 1
            continue
        s = diff.bit_length() - 1
        step[i] = s
        left[i] = np.searchsorted(key >> np.uint64(s + 1), key[i] >> np.uint64(s + 1), side="left")
        w0[i] = i - left[i]
        w1[i] = np.searchsorted(key >> np.uint64(s), key[i] >> np.uint64(s), side="right") - i
    left[0] = 0
    bucket = np.where(step < 0, 63, step)
    step_rows = np.argsort(bucket, kind="stable")
    step_offsets = np.searchsorted(bucket[step_rows], np.arange(3 * depth + 1), side="left")
    as32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return {"perm": as32(perm), "step": as32(step), "left": as32(left), "w0": as32(w0), "w1": as32(w1), "step_rows": as32(step_rows),
            "step_offsets": as32(step_offsets), "status": as32([int((~ok).sum()), duplicates]), "depth": depth, "keys": key}


def _pairs(p, s):
    rows = p["step_rows"][p["step_offsets"][s]:p["step_offsets"][s + 1]].astype(np.int64)
    l = p["left"][rows].astype(np.int64)
    s0 = np.sqrt(p["w0"][rows].astype(np.float64))[:, None]
    s1 = np.sqrt(p["w1"][rows].astype(np.float64))[:, None]
    sn = np.sqrt(p["w0"][rows].astype(np.float64) + p["w1"][rows].astype(np.float64))[:, None]
    return rows, l, s0, s1, sn


def forward(p, attrs):
    """attrs [N,C] in input order -> float64 [N,C] coefficients in Morton row order"""
    v = np.asarray(attrs, dtype=np.float64)[p["perm"]].copy()
    for s in range(3 * p["depth"]):
        r, l, s0, s1, sn = _pairs(p, s)
        a0, a1 = v[l], v[r]
        v[l] = (s0 * a0 + s1 * a1) / sn
        v[r] = (s0 * a1 - s1 * a0) / sn
    return v


def inverse(p, coeffs):
    """coefficients in Morton row order -> attributes in Morton row order"""
    v = np.asarray(coeffs, dtype=np.float64).copy()
    for s in reversed(range(3 * p["depth"])):
        r, l, s0, s1, sn = _pairs(p, s)
        low, high = v[l], v[r]
        v[l] = (s0 * low - s1 * high) / sn
        v[r] = (s1 * low + s0 * high) / sn
    return v


def recursive(keys, attrs, bits):
    """The definition: sorted keys [n], their attributes [n,C] (float64), ``bits`` key bits still undecided -> (dc [C], weight,
    [(row, coefficient [C]), ...]), rows counted from the first of ``keys``.  A node whose rows all lie in one child passes up
    unchanged; otherwise the children's DCs merge and the high-pass coefficient belongs to the first row of the right child."""
    if len(keys) == 1:
        return attrs[0].astype(np.float64), 1, []
    top = bits - 1
    bit = (keys >> np.uint64(top)) & np.uint64(1)
    if bit.min() == bit.max():
        return recursive(keys, attrs, top)
    n0 = int((bit == 0).sum())
    d0, w0, h0 = recursive(keys[:n0], attrs[:n0], top)
    d1, w1, h1 = recursive(keys[n0:], attrs[n0:], top)
    low = (np.sqrt(float(w0)) * d0 + np.sqrt(float(w1)) * d1) / np.sqrt(float(w0) + float(w1))
    high = (np.sqrt(float(w0)) * d1 - np.sqrt(float(w1)) * d0) / np.sqrt(float(w0) + float(w1))
    return low, w0 + w1, h0 + [(r + n0, c) for r, c in h1] + [(n0, high)]


def forward_recursive(p, attrs):
    """the coefficients of ``forward`` by the recursive definition"""
    a = np.asarray(attrs, dtype=np.float64)[p["perm"]]
    dc, weight, high = recursive(p["keys"], a, 3 * p["depth"])
    assert weight == a.shape[0] and len(high) == a.shape[0] - 1
    out = np.full(a.shape, np.nan)
    out[0] = dc
    for r, c in high:
        out[r] = c
    return out


def quantize(coeffs, qstep):
    return np.rint(np.asarray(coeffs, dtype=np.float64) / np.float64(qstep)).astype(np.int64)


def near_rounding_boundary(coeffs, qstep, tol):
    """coefficients whose quotient lies within tol / qstep of a half-integer: a GPU coefficient that differs by up to ``tol`` may
    round to the other side"""
    q = np.asarray(coeffs, dtype=np.float64) / np.float64(qstep)
    return np.abs(np.abs(q - np.floor(q)) - 0.5) <= tol / qstep


def bypass_bits(raw):
    """the coder's escape (compressai's bypass): the remainder in 4-bit nibbles, their count in 4-bit groups of up to 15"""
    nibbles = 0
    while raw >> (4 * nibbles):
        nibbles += 1
    return 4 * nibbles + 4 * (nibbles // 15 + 1)


def choose_tables(symbols, contexts, n_contexts, cdf, cdf_len, offset):
    """per context the table with the smallest ideal code length (units of 2^-20 bit, integers; ties to the lowest index),
    0 for an empty context: the rule of pcc_amd.raht, symbol by symbol"""
    scale = 1 << 20
    n_tables = cdf.shape[0]
    out = np.zeros(n_contexts, dtype=np.uint8)
    for ctx in range(n_contexts):
        values, counts = np.unique(np.asarray(symbols)[np.asarray(contexts) == ctx], return_counts=True)
        if values.size == 0:
            continue
        best, best_cost = 0, None
        for t in range(n_tables):
            maxv = int(cdf_len[t]) - 2
            cost = 0
            for v, k in zip(values.tolist(), counts.tolist()):
                x = v - int(offset[t])
                extra = 0
                if x < 0:
                    extra, x = bypass_bits(-2 * x - 1), maxv
                elif x >= maxv:
                    extra, x = bypass_bits(2 * (x - maxv)), maxv
                freq = int(cdf[t, x + 1]) - int(cdf[t, x])
                cost += k * (int(np.rint((16.0 - np.log2(np.float64(freq))) * scale)) + extra * scale)
            if best_cost is None or cost < best_cost:
                best, best_cost = t, cost
        out[ctx] = best
    return out


# ---- the clouds of tests/test_raht.py and tests/test_anchor.py ---------------------------------------------------------------
def sphere_shell32():
    g = np.stack(np.meshgrid(*[np.arange(32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r = np.linalg.norm(g - 15.5, axis=1)
    return g[np.abs(r - 12.0) < 0.7]


def random_voxels(n, depth, seed, origin=(0, 0, 0)):
    """n distinct voxels of a 2^depth grid, in a random order, shifted by ``origin``"""
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(0, 1 << depth, size=(2 * n + 64, 3)), axis=0)
    assert c.shape[0] >= n
    c = c[rng.permutation(c.shape[0])[:n]]
    return c + np.asarray(origin, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (coords int64 [N,3] in a shuffled order, origin or None, depth or None)"""
    cube = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    dense = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    shell = sphere_shell32()
    shell = shell[np.random.default_rng(5).permutation(shell.shape[0])]
    return {
        "one": (np.array([[3, 4, 5]]), None, None),
        "one_deep": (np.array([[3, 4, 5]]), (0, 0, 0), 3),
        "siblings": (np.array([[6, 2, 5], [6, 2, 4]]), (0, 0, 0), 3),
        "meet_at_top": (np.array([[7, 0, 3], [0, 5, 1]]), (0, 0, 0), 3),
        "cube": (cube[np.random.default_rng(1).permutation(8)], None, None),
        "random92": (random_voxels(92, 3, 2), (0, 0, 0), 3),
        "shell32": (shell, None, None),
        "random4000": (random_voxels(4000, 10, 3), None, None),
        "deep300": (random_voxels(300, 17, 4, origin=(-70000, -65000, -130000)), (-70000, -65000, -130000), 17),
        # the top steps of at most 256 rows share one launch: a first step of exactly 256 rows, and one of 257
        "dense512": (dense[np.random.default_rng(7).permutation(512)], None, None),
        "dense514": (np.concatenate([dense, [[12, 2, 6], [12, 2, 7]]])[np.random.default_rng(8).permutation(514)], None, None),
    }


def attributes(n, c, seed):
    return np.random.default_rng(seed).random((n, c))


def smooth_colours(coords, grid=32.0):
    """rgb in [0, 1] that varies slowly over the grid (what RAHT compacts)"""
    p = np.asarray(coords, dtype=np.float64)
    phase = np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3])
    return 0.5 + 0.4 * np.sin(2 * np.pi * p[:, :1] / grid * np.array([1.0, 2.0, 1.5]) + 2 * np.pi * p[:, 1:2] / grid
                              + np.pi * p[:, 2:3] / grid + phase)


# ---- the anchor codec's cases (tests/test_anchor.py; their rounding margins are checked on the CPU in test_raht_reference.py) --
RGB_TO_YUV = np.array([[0.2126, 0.7152, 0.0722], [-0.1146, -0.3854, 0.5], [0.5, -0.4542, -0.0458]], dtype=np.float64)


def coded_reference(x, colorspace):
    """the colours of a cloud x [N,6] float32 in the coded colour space, float64: BT.709 without truncation or offsets, each
    row (m0 * r + m1 * g) + m2 * b"""
    c = np.asarray(x)[:, 3:6].astype(np.float64)
    if colorspace == "rgb":
        return c
    m = RGB_TO_YUV
    return np.stack([(m[r, 0] * c[:, 0] + m[r, 1] * c[:, 1]) + m[r, 2] * c[:, 2] for r in range(3)], axis=1)


@functools.lru_cache(maxsize=None)
def anchor_cases():
    """name -> (x float32 [N,6] with rows shuffled, qstep, colorspace)"""
    shell = sphere_shell32() + np.array([100, -20, 7])
    shell = shell[np.random.default_rng(6).permutation(shell.shape[0])]
    smooth = np.round(smooth_colours(shell - np.array([100, -20, 7])) * 255.0) / 255.0
    rnd = random_voxels(4000, 10, 3)
    one = np.array([[4.0, 9.0, 2.0, 0.25, 0.5, 1.0]])
    cloud = lambda c, a: np.concatenate([c, a], axis=1).astype(np.float32)
    return {
        "shell_yuv": (cloud(shell, smooth), 4 / 255, "yuv"),
        "shell_rgb_fine": (cloud(shell, smooth), 1 / 255, "rgb"),
        "random_rgb": (cloud(rnd, attributes(4000, 3, 8)), 16 / 255, "rgb"),
        "random_yuv": (cloud(rnd, attributes(4000, 3, 9)), 2 / 255, "yuv"),
        "one": (cloud(one[:, :3], one[:, 3:]), 8 / 255, "yuv"),
    }


def anchor_reference(name):
    """-> (plan, coded attributes in input order, coefficients, tolerance of a GPU coefficient, symbols)"""
    x, qstep, space = anchor_cases()[name]
    p = plan(np.round(x[:, :3]).astype(np.int64))
    a = coded_reference(x, space)
    co = forward(p, a)
    tol = 1e-12 * np.abs(a).max() * np.sqrt(x.shape[0])
    return p, a, co, tol, quantize(co, qstep)
