"""numpy restatement of pcc_voxelize (include/pcc_hip.h) and the inputs its GPU tests share.

Cell: float32 operations in the stated order, ``np.floor((p - o) / v)`` or ``np.rint`` of the same quotient, every operation
rounded separately (numpy's float32 division is correctly rounded).  Order: a first-appearance dictionary over (batch, cell).
Sums: each attribute once to Q32 fixed point, ``np.rint(float64(a) * 2**32)`` as int64 (the product is exact in float64 — a
24-bit significand times a power of two — so the only rounding is the one to an integer, ties to even, which is llrint's), added
with ``np.add.at`` on int64.  The kernel must EQUAL all of it.
"""
import numpy as np

COORD_LIMIT = 130000
BATCH_LIMIT = 1022
COUNT_ERR_RANGE = -2
ERR_ARG = -1
Q32 = 4294967296.0
FLOOR, NEAREST = 0, 1


def to_q32(a):
    """float32 attributes -> int64 Q32 fixed point, ties to even"""
    a = np.asarray(a, dtype=np.float32)
    return np.rint(a.astype(np.float64) * Q32).astype(np.int64)


def mean_of(sums, npts):
    """the Python layer's mean: float32(float64(sum) / float64(npts) / 2**32)"""
    return (sums.astype(np.float64) / npts.astype(np.float64)[:, None] / Q32).astype(np.float32)


def cells_of(xyz, origin, voxel, rounding):
    """float32 [n,3] of rounded quotients (not yet integers: they may be non-finite or out of range)"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    o = np.asarray(origin, dtype=np.float32).reshape(3)
    v = np.float32(voxel)
    with np.errstate(all="ignore"):
        g = ((xyz - o[None, :]).astype(np.float32) / v).astype(np.float32)
        assert g.dtype == np.float32
        return np.rint(g) if rounding == NEAREST else np.floor(g)


def voxelize_reference(xyz, batch=None, nbatch=1, attr=None, origin=(0, 0, 0), voxel=1.0, rounding=FLOOR):
    """-> dict(coords int32 [m,4], first int32 [m], npts int32 [m], sum int64 [m,c], row int32 [n]), or COUNT_ERR_RANGE, or
    ERR_ARG for the arguments the host refuses"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    c = 0 if attr is None else np.asarray(attr).shape[1]
    attr = np.zeros((n, 0), np.float32) if attr is None else np.asarray(attr, dtype=np.float32).reshape(n, c)
    v = np.float32(voxel)
    if not (v > 0) or not np.isfinite(v) or not 0 <= c <= 16 or rounding not in (FLOOR, NEAREST) or not 1 <= nbatch <= BATCH_LIMIT + 1:
        return ERR_ARG
    b = np.zeros(n, np.int32) if batch is None else np.asarray(batch, dtype=np.int32).reshape(n)
    f = cells_of(xyz, origin, voxel, rounding)
    with np.errstate(all="ignore"):
        bad = (~np.isfinite(f)).any() or (np.abs(f) > COORD_LIMIT).any() or (b < 0).any() or (b >= nbatch).any()
        bad = bad or (~np.isfinite(attr)).any() or (np.abs(attr) > 1).any()
    if bad:
        return COUNT_ERR_RANGE
    cells = np.concatenate([b[:, None], f.astype(np.int32)], axis=1).astype(np.int32)
    seen, first, row = {}, [], np.empty(n, np.int32)
    for i, key in enumerate(map(tuple, cells.tolist())):
        r = seen.get(key)
        if r is None:
            r = seen[key] = len(first)
            first.append(i)
        row[i] = r
    first = np.asarray(first, dtype=np.int32)
    m = first.shape[0]
    npts = np.zeros(m, np.int32)
    np.add.at(npts, row, 1)
    sums = np.zeros((m, c), np.int64)
    np.add.at(sums, row, to_q32(attr))
    return {"coords": cells[first].reshape(m, 4), "first": first, "npts": npts, "sum": sums, "row": row}


def colours(n, seed=0, c=3):
    """float32 [n,c] of k/255, k uniform in 0..255"""
    return (np.random.default_rng(seed).integers(0, 256, (n, c)).astype(np.float32) / np.float32(255.0)).astype(np.float32)
