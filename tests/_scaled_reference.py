"""numpy restatement of the position scaling (include/pcc_hip.h: pcc_scaled_cells, pcc_scaled_transfer; pcc_amd/rescale.py) and
the inputs its tests share.

Formulas: Python / int64 integers with floor division.  Cells: a first-appearance dictionary over (batch, cell).  Nearest: a
chunked brute-force search over ALL cells' positions with the tie rule (smallest (x, y, z), same batch item only).  Sums: each
attribute once to Q32 fixed point (tests/_voxelize_reference.py: to_q32), added with ``np.add.at`` on int64.  ``shell_walk``
restates the kernel's walk with its bound, one point at a time, and reports the deepest shell it scanned.  The kernels and the
Python layer must EQUAL all of it.
"""
import functools

import numpy as np

from _voxelize_reference import Q32, to_q32

SCALES = ((1, 8), (1, 4), (1, 2), (3, 4), (5, 7), (15, 16), (1, 1))
FAR = np.iinfo(np.int64).max


def cells_of(p, num, den):
    return (2 * np.asarray(p, dtype=np.int64) * num + den) // (2 * den)


def positions_of(c, num, den):
    return (2 * np.asarray(c, dtype=np.int64) * den + num) // (2 * num)


def first_appearance(cells):
    """cells int [n,4] -> (distinct rows in order of first appearance [m,4], first [m], npts [m], row [n])"""
    seen, first, row = {}, [], np.empty(len(cells), np.int32)
    for i, key in enumerate(map(tuple, np.asarray(cells).tolist())):
        r = seen.get(key)
        if r is None:
            r = seen[key] = len(first)
            first.append(i)
        row[i] = r
    first = np.asarray(first, dtype=np.int32)
    npts = np.zeros(first.shape[0], np.int32)
    np.add.at(npts, row, 1)
    return np.asarray(cells)[first].reshape(-1, 4).astype(np.int32), first, npts, row


def lex_rank(rows):
    """rank of every row [m,4] in the lexicographic order of (batch, x, y, z); equal rows get the rank of the lowest index"""
    rows = np.asarray(rows, dtype=np.int64)
    order = np.lexsort((np.arange(len(rows)), rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))
    rank = np.empty(len(rows), np.int64)
    rank[order] = np.arange(len(rows))
    return rank


def brute_nearest(queries, targets, chunk=512):
    """queries [n,4], targets [m,4] (batch, x, y, z) -> (index of the nearest target of the same batch item [n], squared distance
    [n], number of equidistant nearest targets [n]); ties to the smallest (x, y, z), then the lowest row"""
    q, t = np.asarray(queries, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    rank = lex_rank(t)
    idx, d2, ties = np.empty(len(q), np.int32), np.empty(len(q), np.int64), np.empty(len(q), np.int32)
    for a in range(0, len(q), chunk):
        part = q[a:a + chunk]
        d = ((part[:, None, 1:] - t[None, :, 1:]) ** 2).sum(axis=2)
        d = np.where(part[:, None, 0] == t[None, :, 0], d, FAR)
        best = d.min(axis=1)
        assert (best < FAR).all(), "a query without a target in its batch item"
        tied = d == best[:, None]
        idx[a:a + chunk] = np.where(tied, rank[None, :], FAR).argmin(axis=1)
        d2[a:a + chunk] = best
        ties[a:a + chunk] = tied.sum(axis=1)
    return idx, d2, ties


def shell_walk(points, cells, num, den):
    """the kernel's walk, one point at a time: shells k = 0, 1, 2 ... of Chebyshev radius k in the cell domain around cell(p),
    true distances to pos(c), stop before shell k once best < L(k) -> (nearest [n], d2 [n], deepest shell scanned)"""
    table = {tuple(c): r for r, c in enumerate(np.asarray(cells).tolist())}
    pos = lambda c: (2 * c * den + num) // (2 * num)
    nearest, d2s, deepest = np.empty(len(points), np.int32), np.empty(len(points), np.int64), 0
    for i, (b, *p) in enumerate(np.asarray(points).tolist()):
        c0 = [(2 * v * num + den) // (2 * den) for v in p]
        best, best_key, best_row, k = None, None, -1, 0
        while True:
            if k > 0:
                bound = min(min((pos(c0[a] + k) - p[a]) ** 2, (p[a] - pos(c0[a] - k)) ** 2) for a in range(3))
                if best < bound:
                    break
            deepest = max(deepest, k)
            for dx in range(-k, k + 1):
                for dy in range(-k, k + 1):
                    for dz in range(-k, k + 1):
                        if max(abs(dx), abs(dy), abs(dz)) != k:
                            continue
                        key = (b, c0[0] + dx, c0[1] + dy, c0[2] + dz)
                        r = table.get(key)
                        if r is None:
                            continue
                        d = sum((pos(key[1 + a]) - p[a]) ** 2 for a in range(3))
                        if best is None or d < best or (d == best and key < best_key):
                            best, best_key, best_row = d, key, r
            assert best is not None, "the point's own cell is not in the set"
            k += 1
        nearest[i], d2s[i] = best_row, best
    return nearest, d2s, deepest


def mean_of(sums, counts):
    """float32(float64(sum) / float64(max(count, 1)) / 2**32)"""
    return (sums.astype(np.float64) / np.maximum(counts, 1).astype(np.float64)[:, None] / Q32).astype(np.float32)


def quantize_reference(coords, attr, num, den):
    """coords int [n,4], attr float32 [n,c] -> dict: cells, positions, first, row, own_npts, own_sums, own_features ("cell"),
    nearest, d2, ties, counts, sums, features ("nearest", after the empty-cell rule), empty (the rows no point chose)"""
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    n = coords.shape[0]
    attr = np.zeros((n, 0), np.float32) if attr is None else np.asarray(attr, dtype=np.float32).reshape(n, -1)
    c = attr.shape[1]
    own = np.concatenate([coords[:, :1], cells_of(coords[:, 1:], num, den)], axis=1)
    cells, first, own_npts, row = first_appearance(own)
    m = cells.shape[0]
    q = to_q32(attr)
    own_sums = np.zeros((m, c), np.int64)
    np.add.at(own_sums, row, q)
    positions = positions_of(cells[:, 1:], num, den)
    recon = np.concatenate([cells[:, :1].astype(np.int64), positions], axis=1)
    nearest, d2, ties = brute_nearest(coords, recon)
    counts = np.zeros(m, np.int32)
    np.add.at(counts, nearest, 1)
    sums = np.zeros((m, c), np.int64)
    np.add.at(sums, nearest, q)
    empty = np.flatnonzero(counts == 0)
    if empty.size:
        back, _, _ = brute_nearest(recon[empty], coords)
        sums[empty] = q[back]
    return {"cells": cells, "positions": positions.astype(np.int32), "first": first, "row": row, "own_npts": own_npts,
            "own_sums": own_sums, "own_features": mean_of(own_sums, own_npts), "nearest": nearest, "d2": d2, "ties": ties,
            "counts": counts, "sums": sums, "features": mean_of(sums, counts), "empty": empty}


def morton_order(xyz):
    """the permutation that sorts integer points [n,3] by the Morton key of (p - min)"""
    v = np.asarray(xyz, dtype=np.int64)
    v = v - v.min(axis=0)
    key = np.zeros(len(v), np.int64)
    for bit in range(20):
        for a in range(3):
            key |= ((v[:, a] >> bit) & 1) << (3 * bit + (2 - a))
    return np.argsort(key, kind="stable")


@functools.lru_cache(maxsize=None)
def shell(seed=3, n=3000):
    """a noisy sphere shell of distinct integer points with negative coordinates in a box of about 64^3, in a shuffled order:
    int64 [N,3], N <= n"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.rint(d * (24.0 + rng.normal(size=(n, 1))) + np.array([-5.0, 3.0, -12.0])).astype(np.int64)
    p = np.unique(p, axis=0)
    p = p[rng.permutation(len(p))]
    p.setflags(write=False)
    return p


def colours(n, c, seed):
    """float32 [n,c] of k/255"""
    return (np.random.default_rng(seed).integers(0, 256, (n, c)).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def with_batch(xyz, b=0):
    xyz = np.asarray(xyz, dtype=np.int64)
    return np.concatenate([np.full((len(xyz), 1), b, np.int64), xyz], axis=1)


@functools.lru_cache(maxsize=None)
def shell_reference(num, den, c=3, seed=3):
    """the restatement on the whole shell with c colour channels (computed once per scale, shared by the tests; read only)"""
    p = shell(seed)
    return quantize_reference(with_batch(p), colours(len(p), c, 11), num, den)


def one_cell_points(count=300, cell=(-3, 2, 1), seed=4):
    """``count`` distinct points that all fall into one cell at scale 1/8 (cell(p) = floor((p + 4) / 8): 8 c - 4 .. 8 c + 3)"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(-4, 4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return g[rng.permutation(512)[:count]] + 8 * np.asarray(cell, dtype=np.int64)
