"""The numpy restatement of the position scaling (tests/_scaled_reference.py) against Fraction arithmetic and a plain Python loop,
its shell walk against brute force, the conditions the GPU tests rely on, the optimality of the "nearest" colouring, and the
host-side checks of pcc_scaled_cells / pcc_scaled_transfer, rescale.as_scale and the PCA2 header (no GPU needed)."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import _scaled_reference as ref
from _voxelize_reference import ERR_ARG


def test_formulas_equal_fraction_arithmetic(pcc):
    from pcc_amd import rescale
    p = np.arange(-300, 301)
    for num, den in ref.SCALES + ((2, 3), (31, 32), (1, 255), (254, 255)):
        s = Fraction(num, den)
        cell = [math.floor(int(v) * s + Fraction(1, 2)) for v in p]             # p s rounded to nearest, halves up
        pos = [math.floor(int(v) / s + Fraction(1, 2)) for v in p]              # c / s rounded to nearest, halves up
        assert ref.cells_of(p, num, den).tolist() == cell and ref.positions_of(p, num, den).tolist() == pos
        assert all(b > a for a, b in zip(pos, pos[1:]))                         # strictly increasing
        assert ref.cells_of(pos, num, den).tolist() == p.tolist()               # cell(pos(c)) = c
        assert all(b >= a for a, b in zip(cell, cell[1:]))
        # the package's formulas on arrays and tensors, in the dtype given
        for dtype in (np.int32, np.int64):
            assert rescale.cells_of(p.astype(dtype), num, den).tolist() == cell
            assert rescale.positions_of(p.astype(dtype), num, den).dtype == dtype
        t = torch.from_numpy(p.astype(np.int32))
        assert rescale.cells_of(t, num, den).tolist() == cell and rescale.positions_of(t, num, den).tolist() == pos
        assert rescale.positions_of(t, num, den).dtype == torch.int32
    with pytest.raises(ValueError):
        rescale.cells_of(np.zeros(3, np.float32), 1, 2)


def loop_reference(coords, attr, num, den):
    """one point at a time, Python integers throughout"""
    s = Fraction(num, den)
    seen, cells, first, row = {}, [], [], []
    for i, (b, *p) in enumerate(coords):
        key = (b,) + tuple(math.floor(v * s + Fraction(1, 2)) for v in p)
        if key not in seen:
            seen[key] = len(cells)
            cells.append(key)
            first.append(i)
        row.append(seen[key])
    positions = [tuple(math.floor(v / s + Fraction(1, 2)) for v in key[1:]) for key in cells]
    nearest, d2 = [], []
    for b, *p in coords:
        best = None
        for r, key in enumerate(cells):
            if key[0] != b:
                continue
            d = sum((positions[r][a] - p[a]) ** 2 for a in range(3))
            cand = (d, positions[r], r)
            if best is None or cand[:2] < best[:2]:
                best = cand
        nearest.append(best[2])
        d2.append(best[0])
    counts = [0] * len(cells)
    sums = [[0] * attr.shape[1] for _ in cells]
    for i, r in enumerate(nearest):
        counts[r] += 1
        for ch in range(attr.shape[1]):
            sums[r][ch] += round(float(attr[i][ch]) * 4294967296.0)
    for r in range(len(cells)):
        if counts[r] == 0:
            best = None
            for i, (b, *p) in enumerate(coords):
                if b == cells[r][0]:
                    cand = (sum((positions[r][a] - p[a]) ** 2 for a in range(3)), tuple(p), i)
                    if best is None or cand < best:
                        best = cand
            sums[r] = [round(float(attr[best[2]][ch]) * 4294967296.0) for ch in range(attr.shape[1])]
    return cells, positions, first, row, nearest, d2, counts, sums


def test_restatement_equals_a_plain_loop():
    rng = np.random.default_rng(2)
    for num, den in ((1, 2), (3, 4), (5, 7), (1, 8)):
        xyz = np.unique(rng.integers(-9, 10, (520, 3)), axis=0)
        xyz = xyz[rng.permutation(len(xyz))[:400]]
        coords = np.concatenate([rng.integers(0, 2, (400, 1)), xyz], axis=1)
        attr = ref.colours(400, 2, 7)
        got = ref.quantize_reference(coords, attr, num, den)
        cells, positions, first, row, nearest, d2, counts, sums = loop_reference(coords.tolist(), attr, num, den)
        assert got["cells"].tolist() == [list(c) for c in cells] and got["positions"].tolist() == [list(p) for p in positions]
        assert got["first"].tolist() == first and got["row"].tolist() == row
        assert got["nearest"].tolist() == nearest and got["d2"].tolist() == d2
        assert got["counts"].tolist() == counts and got["sums"].tolist() == sums
        assert int(got["own_npts"].sum()) == 400 and int(got["counts"].sum()) == 400 and got["sums"].dtype == np.int64


@pytest.mark.parametrize("scale", ref.SCALES)
def test_shell_walk_equals_brute_force_and_case_conditions(scale):
    num, den = scale
    p = ref.shell()
    assert 2000 < len(p) <= 3000 and p.min() < -20 and p.max() - p.min() < 72
    want = ref.shell_reference(num, den)
    nearest, d2, deepest = ref.shell_walk(ref.with_batch(p), want["cells"], num, den)
    assert np.array_equal(nearest, want["nearest"]) and np.array_equal(d2, want["d2"])
    ties, moved, empty = int((want["ties"] > 1).sum()), int((want["nearest"] != want["row"]).sum()), int(want["empty"].size)
    print(f"scale {num}/{den}: {len(p)} points, {len(want['cells'])} cells, deepest shell {deepest}, {ties} points with a tie, "
          f"{moved} whose nearest cell is not their own, {empty} cells no point chose")
    assert deepest <= 1
    if num < den:
        assert ties >= 1 and moved >= 1 and empty >= 1
    else:
        assert ties == 0 and moved == 0 and empty == 0 and not want["d2"].any()


def test_no_scale_sends_the_walk_into_shell_two():
    """The search for a cloud whose walk must enter shell 2, made complete.  A point's own cell is occupied, so after shell 0
    best <= D0 = the squared distance to its own position, and shell k is entered iff best >= L(k).  cell and pos are periodic
    (cell(p + den) = cell(p) + num, pos(c + num) = pos(c) + den), so per axis the offset o(p) = (pos(cell(p)) - p)^2 and the
    bound term l_k(p) take their values on the residues p = 0 .. den - 1.  With L(k) attained on some axis at residue p, D0 <=
    o(p) + 2 max o.  For EVERY scale 1 <= num <= den <= 255 and every residue, o(p) + 2 max o < l_2(p): a one-point cloud, the
    cloud with the largest best, never reaches shell 2, so no cloud does."""
    entered = []
    for den in range(1, 256):
        p = np.arange(den, dtype=np.int64)
        for num in range(1, den + 1):
            c0 = ref.cells_of(p, num, den)
            o = (ref.positions_of(c0, num, den) - p) ** 2
            l2 = np.minimum((ref.positions_of(c0 + 2, num, den) - p) ** 2, (p - ref.positions_of(c0 - 2, num, den)) ** 2)
            if (o + 2 * o.max() >= l2).any():
                entered.append((num, den))
    assert entered == []


def test_nearest_colouring_is_optimal():
    """the squared attribute error summed over the points against the colour of their nearest cell: no larger with "nearest"
    features than with "cell" features"""
    p = ref.shell()
    attr = ref.colours(len(p), 3, 11).astype(np.float64)
    for num, den in ref.SCALES:
        want = ref.shell_reference(num, den)
        err = lambda f: float(((attr - f.astype(np.float64)[want["nearest"]]) ** 2).sum())
        e_near, e_cell = err(want["features"]), err(want["own_features"])
        print(f"scale {num}/{den}: A->B squared colour error {e_near:.6f} with nearest features, {e_cell:.6f} with cell features")
        assert e_near <= e_cell * (1 + 1e-12)
        if num == den:
            assert np.array_equal(want["features"], want["own_features"])


def test_as_scale(pcc):
    from pcc_amd.rescale import as_scale
    assert as_scale((1, 8)) == (1, 8) and as_scale([3, 4]) == (3, 4) and as_scale((2, 4)) == (1, 2) and as_scale((255, 255)) == (1, 1)
    assert as_scale(Fraction(5, 7)) == (5, 7) and as_scale(Fraction(10, 14)) == (5, 7)
    assert [as_scale(f) for f in (0.125, 0.25, 0.5, 0.75, 1.0, 1)] == [(1, 8), (1, 4), (1, 2), (3, 4), (1, 1), (1, 1)]
    assert as_scale(np.float32(0.375)) == (3, 8)
    for bad in (0.3, 0.0, -0.5, 1.5, 2, float("nan"), float("inf"), 1 / 256, (0, 4), (5, 4), (1, 256), (1, 2, 3), (0.5, 1), (1,),
                Fraction(3, 2), Fraction(1, 256), Fraction(0), "1/2", None, True):
        with pytest.raises(ValueError):
            as_scale(bad)


def test_bad_pca2_headers(pcc):
    """refused before the device is touched"""
    from pcc_amd import anchor
    assert anchor.MAGIC_SCALED == b"PCA2"
    body = b"\0" * 40
    head = lambda space, num, den, zero, glen: b"PCA2" + struct.pack("<BBBBI", space, num, den, zero, glen)
    for bad in (head(1, 0, 4, 0, 40) + body,          # num = 0
                head(1, 5, 4, 0, 40) + body,          # num > den
                head(1, 0, 0, 0, 40) + body,
                head(1, 1, 4, 1, 40) + body,          # the reserved byte
                head(7, 1, 4, 0, 40) + body,          # no such colour space
                head(1, 1, 4, 0, 41) + body,          # truncated geometry
                head(1, 1, 4, 0, 40)[:11],            # truncated header
                b"PCA3" + head(1, 1, 4, 0, 40)[4:] + body):
        with pytest.raises(ValueError):
            anchor.decompress(bad, "cpu")
    assert anchor.qp_to_qstep(4) == 1 / 255 and anchor.qp_to_qstep(40) == 64 / 255
    assert anchor.GPCC_POINTS == ((0.125, 51), (0.25, 46), (0.5, 40), (0.75, 34))


def test_host_argument_checks_without_gpu(pcc):
    """refused on the host before any launch: the pointers are never dereferenced"""
    L = pcc.lib()
    n, cap = 1000, L.pcc_hash_capacity(1000)
    P = 4096                                               # a non-null pointer value nothing reads

    def cells(num=1, den=2, c=3, cap=cap, n=n, coords=P, attr=P, keys=P, vals=P, scratch=P, out=P, first=P, npts=P, sums=P, row=P,
              count=P):
        return L.pcc_scaled_cells(coords, n, attr, c, num, den, keys, vals, cap, scratch, out, first, npts, sums, row, count, None)

    def transfer(num=1, den=2, c=3, cap=cap, n=n, m=10, coords=P, attr=P, keys=P, vals=P, nearest=P, d2=P, npts=P, sums=P):
        return L.pcc_scaled_transfer(coords, n, attr, c, num, den, keys, vals, cap, m, nearest, d2, npts, sums, None)

    scale = [({"num": 0}, b"scale"), ({"num": 3, "den": 2}, b"scale"), ({"den": 256, "num": 1}, b"scale"), ({"num": -1}, b"scale"),
             ({"den": 0, "num": 0}, b"scale"), ({"c": 17}, b"channels"), ({"c": -1}, b"channels"), ({"n": -1}, b"count")]
    for kw, word in scale + [({"cap": 1024}, b"capacity"), ({"cap": cap + 1}, b"capacity"), ({"cap": 0}, b"capacity"),
                             ({"keys": None}, b"null"), ({"vals": None}, b"null"), ({"scratch": None}, b"null"),
                             ({"count": None}, b"null"), ({"coords": None}, b"null"), ({"out": None}, b"null"),
                             ({"first": None}, b"null"), ({"npts": None}, b"null"), ({"row": None}, b"null"),
                             ({"attr": None}, b"null"), ({"sums": None}, b"null")]:
        assert cells(**kw) == ERR_ARG, kw
        assert word in L.pcc_last_error(), (kw, L.pcc_last_error())
    for kw, word in scale + [({"cap": cap + 1}, b"capacity"), ({"cap": 0}, b"capacity"), ({"m": -1}, b"rows"), ({"m": n + 1}, b"rows"),
                             ({"m": 0}, b"null"), ({"keys": None}, b"null"), ({"vals": None}, b"null"), ({"coords": None}, b"null"),
                             ({"nearest": None}, b"null"), ({"d2": None}, b"null"), ({"npts": None}, b"null"),
                             ({"attr": None}, b"null"), ({"sums": None}, b"null")]:
        assert transfer(**kw) == ERR_ARG, kw
        assert word in L.pcc_last_error(), (kw, L.pcc_last_error())
