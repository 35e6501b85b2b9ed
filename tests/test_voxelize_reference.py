"""The numpy restatement of pcc_voxelize (tests/_voxelize_reference.py) against a plain Python loop, the Q32 facts the contract
relies on, the figures the GPU tests quote, and the host-side argument checks of the entry point (no GPU needed)."""
import math

import numpy as np

import _augment_reference as aug
import _voxelize_reference as ref


def loop_reference(xyz, batch, attr, origin, voxel, rounding):
    """one point at a time, Python ints for the sums and np.float32 scalars for the cell"""
    seen, coords, first, npts, sums, row = {}, [], [], [], [], []
    v = np.float32(voxel)
    for i in range(len(xyz)):
        cell = [int(batch[i])]
        for ax in range(3):
            g = np.float32(np.float32(xyz[i][ax]) - np.float32(origin[ax])) / v
            assert type(g) is np.float32
            cell.append(int(np.rint(g)) if rounding else math.floor(g))
        key = tuple(cell)
        if key not in seen:
            seen[key] = len(coords)
            coords.append(cell)
            first.append(i)
            npts.append(0)
            sums.append([0] * attr.shape[1])
        r = seen[key]
        row.append(r)
        npts[r] += 1
        for ch in range(attr.shape[1]):
            x = float(attr[i][ch]) * 4294967296.0
            q = round(x)                                   # Python's round: ties to even, exact on floats
            sums[r][ch] += q
    return coords, first, npts, sums, row


def test_restatement_equals_a_plain_loop():
    rng = np.random.default_rng(5)
    for rounding, voxel, origin in ((0, 0.75, (0, 0, 0)), (1, 0.5, (0.25, -1, 3)), (0, 2, (-7, 0, 0.5))):
        xyz = (rng.random((400, 3), dtype=np.float32) * 4 - 2).astype(np.float32)
        xyz[::7] = np.rint(xyz[::7])                                   # some exact grid points and .5 ties
        xyz[1::7] = np.rint(xyz[1::7]) + np.float32(0.5)
        batch = rng.integers(0, 3, 400).astype(np.int32)
        attr = rng.random((400, 2), dtype=np.float32) * 2 - 1
        got = ref.voxelize_reference(xyz, batch, 3, attr, origin, voxel, rounding)
        coords, first, npts, sums, row = loop_reference(xyz, batch, attr, origin, voxel, rounding)
        assert len(coords) < 400
        assert got["coords"].tolist() == coords and got["first"].tolist() == first and got["npts"].tolist() == npts
        assert got["sum"].tolist() == sums and got["row"].tolist() == row
        assert got["sum"].dtype == np.int64 and got["coords"].dtype == np.int32 and int(got["npts"].sum()) == 400


def test_q32_facts():
    k = np.arange(256)
    a = (k.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    q = ref.to_q32(a)
    assert np.array_equal(q.astype(np.float64) / ref.Q32, a.astype(np.float64))         # every k/255 is exact
    assert ref.to_q32(np.float32(2.0 ** -33)) == 0                                      # a tie: to even
    assert ref.to_q32(np.float32(3 * 2.0 ** -33)) == 2                                  # a tie: to even
    assert ref.to_q32(np.float32(2.0 ** -9 + 2.0 ** -33)) == 2 ** 23                    # 2^23 + 0.5: to even
    assert ref.to_q32(np.float32(1.0)) == 2 ** 32 and ref.to_q32(np.float32(-1.0)) == -2 ** 32
    # a value of at least 2^-8 has an ulp of at least 2^-32: exact; below, the error is at most 2^-33
    rng = np.random.default_rng(0)
    x = rng.random(10000, dtype=np.float32)
    err = np.abs(ref.to_q32(x).astype(np.float64) / ref.Q32 - x.astype(np.float64))
    assert err[x >= 2.0 ** -8].max() == 0 and err.max() <= 2.0 ** -33
    # 2^31 - 1 points of |a| = 1 stay below 2^63
    assert (2 ** 31 - 1) * 2 ** 32 < 2 ** 63
    # the mean of equal k/255 is that value again
    s = np.array([[5 * int(q[77])]], dtype=np.int64)
    assert ref.mean_of(s, np.array([5], np.int32))[0, 0] == a[77]


def test_division_differs_from_the_reciprocal_where_the_gpu_test_says():
    p = np.arange(130000, dtype=np.float32)
    v = np.float32(0.3)
    r = np.float32(1.0) / v
    d = np.floor(p / v) != np.floor((p * r).astype(np.float32))
    assert int(d.sum()) == 17119 and int(np.flatnonzero(d)[0]) == 9
    q = (p + np.float32(0.5)).astype(np.float32)
    r7 = np.float32(1.0) / np.float32(7.0)
    d7 = np.rint(q / np.float32(7.0)) != np.rint((q * r7).astype(np.float32))
    assert int(d7.sum()) == 5454


def test_shell_figures():
    shell = aug.cube_shell(128)
    assert shell.shape[0] == 42608
    for voxel, m, most in ((2, 13280, 6), (3, 6224, 15), (8, 968, 82)):
        out = ref.voxelize_reference(shell, voxel=voxel)
        assert out["coords"].shape[0] == m and int(out["npts"].max()) == most and int(out["npts"].sum()) == 42608
    assert ref.voxelize_reference(shell, voxel=0.7)["coords"].shape[0] == 42608


def test_error_cases_of_the_restatement():
    xyz = np.zeros((4, 3), np.float32)
    ok = ref.voxelize_reference(xyz)
    assert ok["coords"].tolist() == [[0, 0, 0, 0]] and ok["npts"].tolist() == [4] and ok["sum"].shape == (1, 0)
    for bad in (np.nan, np.inf, -np.inf, 130001.0):
        x = xyz.copy()
        x[2, 1] = bad
        assert ref.voxelize_reference(x) == ref.COUNT_ERR_RANGE
    x = xyz.copy()
    x[0, 0] = 130000.0
    assert not isinstance(ref.voxelize_reference(x), int)
    assert ref.voxelize_reference(xyz, batch=[0, 1, 2, 3], nbatch=3) == ref.COUNT_ERR_RANGE
    assert ref.voxelize_reference(xyz, batch=[0, -1, 2, 1], nbatch=3) == ref.COUNT_ERR_RANGE
    for a in (np.float32(1) + np.float32(2.0 ** -23), np.nan, -np.inf):
        attr = np.zeros((4, 1), np.float32)
        attr[3, 0] = a
        assert ref.voxelize_reference(xyz, attr=attr) == ref.COUNT_ERR_RANGE
    for voxel in (0.0, -1.0, np.nan, np.inf):
        assert ref.voxelize_reference(xyz, voxel=voxel) == ref.ERR_ARG
    assert ref.voxelize_reference(xyz, attr=np.zeros((4, 17), np.float32)) == ref.ERR_ARG


def test_host_argument_checks_without_gpu(pcc):
    """refused on the host before any launch: the pointers are never dereferenced"""
    L = pcc.lib()
    n, cap = 1000, L.pcc_hash_capacity(1000)
    P = 4096                                               # a non-null pointer value nothing reads

    def call(voxel=1.0, c=3, cap=cap, n=n, nbatch=1, rounding=0, origin=(0.0, 0.0, 0.0), xyz=P, attr=P, keys=P, vals=P, scratch=P, coords=P,
             first=P, npts=P, sums=P, row=P, count=P):
        return L.pcc_voxelize(xyz, None, n, nbatch, attr, c, origin[0], origin[1], origin[2], voxel, rounding, keys, vals, cap, scratch,
                              coords, first, npts, sums, row, count, None)

    for kw, word in (({"voxel": 0.0}, b"voxel"), ({"voxel": -2.0}, b"voxel"), ({"voxel": float("nan")}, b"voxel"),
                     ({"voxel": float("inf")}, b"voxel"), ({"c": 17}, b"channels"), ({"c": -1}, b"channels"),
                     ({"cap": 1024}, b"capacity"), ({"cap": cap + 1}, b"capacity"), ({"cap": 0}, b"capacity"),
                     ({"n": -1}, b"count"), ({"nbatch": 0}, b"nbatch"), ({"nbatch": 1024}, b"nbatch"), ({"rounding": 2}, b"rounding"),
                     ({"origin": (0.0, float("nan"), 0.0)}, b"origin"),
                     ({"keys": None}, b"null"), ({"vals": None}, b"null"), ({"scratch": None}, b"null"), ({"count": None}, b"null"),
                     ({"xyz": None}, b"null"), ({"coords": None}, b"null"), ({"first": None}, b"null"), ({"npts": None}, b"null"),
                     ({"row": None}, b"null"), ({"attr": None}, b"null"), ({"sums": None}, b"null")):
        assert call(**kw) == ref.ERR_ARG, kw
        assert word in L.pcc_last_error(), (kw, L.pcc_last_error())
