"""pcc_voxelize (csrc/voxelize.hip) through the C-ABI, every output buffer pre-filled with a sentinel: the voxels, their first
points, the point rows, the counts and the Q32 sums EQUAL the numpy restatement (tests/_voxelize_reference.py) — the contract of
include/pcc_hip.h fixes every operation, so nothing is approximate — over the sizes at which the flag scan changes tile count,
the points at which a division differs from a multiplication by the reciprocal, exact ties, the run shapes at which a wave-level
fold can go wrong, channel counts, batches, the Q32 edges and the range error path."""
import functools

import numpy as np
import pytest
import torch

import _augment_reference as aug
import _voxelize_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7


def run_abi(pcc, xyz, batch=None, nbatch=1, attr=None, origin=(0, 0, 0), voxel=1.0, rounding=0):
    """-> dict like the restatement's, as numpy, or the negative count word"""
    from pcc_amd._lib import check, ptr, stream
    L = pcc.lib()
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    c = 0 if attr is None else np.asarray(attr).shape[1]
    X = torch.from_numpy(xyz).to(DEV)
    B = None if batch is None else torch.from_numpy(np.ascontiguousarray(batch, dtype=np.int32)).to(DEV)
    A = None if attr is None else torch.from_numpy(np.ascontiguousarray(attr, dtype=np.float32).reshape(n, c)).to(DEV)
    cap = L.pcc_hash_capacity(n)
    keys = torch.full((cap,), SENTINEL, dtype=torch.int64, device=DEV)
    vals = torch.full((cap,), SENTINEL, dtype=torch.int32, device=DEV)
    scratch = torch.full((L.pcc_scan_scratch_elems(n),), SENTINEL, dtype=torch.int32, device=DEV)
    m1 = max(n, 1)
    coords = torch.full((m1, 4), SENTINEL, dtype=torch.int32, device=DEV)
    first = torch.full((m1,), SENTINEL, dtype=torch.int32, device=DEV)
    npts = torch.full((m1,), SENTINEL, dtype=torch.int32, device=DEV)
    sums = torch.full((m1, max(c, 1)), SENTINEL, dtype=torch.int64, device=DEV)
    row = torch.full((m1,), SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    o = [float(np.float32(v)) for v in origin]
    check(L.pcc_voxelize(ptr(X), ptr(B), n, nbatch, ptr(A), c, o[0], o[1], o[2], float(np.float32(voxel)), rounding, ptr(keys), ptr(vals),
                         cap, ptr(scratch), ptr(coords), ptr(first), ptr(npts), ptr(sums), ptr(row), ptr(count), stream()))
    m = int(count.item())
    if m < 0:
        return m
    # rows behind the count are not written
    assert bool((coords[m:] == SENTINEL).all()) and bool((npts[m:] == SENTINEL).all()) and bool((sums[m:] == SENTINEL).all())
    # on return the table indexes the output set with tensor stride 1: every output row finds itself
    if m:
        idx = torch.empty(m, dtype=torch.int32, device=DEV)
        check(L.pcc_hash_lookup(ptr(keys), ptr(vals), cap, 1, ptr(coords), m, ptr(idx), stream()))
        assert np.array_equal(idx.cpu().numpy(), np.arange(m))
    return {"coords": coords[:m].cpu().numpy(), "first": first[:m].cpu().numpy(), "npts": npts[:m].cpu().numpy(),
            "sum": sums[:m, :c].cpu().numpy(), "row": row[:n].cpu().numpy()}


def assert_equal_to_reference(pcc, xyz, **kw):
    want = ref.voxelize_reference(xyz, **kw)
    got = run_abi(pcc, xyz, **kw)
    assert not isinstance(want, int), "the case is meant to be in range"
    assert not isinstance(got, int), got
    for name in ("coords", "first", "row", "npts", "sum"):
        assert got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        assert got[name].dtype == want[name].dtype, (name, got[name].dtype)
        assert np.array_equal(got[name], want[name]), name
    return got


@functools.lru_cache(maxsize=None)
def shell():
    s = aug.cube_shell(128).astype(np.float32)
    assert s.shape[0] == 42608
    return s


@functools.lru_cache(maxsize=None)
def shell_colours():
    return ref.colours(42608, seed=1)


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, 8192, 8193))
def test_scan_boundaries(pcc, n):
    """one workgroup and its neighbours, and 8192 / 8193: the sizes at which the flag scan changes tile count"""
    out = assert_equal_to_reference(pcc, shell()[:n], attr=shell_colours()[:n], voxel=2.0)
    assert int(out["npts"].sum()) == n


@pytest.mark.parametrize("voxel,m,most", ((2.0, 13280, 6), (3.0, 6224, 15), (8.0, 968, 82), (0.7, 42608, 1)))
def test_whole_shell(pcc, voxel, m, most):
    out = assert_equal_to_reference(pcc, shell(), attr=shell_colours(), voxel=voxel)
    assert out["coords"].shape[0] == m and int(out["npts"].max()) == most and int(out["npts"].sum()) == 42608


def test_division_is_not_a_multiplication_by_the_reciprocal(pcc):
    """floor(p / 0.3f) differs from floor(p * (1 / 0.3f)) at 17,119 of the integers below 130,000 (the first is 9), and
    rint((p + 0.5) / 7) from its reciprocal form at 5,454: a few thousand of exactly those points, and as many others"""
    p = np.arange(130000, dtype=np.float32)
    for voxel, offset, rounding in ((0.3, 0.0, 0), (7.0, 0.5, 1)):
        v = np.float32(voxel)
        q = (p + np.float32(offset)).astype(np.float32)
        rnd = np.rint if rounding else np.floor
        differs = np.flatnonzero(rnd(q / v) != rnd((q * (np.float32(1.0) / v)).astype(np.float32)))
        assert differs.shape[0] == (5454 if rounding else 17119)
        if not rounding:
            assert differs[0] == 9
        # (p / 0.3 must stay inside the coordinate range)
        pick = differs[q[differs] / v < ref.COORD_LIMIT][:3000]
        assert pick.shape[0] == 3000
        x = np.zeros((6000, 3), np.float32)
        x[:3000, 0] = q[pick]
        x[3000:, 1] = q[pick - 1]
        x = x[np.random.default_rng(2).permutation(6000)]
        assert_equal_to_reference(pcc, x, voxel=voxel, rounding=rounding)


def test_ties_negatives_and_origin(pcc):
    g = np.arange(-40, 41, dtype=np.float32) * np.float32(0.5)            # -20 .. 20 in halves: every second one an exact .5 tie
    xyz = np.stack(np.meshgrid(g, g, np.float32([-1.5, 2.5]), indexing="ij"), -1).reshape(-1, 3)
    xyz = xyz[np.random.default_rng(3).permutation(xyz.shape[0])]
    out = assert_equal_to_reference(pcc, xyz, voxel=1.0, rounding=1)
    src = xyz[out["first"]]
    tie = src[:, 0] % 1 != 0
    assert tie.sum() > 100 and (src[tie, 0] < 0).any() and (src[tie, 0] > 0).any()
    assert np.all(out["coords"][tie, 1] % 2 == 0)                        # every tie went to the even neighbour
    assert set(out["coords"][:, 3].tolist()) == {-2, 2}                  # -1.5 -> -2, 2.5 -> 2
    # floor on negative coordinates: towards minus infinity
    out = assert_equal_to_reference(pcc, xyz, voxel=1.0, rounding=0)
    assert np.array_equal(out["coords"][:, 1], np.floor(xyz[out["first"], 0]).astype(np.int32)) and out["coords"][:, 1].min() == -20
    assert set(out["coords"][:, 3].tolist()) == {-2, 2}
    # a non-zero origin, both roundings, a voxel that is no power of two
    for rounding in (0, 1):
        assert_equal_to_reference(pcc, xyz, attr=ref.colours(xyz.shape[0], 4), origin=(-20.25, 0.125, -3.0), voxel=0.75, rounding=rounding)


def test_contention_on_one_voxel(pcc):
    n = 8193
    xyz = np.random.default_rng(6).random((n, 3), dtype=np.float32) * 900
    out = assert_equal_to_reference(pcc, xyz, attr=ref.colours(n, 7), voxel=1000.0)
    assert out["npts"].tolist() == [n]


@pytest.mark.parametrize("run", (1, 2, 63, 64, 65, "alternating"))
def test_runs_of_equal_cells(pcc, run):
    """rows arriving in runs of equal cells, with a ragged last wave: where a wave-level fold goes wrong"""
    n = 64 * 37 + 29
    if run == "alternating":
        cell = np.arange(n) % 2
    else:
        cell = (np.arange(n) // run) % 11                   # the same 11 cells come back: runs of one row far apart
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 2] = cell * 3 + 1
    out = assert_equal_to_reference(pcc, xyz, attr=ref.colours(n, 8), voxel=3.0)
    assert out["coords"].shape[0] == (2 if run == "alternating" else 11)


@pytest.mark.parametrize("c", (0, 1, 3, 16))
def test_channel_counts(pcc, c):
    n = 5000
    attr = None if c == 0 else ref.colours(n, 9, c)
    assert_equal_to_reference(pcc, shell()[:n], attr=attr, voxel=4.0)


def test_batch_items_do_not_merge(pcc):
    n = 3000
    xyz = np.concatenate([shell()[:n]] * 3)
    batch = np.repeat(np.arange(3, dtype=np.int32), n)
    attr = ref.colours(3 * n, 10)
    alone = assert_equal_to_reference(pcc, shell()[:n], attr=attr[:n], voxel=4.0)
    out = assert_equal_to_reference(pcc, xyz, batch=batch, nbatch=3, attr=attr, voxel=4.0)
    m = alone["coords"].shape[0]
    assert out["coords"].shape[0] == 3 * m and np.array_equal(out["coords"][:m], alone["coords"])
    assert np.array_equal(out["coords"][m:2 * m, 1:], alone["coords"][:, 1:]) and np.all(out["coords"][m:2 * m, 0] == 1)
    # interleaved items: still nothing merges across them, and a null batch puts everything into item 0
    perm = np.random.default_rng(11).permutation(3 * n)
    assert_equal_to_reference(pcc, xyz[perm], batch=batch[perm], nbatch=3, attr=attr[perm], voxel=4.0)
    merged = assert_equal_to_reference(pcc, xyz, attr=attr, voxel=4.0)
    assert merged["coords"].shape[0] == m and np.array_equal(merged["npts"], 3 * alone["npts"])


def test_q32_edges(pcc):
    vals = np.float32([0, 1, -1, 2.0 ** -33, 3 * 2.0 ** -33, 2.0 ** -9 + 2.0 ** -33])
    n = 6 * 50
    attr = np.stack([np.tile(vals, 50), np.repeat(vals, 50), np.tile(vals[::-1], 50)], 1).astype(np.float32)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = np.arange(n) % 4
    out = assert_equal_to_reference(pcc, xyz, attr=attr, voxel=1.0)
    assert out["sum"][:, 0].sum() == 50 * (0 + 2 ** 32 - 2 ** 32 + 0 + 2 + 2 ** 23)
    one = assert_equal_to_reference(pcc, np.zeros((3, 3), np.float32), attr=np.float32([[1], [1], [1]]), voxel=1.0)
    assert one["sum"].tolist() == [[3 * 2 ** 32]]


def _offenders():
    big = np.float32(130001.0)
    return {"nan": ("xyz", np.nan), "inf": ("xyz", np.inf), "minus_inf": ("xyz", -np.inf), "beyond_limit": ("xyz", big),
            "batch": ("batch", 2), "attr_above_one": ("attr", np.float32(1) + np.float32(2.0 ** -23)), "attr_nan": ("attr", np.nan)}


@pytest.mark.parametrize("case", sorted(_offenders()))
def test_range_errors(pcc, case):
    """one offender among 9,000 points: the count word is PCC_COUNT_ERR_RANGE; without it the call equals the restatement"""
    what, value = _offenders()[case]
    n, at = 9000, 4321
    xyz = shell()[:n].copy()
    batch = (np.arange(n) % 2).astype(np.int32)
    attr = shell_colours()[:n].copy()
    if what == "xyz":
        xyz[at, 1] = value
    elif what == "batch":
        batch[at] = value
    else:
        attr[at, 2] = value
    kw = dict(nbatch=2, voxel=1.0)
    assert ref.voxelize_reference(xyz, batch=batch, attr=attr, **kw) == ref.COUNT_ERR_RANGE
    assert run_abi(pcc, xyz, batch=batch, attr=attr, **kw) == ref.COUNT_ERR_RANGE
    keep = np.arange(n) != at
    assert_equal_to_reference(pcc, xyz[keep], batch=batch[keep], attr=attr[keep], **kw)


def test_the_limit_itself_is_in_range(pcc):
    xyz = np.float32([[130000, -130000, 0], [0, 0, 0], [130000, -130000, 0.5]])
    out = assert_equal_to_reference(pcc, xyz, voxel=1.0)
    assert out["coords"].tolist() == [[0, 130000, -130000, 0], [0, 0, 0, 0]]


def test_order_independence(pcc):
    """the shell at voxel 3 in two orders: after sorting the output rows by coordinate, counts and sums are identical arrays"""
    outs = []
    for seed in (21, 22):
        perm = np.random.default_rng(seed).permutation(42608)
        out = assert_equal_to_reference(pcc, shell()[perm], attr=shell_colours()[perm], voxel=3.0)
        order = np.lexsort(out["coords"].T[::-1])
        outs.append((out["coords"][order], out["npts"][order], out["sum"][order]))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
