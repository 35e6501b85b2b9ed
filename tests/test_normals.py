"""pcc_estimate_normals (csrc/normals.hip) through normals.estimate_normals against the numpy restatement
(tests/_normals_reference.py): counts, moments and validity are integers and must be EQUAL; normals agree with numpy.linalg.eigh
up to sign wherever the smallest eigenvalue is separated from the next one.

The bound on the normals: an eigenvector moves by (perturbation of the matrix) / (eigen-gap).  Both sides carry float64
round-off of O(10^2) units over their iterations, 1.1e-16 * 1e2 relative to the largest eigenvalue, so at the relative gap
floor of 1e-3 the two agree to 1e-11 rad: |n x n_ref| <= 1e-9 holds with two orders to spare.  Points below the floor are left
out; they may be 1 % of an input at most, and the two shells have none (tests/test_normals_reference.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _normals_reference as ref

DEV = "cuda:0"
GAP_FLOOR = 1e-3


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name == "shell":
        return ref.shell(32, 11, 0.875)
    if name == "thin":
        return ref.shell(64, 25, 0.5)
    if name == "random":
        return ref.random_cloud()
    if name == "plane":
        g = np.arange(16)
        p = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
        return np.concatenate([p, np.full((256, 1), 5)], axis=1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, R):
    pts = cloud(name)
    count, moments = ref.ball_moments(pts, np.zeros(len(pts), np.int64), R)
    return (count, moments) + ref.reference_normals(count, moments)


def run_gpu(pts, R, batch=None, **kw):
    from pcc_amd import CoordMap, estimate_normals
    b = np.zeros(len(pts), np.int64) if batch is None else batch
    coords = torch.from_numpy(np.concatenate([b[:, None], pts], axis=1).astype(np.int32)).to(DEV)
    cmap = CoordMap(coords, 1, nbatch=int(b.max()) + 1)
    normals, count, moments = estimate_normals(coords, radius=R, coord_map=cmap, return_moments=True, **kw)
    assert normals.dtype == torch.float64 and count.dtype == torch.int32 and moments.dtype == torch.int64
    return normals.cpu().numpy(), count.cpu().numpy(), moments.cpu().numpy()


@functools.lru_cache(maxsize=None)
def gpu(name, R):
    return run_gpu(cloud(name), R)


def test_argument_checks_of_the_c_abi(pcc):
    """host-side: the radius is checked before anything is launched (runs without a GPU)"""
    L = pcc.lib()
    out = np.zeros(3)
    for R in (0, 9):
        assert L.pcc_estimate_normals(None, 1, None, None, 1024, 1, R, 0, None, out.ctypes.data, None, None, None) < 0
        assert b"radius" in L.pcc_last_error()
    assert L.pcc_estimate_normals(None, 1, None, None, 1000, 1, 3, 0, None, out.ctypes.data, None, None, None) < 0      # capacity
    assert L.pcc_estimate_normals(None, 1, None, None, 1024, 1, 3, 3, None, out.ctypes.data, None, None, None) < 0      # orient_mode
    assert L.pcc_estimate_normals(None, 1, None, None, 1024, 1, 3, 1, None, out.ctypes.data, None, None, None) < 0      # no direction
    assert L.pcc_estimate_normals(None, 1, None, None, 1024, 1, 3, 0, None, None, None, None, None) < 0                 # no output
    assert L.pcc_estimate_normals(None, 0, None, None, 1024, 1, 3, 0, None, out.ctypes.data, None, None, None) == 0     # nothing to do


CASES = [("shell", 1), ("shell", 2), ("shell", 3), ("shell", 8), ("thin", 3), ("random", 2), ("plane", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,R", CASES)
def test_counts_and_moments_equal_the_reference(pcc, name, R):
    want_count, want_moments = reference(name, R)[:2]
    _, count, moments = gpu(name, R)
    assert np.array_equal(count, want_count)
    assert np.array_equal(moments, want_moments)


@pytest.mark.gpu
def test_batch_items_do_not_leak(pcc):
    """two items, the second the shell shifted by one voxel: the first one's rows equal the single-item run bit for bit"""
    pts = cloud("shell")
    both = np.concatenate([pts, pts + [1, 0, 0]])
    batch = np.concatenate([np.zeros(len(pts), np.int64), np.ones(len(pts), np.int64)])
    normals, count, moments = run_gpu(both, 3, batch=batch)
    one_normals, one_count, one_moments = gpu("shell", 3)
    n = len(pts)
    assert np.array_equal(count[:n], one_count) and np.array_equal(moments[:n], one_moments)
    assert np.array_equal(normals[:n].view(np.int64), one_normals.view(np.int64))
    want_count, want_moments = ref.ball_moments(both, batch, 3)
    assert np.array_equal(count, want_count) and np.array_equal(moments, want_moments)
    assert np.array_equal(count[n:], one_count) and np.array_equal(normals[n:].view(np.int64), one_normals.view(np.int64))


@pytest.mark.gpu
def test_validity_equals_the_reference(pcc):
    _, _, _, valid, _ = reference("random", 2)
    assert (~valid).any() and valid.any()
    normals, _, _ = gpu("random", 2)
    assert np.array_equal((normals != 0).any(1), valid)
    assert not normals[~valid].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name,R", [("shell", 3), ("thin", 3), ("random", 2), ("shell", 8), ("shell", 2)])
def test_normals_match_the_reference(pcc, name, R):
    _, _, want, valid, gap = reference(name, R)
    normals, _, _ = gpu(name, R)
    assert np.array_equal((normals != 0).any(1), valid)
    judged = valid & (gap >= GAP_FLOOR)
    left_out = int((valid & ~judged).sum())
    assert left_out <= 0.01 * valid.sum()
    if name in ("shell", "thin") and R == 3:
        assert left_out == 0
    cross = np.linalg.norm(np.cross(normals[judged], want[judged]), axis=1)
    length = np.abs(np.linalg.norm(normals[valid], axis=1) - 1.0)
    print("%s R=%d: %d valid, %d below the gap floor, |n x n_ref| max %.3g, ||n| - 1| max %.3g" % (name, R, valid.sum(), left_out,
                                                                                                cross.max(), length.max()))
    assert cross.max() <= 1e-9
    assert length.max() <= 1e-12


@pytest.mark.gpu
def test_plane_normals_are_exact(pcc):
    pts = cloud("plane")
    normals, count, _ = gpu("plane", 3)
    interior = ((pts[:, :2] >= 3) & (pts[:, :2] <= 12)).all(1)
    assert (count[interior] == 29).all()
    assert np.array_equal(np.abs(normals), np.tile([0.0, 0.0, 1.0], (256, 1)))      # border points too: their neighbours lie in the plane


@pytest.mark.gpu
def test_orientation(pcc):
    from pcc_amd import estimate_normals
    pts = cloud("shell")
    plain, _, _ = gpu("shell", 3)
    x = torch.from_numpy(pts.astype(np.float32)).to(DEV)             # the [N, 3+] cloud form of the call
    n_dir, count = estimate_normals(x, radius=3, direction=(0, 0, 1))
    n_dir = n_dir.cpu().numpy()
    assert np.array_equal(count.cpu().numpy(), reference("shell", 3)[0])
    assert (n_dir[:, 2] >= 0).all() and (n_dir[:, 2] > 0).any() and (plain[:, 2] < 0).any()
    assert np.array_equal(np.abs(n_dir).view(np.int64), np.abs(plain).view(np.int64))
    assert np.array_equal(n_dir, np.where((plain[:, 2:3] < 0), -plain, plain))
    centre = (15.5, 15.5, 15.5)
    n_cam = estimate_normals(x, radius=3, camera=centre)[0].cpu().numpy()
    dot = (n_cam * (np.array(centre) - pts)).sum(1)
    assert (dot >= 0).all() and dot.min() > 5.0                       # inward, and far from the sign's edge (the shell's radius is 11)
    assert np.array_equal(np.abs(n_cam).view(np.int64), np.abs(plain).view(np.int64))
    n_out = estimate_normals(x, radius=3, camera=np.array(centre), coord_map=None)[0].cpu().numpy()
    assert np.array_equal(n_out, n_cam)
    with pytest.raises(ValueError):
        estimate_normals(x, radius=3, direction=(0, 0, 1), camera=centre)
    with pytest.raises(ValueError):
        estimate_normals(x + 0.5, radius=3)


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal(pcc):
    first = gpu("thin", 3)
    again = run_gpu(cloud("thin"), 3)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [0, 9])
def test_radius_out_of_range_raises(pcc, R):
    from pcc_amd._lib import PccError
    with pytest.raises(PccError, match="radius"):
        run_gpu(cloud("plane"), R)
    assert b"radius" in pcc.lib().pcc_last_error()
