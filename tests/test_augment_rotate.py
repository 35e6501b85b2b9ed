"""pcc_augment_rotate (csrc/augment.hip) through the C-ABI: the output rows, their source rows and the count EQUAL the
numpy float32 restatement (tests/_augment_reference.py) — the arithmetic is specified operation by operation, so nothing is
approximate — over the sizes at which the coordinate-set code changes path, matrices that make rounding order matter, exact .5
ties, heavy collapses, batches, duplicates and the range / NaN error path."""
import functools

import numpy as np
import pytest
import torch

import _augment_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EYE = np.eye(3, dtype=np.float32).reshape(9)


def run_abi(pcc, coords, rot, half):
    """-> (out_coords, out_src) as numpy, or the negative count word"""
    from pcc_amd._lib import check, ptr, stream
    L = pcc.lib()
    coords = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 4)
    rot = np.ascontiguousarray(rot, dtype=np.float32).reshape(-1, 9)
    n = coords.shape[0]
    C = torch.from_numpy(coords).to(DEV)
    R = torch.from_numpy(rot).to(DEV)
    cap = L.pcc_hash_capacity(n)
    keys = torch.empty(cap, dtype=torch.int64, device=DEV)
    vals = torch.empty(cap, dtype=torch.int32, device=DEV)
    scratch = torch.empty(L.pcc_scan_scratch_elems(n), dtype=torch.int32, device=DEV)
    out = torch.full((max(n, 1), 4), -7, dtype=torch.int32, device=DEV)
    src = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    check(L.pcc_augment_rotate(ptr(C), n, ptr(R), rot.shape[0], float(half), ptr(keys), ptr(vals), cap, ptr(scratch), ptr(out), ptr(src),
                               ptr(count), stream()))
    m = int(count.item())
    if m < 0:
        return m
    oc, os_ = out[:m].cpu().numpy(), src[:m].cpu().numpy()
    # on return the table indexes the output set with tensor stride 1: every output row finds itself
    if m:
        idx = torch.empty(m, dtype=torch.int32, device=DEV)
        check(L.pcc_hash_lookup(ptr(keys), ptr(vals), cap, 1, ptr(out), m, ptr(idx), stream()))
        assert np.array_equal(idx.cpu().numpy(), np.arange(m))
    return oc, os_


def assert_equal_to_reference(pcc, coords, rot, half):
    want = ref.rotate_reference(coords, rot, half)
    got = run_abi(pcc, coords, rot, half)
    assert not isinstance(want, int), "the case is meant to be in range"
    assert not isinstance(got, int), got
    assert got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])
    return got


@functools.lru_cache(maxsize=None)
def cloud(n):
    """n distinct voxels of a 128-block (the 40 k shell of a sphere, or a prefix of it), shuffled"""
    shell = ref.cube_shell(128)
    assert shell.shape[0] >= n
    return ref.rows_of(shell[:n])


def random_matrix(seed):
    rng = np.random.default_rng(seed)
    return ref.angle_matrix(rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi))


SIZES = (0, 1, 255, 256, 257, 8192, 8193)


@pytest.mark.parametrize("n", SIZES)
def test_random_angles_over_the_path_boundaries(pcc, n):
    """one workgroup and its neighbours, and 8192 / 8193 — eight and nine tiles of the flag scan (the boundary at which the
    coordinate manager's own set construction changes form)"""
    oc, _ = assert_equal_to_reference(pcc, cloud(n), random_matrix(n), 64.0)
    assert oc.shape[0] <= n and (n == 0 or oc.shape[0] > 0.5 * n)


def test_shell_of_a_128_cube(pcc):
    c = ref.rows_of(ref.cube_shell(128))
    assert 35000 < c.shape[0] < 50000
    for seed in (1, 2):
        oc, os_ = assert_equal_to_reference(pcc, c, random_matrix(100 + seed), 64.0)
        assert np.unique(oc, axis=0).shape[0] == oc.shape[0]
    # the identity passes every row through
    oc, os_ = assert_equal_to_reference(pcc, c, EYE, 64.0)
    assert np.array_equal(oc, c) and np.array_equal(os_, np.arange(c.shape[0]))


@pytest.mark.parametrize("n", (8192, 40000))
def test_quarter_scale_collapse(pcc, n):
    c = cloud(n) if n <= 8192 else ref.rows_of(ref.cube_shell(128)[:n])
    oc, _ = assert_equal_to_reference(pcc, c, 0.25 * EYE, 64.0)
    assert oc.shape[0] < c.shape[0] / 2             # (a surface: 16-fold at full density, less for a sample of it)


def test_ties_to_even_on_both_sides_of_zero(pcc):
    """ref.HALF_MATRIX, half = 63.5: x' = (x + y) / 2 exactly, so odd x + y is an exact .5 tie; the block spans both signs"""
    g = np.arange(-20, 21)
    xyz = np.stack(np.meshgrid(g, g, np.array([3, 4]), indexing="ij"), -1).reshape(-1, 3)
    xyz = xyz[np.random.default_rng(3).permutation(xyz.shape[0])]
    oc, os_ = assert_equal_to_reference(pcc, ref.rows_of(xyz), ref.HALF_MATRIX, 63.5)
    s = xyz[os_, 0] + xyz[os_, 1]
    odd = s % 2 != 0
    assert odd.sum() > 100 and (s[odd] < 0).any() and (s[odd] > 0).any()
    assert np.all(oc[odd, 1] % 2 == 0)                       # every tie went to the even neighbour
    assert np.array_equal(oc[~odd, 1], s[~odd] // 2)


def test_three_items_equal_the_items_coded_alone(pcc):
    rng = np.random.default_rng(9)
    shell = ref.cube_shell(128)
    sizes = (3000, 700, 9000)
    mats = np.stack([random_matrix(31), EYE, random_matrix(33)])
    parts, alone_c, alone_s, base = [], [], [], 0
    for b, n in enumerate(sizes):
        xyz = shell[rng.permutation(shell.shape[0])[:n]]
        parts.append(ref.rows_of(xyz, b))
        oc, os_ = assert_equal_to_reference(pcc, ref.rows_of(xyz, 0), mats[b], 64.0)
        oc = oc.copy()
        oc[:, 0] = b
        alone_c.append(oc)
        alone_s.append(os_ + base)
        base += n
    oc, os_ = assert_equal_to_reference(pcc, np.concatenate(parts), mats, 64.0)
    assert np.array_equal(oc, np.concatenate(alone_c)) and np.array_equal(os_, np.concatenate(alone_s))
    assert np.array_equal(oc[oc[:, 0] == 1], parts[1])       # the identity item is unchanged
    assert np.all(np.diff(oc[:, 0]) >= 0)                    # still grouped by item


def test_same_xyz_in_two_items_stays_separate(pcc):
    xyz = ref.cube_shell(128)[:500]
    c = np.concatenate([ref.rows_of(xyz, 0), ref.rows_of(xyz, 1)])
    m = random_matrix(5)
    oc, os_ = assert_equal_to_reference(pcc, c, np.stack([m, m]), 64.0)
    k = oc.shape[0] // 2
    assert oc.shape[0] == 2 * k and np.array_equal(oc[:k, 1:], oc[k:, 1:]) and np.array_equal(os_[:k] + 500, os_[k:])


def test_duplicate_input_rows_first_wins(pcc):
    xyz = ref.cube_shell(128)[:300]
    c = ref.rows_of(np.concatenate([xyz, xyz[::-1], xyz[:50]]))
    oc, os_ = assert_equal_to_reference(pcc, c, EYE, 64.0)
    assert np.array_equal(os_, np.arange(300)) and np.array_equal(oc, c[:300])


@pytest.mark.parametrize("n", (200, 20000))
def test_out_of_range_and_nan_are_errors(pcc, n):
    """a handled error path: the count word is PCC_COUNT_ERR_RANGE, Python raises ValueError; a NaN is never converted"""
    from pcc_amd import augment
    c = cloud(8192)[:n] if n <= 8192 else ref.rows_of(ref.cube_shell(128)[:n])
    far = 4000.0 * EYE                                       # 64 * 4000 leaves +-130000
    nan = EYE.copy()
    nan[4] = np.nan
    inf = EYE.copy()
    inf[0] = np.inf
    for m in (far, nan, inf):
        assert ref.rotate_reference(c, m, 64.0) == ref.COUNT_ERR_RANGE
        assert run_abi(pcc, c, m, 64.0) == ref.COUNT_ERR_RANGE
        C = torch.from_numpy(c).to(DEV)
        F = torch.zeros((n, 3), device=DEV)
        with pytest.raises(ValueError):
            augment.random_rotate(C, F, m.reshape(1, 9), 128)
    # a batch index without a matrix is the same error, not a read past the matrices
    c2 = c.copy()
    c2[-1, 0] = 1
    assert run_abi(pcc, c2, EYE, 64.0) == ref.COUNT_ERR_RANGE
    # and the path is still usable afterwards
    assert_equal_to_reference(pcc, c, EYE, 64.0)


def test_python_random_rotate_gathers_colours(pcc):
    from pcc_amd import augment
    c = cloud(8193)
    F = np.random.default_rng(4).random((c.shape[0], 3), dtype=np.float32)
    m = random_matrix(77)
    C2, F2 = augment.random_rotate(torch.from_numpy(c).to(DEV), torch.from_numpy(F).to(DEV), m.reshape(1, 9), 128)
    want_c, want_s = ref.rotate_reference(c, m, 64.0)
    assert np.array_equal(C2.cpu().numpy(), want_c) and np.array_equal(F2.cpu().numpy(), F[want_s])


def test_rotation_matrices_match_the_matrix_product(pcc):
    from pcc_amd import augment
    rng = np.random.default_rng(8)
    phi, theta = rng.uniform(0, 2 * np.pi, 16), rng.uniform(0, 2 * np.pi, 16)
    got = augment.rotation_matrices(phi, theta)
    want = np.stack([ref.angle_matrix(p, t) for p, t in zip(phi, theta)])
    assert got.dtype == np.float32 and got.shape == (16, 9) and np.abs(got - want).max() <= 1.2e-7
    assert np.array_equal(augment.rotation_matrices([0.0], [0.0])[0], EYE)
