"""Known-answer tests of the numpy restatements the augmentation kernels are held to (tests/_augment_reference.py), and the
measurement of the jitter tolerance: float32 restatement against float64 restatement over the GPU test's inputs."""
import numpy as np
import pytest

import _augment_reference as ref


def _cloud(n=500, seed=1, lo=0, hi=64):
    rng = np.random.default_rng(seed)
    xyz = np.unique(rng.integers(lo, hi, (n, 3)), axis=0)
    return ref.rows_of(xyz[rng.permutation(xyz.shape[0])])


def test_rotate_identity_passes_rows_through():
    c = _cloud()
    for half in (32.0, 31.5, 64.0):
        out, src = ref.rotate_reference(c, np.eye(3, dtype=np.float32).reshape(1, 9), half)
        assert np.array_equal(out, c) and np.array_equal(src, np.arange(c.shape[0]))


def test_rotate_signed_permutations_are_exact_relabellings():
    c = _cloud()
    half = 31.5                                              # the centre of a 64-block's voxel centres: the block maps onto itself
    for M in ref.signed_permutations():
        out, src = ref.rotate_reference(c, M.reshape(1, 9), half)
        R = M.reshape(3, 3).astype(np.int64)
        want = ((2 * c[:, 1:].astype(np.int64) - 63) @ R.T + 63) // 2        # exact integer arithmetic on doubled coordinates
        assert np.array_equal(src, np.arange(c.shape[0]))                    # a bijection: nothing merges
        assert np.array_equal(out[:, 1:], want) and np.array_equal(out[:, 0], c[:, 0])
        assert want.min() >= 0 and want.max() <= 63


def test_rotate_first_occurrence_ties_and_errors():
    c = ref.rows_of([(0, 0, 0), (1, 0, 0), (0, 0, 0), (3, 3, 3), (1, 0, 0)])
    out, src = ref.rotate_reference(c, np.eye(3, dtype=np.float32).reshape(1, 9), 2.0)
    assert src.tolist() == [0, 1, 3] and out[:, 1:].tolist() == [[0, 0, 0], [1, 0, 0], [3, 3, 3]]
    big = (4000.0 * np.eye(3, dtype=np.float32)).reshape(1, 9)
    assert ref.rotate_reference(ref.rows_of([(100, 0, 0)]), big, 0.0) == ref.COUNT_ERR_RANGE
    nan = np.full((1, 9), np.nan, dtype=np.float32)
    assert ref.rotate_reference(c, nan, 2.0) == ref.COUNT_ERR_RANGE
    # two items with the same xyz stay separate
    two = np.concatenate([ref.rows_of([(1, 2, 3)], 0), ref.rows_of([(1, 2, 3)], 1)])
    out, src = ref.rotate_reference(two, np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (2, 1)), 2.0)
    assert out.shape[0] == 2 and src.tolist() == [0, 1]


def test_rint_ties_to_even_in_the_half_matrix_case():
    """ref.HALF_MATRIX with half = 63.5: x' = (0.5 (x - 63.5) + 0.5 (y - 63.5)) + 63.5 = (x + y) / 2, every step exact in fp32, so
    odd x + y gives exact .5 ties on both sides of zero, which go to the even neighbour"""
    pts = ref.rows_of([(1, 0, 9), (2, 1, 9), (3, 2, 9), (-3, 2, 9), (-2, -1, 9), (-4, 1, 9), (-6, -1, 9), (4, 4, 9)])
    out, src = ref.rotate_reference(pts, ref.HALF_MATRIX.reshape(1, 9), 63.5)
    # (x + y) / 2 = 0.5, 1.5, 2.5, -0.5, -1.5, -1.5, -3.5, 4 -> 0, 2, 2, 0, -2, -2, -4, 4; y' = y / 2 + 31.75 tells the rows apart
    got = {int(r): int(v) for r, v in zip(src, out[:, 1])}
    assert got == {0: 0, 1: 2, 2: 2, 3: 0, 4: -2, 5: -2, 6: -4, 7: 4}, got


def _img(n=64, seed=5):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jitter_identity(dtype):
    c = _img()
    for order in ref.ORDERS:
        out = ref.jitter_item(c, (1.0, 1.0, 1.0, 0.0), order, dtype)
        assert out.dtype == dtype and np.abs(out - c).max() <= (1e-12 if dtype == np.float64 else 5e-7)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jitter_saturation_zero_gives_gray(dtype):
    c = _img()
    out = ref.jitter_item(c, (1.0, 1.0, 0.0, 0.0), [ref.SATURATION, ref.BRIGHTNESS, ref.CONTRAST, ref.HUE], dtype)
    g = 0.2989 * c[:, 0].astype(np.float64) + 0.587 * c[:, 1] + 0.114 * c[:, 2]
    assert np.abs(out - g[:, None]).max() <= 5e-7


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jitter_hue_third_turns_red_into_green(dtype):
    red = np.array([[1.0, 0.0, 0.0]], dtype=np.float32)
    out = ref.jitter_item(red, (1.0, 1.0, 1.0, 1.0 / 3.0), [ref.HUE, ref.BRIGHTNESS, ref.SATURATION, ref.CONTRAST], dtype)
    assert np.abs(out - np.array([[0.0, 1.0, 0.0]])).max() <= 1e-6
    out = ref.jitter_item(red, (1.0, 1.0, 1.0, -1.0 / 3.0), [ref.HUE, ref.BRIGHTNESS, ref.SATURATION, ref.CONTRAST], dtype)
    assert np.abs(out - np.array([[0.0, 0.0, 1.0]])).max() <= 1e-6           # the other direction wraps below zero


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jitter_gray_passes_through_hue(dtype):
    g = np.repeat(np.linspace(0, 1, 33, dtype=np.float32)[:, None], 3, axis=1)
    for f in (-0.3, 0.1, 0.3):
        out = ref.jitter_item(g, (1.0, 1.0, 1.0, f), [ref.HUE, ref.BRIGHTNESS, ref.SATURATION, ref.CONTRAST], dtype)
        assert np.array_equal(out.astype(np.float32), g)


def test_jitter_contrast_uses_the_mean_at_its_stage():
    c = _img(200)
    out = ref.jitter_item(c, (0.5, 0.75, 1.0, 0.0), [ref.BRIGHTNESS, ref.CONTRAST, ref.SATURATION, ref.HUE])
    b = 0.5 * c.astype(np.float64)
    m = (0.2989 * b[:, 0] + 0.587 * b[:, 1] + 0.114 * b[:, 2]).mean()
    assert np.abs(out - np.clip(0.75 * b + 0.25 * m, 0, 1)).max() <= 1e-12


def measured_deviation():
    worst = 0.0
    for name, (rgb, off, par, order) in ref.jitter_cases().items():
        a = ref.jitter_reference(rgb, off, par, order, np.float64)
        b = ref.jitter_reference(rgb, off, par, order, np.float32)
        assert b.dtype == np.float32 and a.min() >= 0.0 and a.max() <= 1.0
        worst = max(worst, float(np.abs(a - b.astype(np.float64)).max()))
    return worst


def test_measured_jitter_tolerance():
    """JITTER_F32_DEVIATION is the float32 restatement's largest deviation from the float64 one over the GPU test's inputs, as
    measured (another numpy build may sum the contrast mean in another shape: the recording is held to 1 % of what this run
    measures), JITTER_TOL four times that"""
    worst = measured_deviation()
    print(f"float32 vs float64 restatement: max deviation {worst:.3e}; recorded {ref.JITTER_F32_DEVIATION:.3e}, tolerance {ref.JITTER_TOL:.3e}")
    assert abs(worst - ref.JITTER_F32_DEVIATION) <= 0.01 * ref.JITTER_F32_DEVIATION
    assert ref.JITTER_TOL == 4 * ref.JITTER_F32_DEVIATION
