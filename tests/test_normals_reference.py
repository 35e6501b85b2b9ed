"""The numpy restatement of the surface normals (tests/_normals_reference.py) checked against geometry whose normals are known:
the yardstick of tests/test_normals.py, tests/test_d2_metric.py and tests/test_facing_map.py.  Runs without a GPU."""
import math

import numpy as np
import pytest

import _normals_reference as ref


@pytest.fixture(scope="module")
def shell3(pcc):
    pts = ref.shell(32, 11, 0.875)
    count, moments = ref.ball_moments(pts, np.zeros(len(pts), np.int64), 3)
    return pts, count, moments, ref.reference_normals(count, moments)


def test_ball_offsets_are_the_lattice_points_of_the_ball():
    assert [len(ref.ball_offsets(R)) for R in (1, 2, 3, 8)] == [7, 33, 123, 2109]


def test_shell_normals_are_radial(shell3):
    pts, count, moments, (normals, valid, gap) = shell3
    assert pts.shape == (2816, 3)
    assert valid.all() and count.min() >= 3
    assert gap.min() >= 0.05                                  # no point near a degenerate smallest eigenvalue
    radial = pts - 15.5
    radial = radial / np.linalg.norm(radial, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip(np.abs((normals * radial).sum(1)), 0.0, 1.0)))
    print("shell R=3: median %.2f deg, 99th percentile %.2f deg, smallest gap %.3f" % (np.median(angle), np.percentile(angle, 99), gap.min()))
    assert np.median(angle) < 5.0 and np.percentile(angle, 99) < 15.0
    assert np.abs(np.linalg.norm(normals, axis=1) - 1.0).max() <= 1e-12


def test_thin_shell_has_no_point_below_the_gap(pcc):
    pts = ref.shell(64, 25, 0.5)
    assert pts.shape == (7832, 3)
    count, moments = ref.ball_moments(pts, np.zeros(len(pts), np.int64), 3)
    _, valid, gap = ref.reference_normals(count, moments)
    assert valid.all() and gap.min() >= 0.05


def test_moments_of_a_hand_counted_neighbourhood():
    """an L of three voxels: (0,0,0), (1,0,0), (0,1,0) at R = 1"""
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    count, moments = ref.ball_moments(pts, np.zeros(3, np.int64), 1)
    assert count.tolist() == [3, 2, 2]
    # the corner: offsets (0,0,0), (1,0,0), (0,1,0) -> S1 = (1,1,0), S2 = diag(1,1,0): M = 3 S2 - S1 S1^T
    assert moments[0].tolist() == [2, -1, 0, 2, 0, 0]
    assert ref.validity(count, moments).tolist() == [True, False, False]
    normals, _, _ = ref.reference_normals(count, moments)
    assert np.array_equal(np.abs(normals[0]), [0.0, 0.0, 1.0]) and not normals[1:].any()


def test_plane_normals_are_exact():
    g = np.arange(16)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    pts = np.concatenate([pts, np.full((256, 1), 5)], axis=1)
    count, moments = ref.ball_moments(pts, np.zeros(256, np.int64), 3)
    assert not moments[:, [2, 4, 5]].any()                    # M's z row and column are zero
    normals, valid, _ = ref.reference_normals(count, moments)
    assert valid.all()
    interior = ((pts[:, :2] >= 3) & (pts[:, :2] <= 12)).all(1)
    assert count[interior].min() == count[interior].max() == 29
    assert np.array_equal(np.abs(normals[interior]), np.tile([0.0, 0.0, 1.0], (interior.sum(), 1)))


def test_points_on_one_line_have_no_normal():
    for step in ([1, 0, 0], [1, 1, 0], [1, 1, 1]):
        pts = np.arange(10)[:, None] * np.array(step)[None, :]
        count, moments = ref.ball_moments(pts, np.zeros(10, np.int64), 3)
        normals, valid, gap = ref.reference_normals(count, moments)
        assert count.min() >= 2 and not valid.any() and not normals.any() and np.isinf(gap).all()


def test_batch_items_do_not_see_each_other():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]])
    count, _ = ref.ball_moments(pts, np.array([0, 0, 0, 1, 1]), 1)
    assert count.tolist() == [3, 2, 2, 1, 1]


def test_random_cloud_touches_the_origin_and_holds_both_kinds(pcc):
    pts = ref.random_cloud()
    assert pts.shape == (500, 3) and len(np.unique(pts, axis=0)) == 500 and not pts[0].any() and pts.min() == 0 and pts.max() <= 11
    count, moments = ref.ball_moments(pts, np.zeros(500, np.int64), 2)
    valid = ref.validity(count, moments)
    assert (count < 3).any() and ((count >= 3) & ~valid).any() and valid.any()      # isolated or paired, collinear, and valid points


def test_reference_d2_and_facing_on_known_cases():
    g = np.arange(8)
    plane = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    a = np.concatenate([plane, np.zeros((64, 1), np.int64)], axis=1)
    n = np.tile([0.0, 0.0, 1.0], (64, 1))
    same = ref.reference_d2(a, a, n, 7)
    assert same["sym_d2_mse"] == 0.0 and same["sym_d2_psnr"] == math.inf
    lifted = ref.reference_d2(a, a + [0, 0, 2], n, 7)          # along the normal: D2 = D1 = 4 / 3
    assert lifted["AB_d2_mse"] == lifted["BA_d2_mse"] == 4.0 / 3.0
    assert lifted["sym_d2_psnr"] == 10 * math.log10(49.0 / (4.0 / 3.0))
    slid = ref.reference_d2(a, np.concatenate([a, a[-8:] + [1, 0, 0]]), n, 7)      # a row added in the plane: no D2 error
    assert slid["sym_d2_mse"] == 0.0
    none = ref.reference_d2(a, a + [0, 0, 2], np.zeros((64, 3)), 7)                # no normals: the full distance
    assert none["AB_d2_mse"] == 4.0 / 3.0
    f = ref.reference_facing(a, n, 0.5, 1.0, direction=(0, 0, 3))
    assert f.dtype == np.float32 and np.array_equal(f, np.tile(np.float32([0.5, 1.0]), (64, 1)))
    f = ref.reference_facing(a, n, 0.5, 1.0, direction=(1, 0, 0), floor=0.25)
    assert np.array_equal(f, np.tile(np.float32([0.125, 0.25]), (64, 1)))
    f = ref.reference_facing(a, np.zeros((64, 3)), 0.5, 1.0, camera=(0, 0, 9))
    assert np.array_equal(f, np.tile(np.float32([0.5, 1.0]), (64, 1)))
    f = ref.reference_facing(np.array([[3, 0, 0]]), np.array([[0.0, 0.0, 1.0]]), 1.0, 1.0, camera=(0, 0, 4))
    assert abs(float(f[0, 0]) - 0.8) <= 1e-7                   # the ray (-3, 0, 4) / 5
