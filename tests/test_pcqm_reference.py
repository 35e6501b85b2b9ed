"""The numpy restatement of the voxel-grid PCQM stand-in (tests/_pcqm_reference.py) against the definition itself, and the
colour conversion of pcc_amd/pcqm.py.  No GPU."""
import numpy as np
import torch

import _pcqm_reference as ref


def test_restatement_equals_brute_force_on_the_tiny_cloud():
    R, D = ref.tiny_pair()
    assert len(R) <= 300 and len(D) <= 300
    r_xyz, d_xyz = R[:, :3].astype(np.int64), D[:, :3].astype(np.int64)
    nn = ref.nearest(r_xyz, d_xyz)
    for radius, h in ((1, 2), (2, 3)):
        ar, ad = ref.attributes(R, radius), ref.attributes(D, radius)
        w = ref.gaussian_weights(h)
        fast = ref.stats(r_xyz, ar, d_xyz, ad, nn, h, w)
        slow = ref.brute_stats(r_xyz, ar, d_xyz, ad, nn, h, w)
        scale = np.maximum(np.abs(slow), 1.0)
        assert (np.abs(fast - slow) / scale).max() <= 1e-13
        assert np.abs(ref.features(fast) - ref.features(slow)).max() <= 1e-13
        assert (fast[:, 12:14] > 0).any() and (fast[:, 15:17] > 0).any()      # both variances are exercised


def test_identical_clouds_give_every_feature_exactly_zero():
    R, _ = ref.shell_pair()
    for radius, h in ((1, 2), (2, 3)):
        total, pooled, f = ref.score(R, R, radius, h)
        assert not f.any() and not pooled.any() and total == 0.0


def test_constant_colour_plane():
    P = ref.plane()
    xyz = P[:, :3].astype(np.int64)
    attrs = ref.attributes(P, 3)
    nn = np.arange(len(P))
    st = ref.stats(xyz, attrs, xyz, attrs, nn, 3, np.ones(10))
    f = ref.features(st)
    assert not f[:, :5].any()
    interior = ((xyz[:, :2] >= 3) & (xyz[:, :2] <= 12)).all(1)
    assert (st[interior, 0] == 29).all() and (st[interior, 1] == 29).all()
    count, _ = ref.nref.ball_moments(xyz, np.zeros(len(xyz), np.int64), 3)
    assert np.array_equal(st[:, 0], count.astype(np.float64))
    # a plane of another colour: the colour features move; lightness contrast and structure (constant on both sides) stay at 0
    # up to the two-pass mean's own rounding (the mean of 29 equal numbers need not be that number), under a square root
    other = ref.attributes(np.concatenate([P[:, :3], np.tile([[0.6, 0.3, 0.3]], (256, 1))], axis=1), 3)
    g = ref.features(ref.stats(xyz, attrs, xyz, other, nn, 3, np.ones(10)))
    assert (g[:, 0] > 0).all() and np.abs(g[:, 1:3]).max() <= 1e-6 and (g[:, 3] > 0).all()


def test_lab_planes_white_and_black(pcc):
    from pcc_amd.pcqm import lab_planes
    lab = lab_planes(torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], dtype=torch.float64)).numpy()
    assert lab.shape == (2, 4) and lab.dtype == np.float64
    assert np.abs(lab[0] - [100.0, 0.0, 0.0, 0.0]).max() <= 1e-9
    assert np.abs(lab[1]).max() <= 1e-9


def test_lab_planes_match_the_restatement(pcc):
    from pcc_amd.pcqm import lab_planes
    rgb = np.random.default_rng(2).random((4096, 3))
    got = lab_planes(torch.from_numpy(rgb)).numpy()
    want = ref.lab_planes(rgb)
    assert np.abs(got - want).max() <= 1e-9
    assert 0.0 <= got[:, 0].min() and got[:, 0].max() <= 100.0 and (got[:, 1] >= 0).all()
    grey = lab_planes(torch.full((1, 3), 128 / 255, dtype=torch.float64)).numpy()[0]
    assert abs(grey[0] - 53.585) < 1e-2 and np.abs(grey[1:]).max() <= 1e-9      # CIELAB L* of sRGB mid grey


def test_more_colour_noise_scores_worse_in_the_restatement():
    scores = [ref.score(ref.shell_pair(0)[0], ref.shell_pair(noise)[1], 1, 2)[0] for noise in (4, 12, 36)]
    print("restatement pcqm_voxel at +-4 / 12 / 36 levels:", scores)
    assert 0.0 < scores[0] < scores[1] < scores[2]


def test_default_radii(pcc):
    from pcc_amd.pcqm import default_radii
    R, _ = ref.shell_pair()
    coords = torch.cat([torch.zeros((len(R), 1), dtype=torch.int32), torch.from_numpy(R[:, :3]).to(torch.int32)], dim=1)
    assert default_radii(coords) == (1, 2)
    big = torch.tensor([[0, 0, 0, 0], [0, 1000, 10, 10]], dtype=torch.int32)
    assert default_radii(big) == (4, 8)
    assert default_radii(torch.tensor([[0, 0, 0, 0], [0, 1023, 0, 0]], dtype=torch.int32)) == (4, 8)
