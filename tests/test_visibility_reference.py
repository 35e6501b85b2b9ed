"""The parts of the visibility feature that need no GPU: the numpy reference (tests/_visibility_reference.py) against the
definition by brute force, q_map.visibility_score / visibility_map on CPU tensors against the formula in numpy float64 (bit
for bit: both are IEEE float64 elementwise), and every ValueError of render.visibility and the score, raised before any
library call."""
import itertools
import types

import numpy as np
import pytest
import torch

import _view_reference as vref
import _visibility_reference as ref

FRONT, SIDE, BACK = ((0, 0, 1), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))


def brute_force(xyz, front, up, H, W, frame, ps):
    """the definition, pixel by pixel: (behind, covered pixels, largest depth per pixel or None)"""
    r, u, f = vref.axes(front, up)
    u_min, _, _, v_max, scale, ox, oy = frame
    pixels = []                                             # per point: the in-image pixels of its splat
    top = {}
    for p in xyz:
        c0, r0, d = (int(p @ r) - u_min) * scale + ox, (v_max - int(p @ u)) * scale + oy, int(p @ f)
        mine = [(r0 + j, c0 + i) for j in range(ps) for i in range(ps) if 0 <= r0 + j < H and 0 <= c0 + i < W]
        pixels.append((mine, d))
        for px in mine:
            top[px] = max(top.get(px, d), d)
    behind = np.array([min((top[px] - d for px in mine), default=ref.OFFSCREEN) for mine, d in pixels], dtype=np.int64)
    return behind, len(top)


@pytest.mark.parametrize("scale,extra", list(itertools.product((1, 2), ("one", "scale", "scale+1"))))
def test_reference_against_the_definition(scale, extra):
    ps = {"one": 1, "scale": scale, "scale+1": scale + 1}[extra]
    rng = np.random.default_rng(100 * scale + ps)
    xyz = np.unique(rng.integers(0, 12, size=(200, 3)), axis=0)
    assert 150 < xyz.shape[0] <= 200                           # np.unique leaves them in canonical order
    for view in (FRONT, SIDE, ((0, -1, 0), (0, 0, 1))):
        H, W = 12 * scale + 3, 12 * scale + 5
        own = vref.frame_of(xyz, view[0], view[1], H, W, scale=scale)
        clipped = (own[0] + 3, own[1], own[2], own[3] - 4, scale, -1, -2)       # cut at the left and at the top, and by the size
        for frame, h, w in ((own, H, W), (clipped, 7 * scale, 6 * scale)):
            behind, won = ref.view_visibility(xyz, view[0], view[1], h, w, frame, ps)
            want, covered = brute_force(xyz, view[0], view[1], h, w, frame, ps)
            assert np.array_equal(behind, want)
            assert int(won.sum()) == covered and covered > 0
            assert (behind[won > 0] == 0).all() and (behind >= 0).all()
            assert (won[behind == ref.OFFSCREEN] == 0).all()
        assert (behind == ref.OFFSCREEN).any() and (behind == 0).any() and ((behind > 0) & (behind < ref.OFFSCREEN)).any()


def test_reference_in_any_row_order_and_over_views():
    rng = np.random.default_rng(5)
    xyz = np.unique(rng.integers(0, 12, size=(200, 3)), axis=0)
    b1, w1 = ref.visibility(xyz, [FRONT], 30, 30, point_size=3)
    b2, w2 = ref.visibility(xyz, [BACK], 30, 30, point_size=3)
    perm = rng.permutation(xyz.shape[0])
    b, w = ref.visibility(xyz[perm], [FRONT, BACK], 30, 30, point_size=3)
    assert np.array_equal(b, np.minimum(b1, b2)[perm]) and np.array_equal(w, (w1 + w2)[perm])
    # a row beyond the coordinate range draws nothing and hides nothing
    rows = np.array([[0, 0, 0], [0, 0, 5], [0, 0, ref.COORD_LIMIT + 1]])
    b, w = ref.view_visibility(rows, FRONT[0], FRONT[1], 4, 4, (0, 0, 0, 0, 1, 1, 1))
    assert b.tolist() == [5, 0, ref.OFFSCREEN] and w.tolist() == [0, 1, 0]


def test_reference_counts_on_the_config1_shell(pcc):
    """the counts of the definition's prototype on the 4,904-point shell: front view, every voxel its own scale x scale square"""
    from pcc_amd import synthetic as syn
    xyz = syn.sphere_shell(**syn.CONFIG1)[:, :3].astype(np.int64)
    assert xyz.shape[0] == 4904
    behind, won = ref.visibility(xyz, [FRONT], 160, 96)
    assert (int((behind == 0).sum()), int((behind <= 2).sum()), int((behind == ref.OFFSCREEN).sum())) == (788, 2012, 0)
    assert np.array_equal(won > 0, behind == 0) and int(won.sum()) == 788 * 9          # scale 3, no overlap: nine pixels each
    both, _ = ref.visibility(xyz, [FRONT, BACK], 160, 96)
    assert int((both <= 2).sum()) == 3992
    small, _ = ref.visibility(xyz, [FRONT], 40, 40)                                   # scale 1: the same depths
    assert np.array_equal(small, behind)


TOL, FALL = 2, 8


@pytest.mark.parametrize("falloff", [0, 1, 8])
@pytest.mark.parametrize("floor", [0.0, 0.25, 1.0])
def test_visibility_score_is_the_formula(pcc, falloff, floor):
    from pcc_amd import q_map, render
    assert render.OFFSCREEN == ref.OFFSCREEN == 2147483647
    for tol in (0, TOL, 3):
        values = [0, 1, tol, tol + 1, tol + falloff, tol + falloff + 1, ref.OFFSCREEN]
        for dtype in (torch.int32, torch.int64):
            got = q_map.visibility_score(torch.tensor(values, dtype=dtype), tolerance=tol, falloff=falloff, floor=floor)
            assert got.dtype == torch.float64 and got.device.type == "cpu"
            assert got.numpy().tobytes() == ref.score(values, tol, falloff, floor).tobytes()
        # the formula, spelt out per value
        for b, s in zip(values, got.tolist()):
            hidden = max(b - tol, 0)
            w = 0.0 if b == ref.OFFSCREEN else (1.0 if hidden == 0 else (max(0.0, 1.0 - hidden / falloff) if falloff > 0 else 0.0))
            assert s == floor + (1.0 - floor) * w
    d = q_map.visibility_score(torch.tensor([0, 2, 3, 6, 10, 11], dtype=torch.int32))           # the defaults: 2 and 8
    assert d.tolist() == [1.0, 1.0, 0.875, 0.5, 0.0, 0.0]


def test_visibility_map_channels(pcc):
    from pcc_amd import q_map
    rng = np.random.default_rng(2)
    xyz = np.unique(rng.integers(0, 9, size=(60, 3)), axis=0)
    n = xyz.shape[0]
    coords = torch.from_numpy(np.concatenate([np.zeros((n, 1), dtype=np.int64), xyz], axis=1)).to(torch.int32)
    # a CoordMap lives on the GPU; the builder reads only the map's row count and device, which this stands in for
    cmap = types.SimpleNamespace(n=n, device=coords.device, coords=coords)
    behind = rng.integers(0, 14, size=n)
    behind[::7] = ref.OFFSCREEN
    for floor, falloff in ((0.0, 8), (0.25, 3), (1.0, 0)):
        Q = q_map.visibility_map(cmap, torch.from_numpy(behind).to(torch.int32), 0.4, 0.8, tolerance=1, falloff=falloff, floor=floor)
        s = ref.score(behind, 1, falloff, floor)
        want = np.stack([0.4 * s, 0.8 * s], axis=1).astype(np.float32)
        assert Q.F.dtype == torch.float32 and Q.F.numpy().tobytes() == want.tobytes()
        assert Q.map is cmap
    with pytest.raises(ValueError):
        q_map.visibility_map(cmap, torch.zeros(n + 1, dtype=torch.int32), 0.4, 0.8)


def test_score_refusals(pcc):
    from pcc_amd import q_map
    b = torch.zeros(3, dtype=torch.int32)
    for kw in ({"tolerance": -1}, {"falloff": -1}, {"floor": -0.01}, {"floor": 1.01}, {"floor": float("nan")}):
        with pytest.raises(ValueError):
            q_map.visibility_score(b, **kw)
    with pytest.raises(ValueError):
        q_map.visibility_score(torch.zeros(3, dtype=torch.float32))


def test_visibility_refusals_need_no_gpu(pcc):
    """every ValueError of render.visibility is raised before the library is asked for anything"""
    from pcc_amd import render
    cloud = torch.tensor([[0, 0, 0], [1, 2, 3]], dtype=torch.float32)
    bad_views = [[], (), "front", None, ["top"], [((0, 0, 1),)], [((0, 0, 1), (0, 0, 1))], [((0, 0, 2), (0, 1, 0))],
                 [((0, 0.5, 1), (0, 1, 0))], [3], ["front", ((1, 1, 0), (0, 0, 1))]]
    for views in bad_views:
        with pytest.raises(ValueError):
            render.visibility(cloud, views, 16, 16)
    frame = render.view_frame(cloud, FRONT[0], FRONT[1], 16, 16)
    for frames in ([], [frame, frame], frame, [frame[:6]]):
        with pytest.raises(ValueError):
            render.visibility(cloud, ["front"], 16, 16, frames=frames)
    with pytest.raises(ValueError):
        render.visibility(cloud, ["front", "side"], 16, 16, frames=[frame])
    with pytest.raises(ValueError):
        render.visibility(cloud + 0.5, ["front"], 16, 16)                     # not voxelised
    with pytest.raises(ValueError):
        render.visibility(torch.zeros((4, 2)), ["front"], 16, 16)            # no z column
    for H, W in ((0, 16), (16, 0), (8193, 16), (16, -1)):
        with pytest.raises(ValueError):
            render.visibility(cloud, ["front"], H, W)
    with pytest.raises(ValueError):
        render.visibility(cloud, ["front"], 16, 16, device="cpu")
    far = cloud.clone()
    far[0, 2] = render.COORD_LIMIT + 1
    with pytest.raises(ValueError):
        render.visibility(far, ["front"], 16, 16, device="cuda:0")
