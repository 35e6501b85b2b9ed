"""The parts of the camera views that need no GPU.  The restatement (tests/_camera_reference.py) is held to facts worked out by
hand that do not share its formulas (where a point on the axis lands, pixels per voxel at a depth, who wins on a ray, the near
plane, the splat sizes, rounding of negative offsets, invariance under integer translations and the 24 axis rotations);
render.Camera's quantisation, q_map.distance_score and every ValueError run on the host; and the inputs of the GPU cases
(tests/test_camera.py) are shown to exercise what they are there for."""
import itertools
import types

import numpy as np
import pytest
import torch

import _camera_reference as ref

FRONT, UP = (0, 0, 1), (0, 1, 0)


def cam_z(z, focal, H, W, near=1.0):
    """on the +z axis at (0, 0, z), looking at the origin: right = +x, up = +y"""
    return ref.quantise((0, 0, z), front=FRONT, up=UP, focal=focal, H=H, W=W, near=near)


def spot(p, cam, ps_q=16):
    """(first column, first row, size) of a drawn point"""
    return ref.project(p, cam, ps_q)[:3]


def test_axis_point_lands_on_the_centre():
    # depth 100 voxels, focal 50 px: a voxel is half a pixel -> one pixel, the centre one of an odd image
    assert spot((0, 0, 0), cam_z(100, 50, 65, 33)) == (16, 32, 1)
    # focal 150: 1.5 px -> two pixels, the two centre columns and rows of an even image
    assert spot((0, 0, 0), cam_z(100, 150, 64, 32)) == (15, 31, 2)
    key, winner, behind, won, depth = ref.paint([(0, 0, 0)], cam_z(100, 150, 64, 32))
    assert np.argwhere(winner == 0).tolist() == [[31, 15], [31, 16], [32, 15], [32, 16]]
    assert behind.tolist() == [0] and won.tolist() == [4] and depth.tolist() == [100 * 256]


@pytest.mark.parametrize("focal,per_voxel", [(50, 0.5), (100, 1.0)])
def test_offsets_scale_with_focal_over_depth(focal, per_voxel):
    """at depth 100 a voxel step is focal / 100 pixels: right is a larger column, up a smaller row; doubling focal doubles both"""
    cam = cam_z(100, focal, 65, 65)
    for k in (-6, -2, 0, 2, 4, 10):
        assert spot((k, 0, 0), cam)[:2] == (32 + int(k * per_voxel), 32)
        assert spot((0, k, 0), cam)[:2] == (32, 32 - int(k * per_voxel))
    # the same pixel offset at half the depth needs half the displacement
    # the same offset from the principal point at half the depth needs half the displacement (the splat there is twice as wide)
    assert ref.project((2, 0, 50), cam)[4] == ref.project((4, 0, 0), cam)[4] == int(4 * per_voxel * 16)


def test_nearer_point_on_a_ray_wins():
    cam = cam_z(100, 50, 65, 65)
    rows = [(0, 0, 0), (0, 0, 50), (4, 0, 0), (2, 0, 50)]               # two rays, the nearer point second on each
    key, winner, behind, won, depth = ref.paint(rows, cam)
    assert winner[32, 32] == 1 and winner[32, 34] == 3 and int((winner >= 0).sum()) == 2
    assert behind.tolist() == [50, 0, 50, 0] and won.tolist() == [0, 1, 0, 1] and depth.tolist() == [25600, 12800, 25600, 12800]
    assert key[32, 32] == 12800
    # equal depth keys: the lowest row wins whatever comes later
    key, winner, behind, won, _ = ref.paint([(0, 0, 0), (0, 0, 0)], cam)
    assert winner[32, 32] == 0 and behind.tolist() == [0, 0] and won.tolist() == [1, 0]


def test_near_plane_and_behind_the_camera():
    cam = cam_z(100, 50, 65, 65, near=10.0)
    assert ref.project((0, 0, 90), cam) is not None                       # D == near exactly: drawn
    assert ref.project((0, 0, 91), cam) is None
    pos_q, axes_q, focal_q, near_q, H, W = cam
    one_step = ((0, 0, pos_q[2] - 1), axes_q, focal_q, near_q, H, W)      # the camera a sixteenth of a voxel nearer
    assert ref.project((0, 0, 90), one_step) is None and ref.project((0, 0, 89), one_step) is not None
    assert ref.project((0, 0, 100), cam) is None and ref.project((0, 0, 150), cam) is None      # at and behind the camera
    _, _, behind, won, depth = ref.paint([(0, 0, 150), (0, 0, 0)], cam)
    assert behind.tolist() == [ref.OFFSCREEN, 0] and won.tolist() == [0, 1] and depth.tolist() == [ref.OFFSCREEN, 25600]


def test_splat_sizes_and_both_clamps():
    assert spot((0, 0, 0), cam_z(100, 0.1, 65, 65))[2] == 1               # a thousandth of a pixel: clamped up to 1
    assert spot((0, 0, 0), cam_z(100, 50, 65, 65))[2] == 1
    assert spot((0, 0, 0), cam_z(100, 150, 65, 65))[2] == 2
    assert spot((0, 0, 0), cam_z(100, 200, 65, 65))[2] == 2               # exactly 2 px stays 2 ...
    q = list(cam_z(100, 200, 65, 65))
    q[2] += 1                                                             # ... and a sixteenth of a pixel more focal makes it 3
    assert spot((0, 0, 0), tuple(q))[2] == 3
    assert spot((0, 0, 0), cam_z(100, 1600, 65, 65))[2] == 16
    assert spot((0, 0, 0), cam_z(100, 4000, 65, 65))[2] == 16             # 40 px: clamped down to 16
    # point_size scales the edge: half a pixel per voxel, edges of 0.5 / 3 voxels
    cam = cam_z(100, 50, 65, 65)
    assert spot((0, 0, 0), cam, ref.ps_q_of(0.5))[2] == 1 and spot((0, 0, 0), cam, ref.ps_q_of(3))[2] == 2
    # a 16-pixel splat is centred: 8 columns each side of the centre line of an even image
    assert spot((0, 0, 0), cam_z(100, 1600, 64, 64)) == (24, 24, 16)


def test_negative_offsets_round_down():
    """depth 1000, focal 50: one voxel is 0.8 sixteenths of a pixel.  A voxel LEFT of the axis has X = floor(-0.8) = -1: its
    pixel-wide splat starts at (8 * 65 - 1 - 8) / 16 = 31.94 -> column 31, where rounding towards zero (X = 0) would say 32.  Y is
    floored before it is negated: 19 voxels BELOW the axis Y = floor(-15.2) = -16, the splat starts at (520 + 16 - 8) / 16 = 33 ->
    row 33, where rounding towards zero (Y = -15, 32.94) would say 32"""
    cam = cam_z(1000, 50, 65, 65)
    assert spot((-1, 0, 0), cam)[:2] == (31, 32) and spot((1, 0, 0), cam)[:2] == (32, 32)
    assert spot((0, -19, 0), cam)[:2] == (32, 33) and spot((0, 19, 0), cam)[:2] == (32, 31)
    pr = ref.project((-1, -1, 0), cam)
    assert pr[4:6] == (-1, -1)                                            # X, Y: -0.8 sixteenths, floored
    cam = cam_z(96, 50, 65, 65)
    assert ref.project((-1, -1, 0), cam)[4:6] == (-9, -9)                 # -800 / 96 = -8.33
    assert ref.project((1, 1, 0), cam)[4:6] == (8, 8)


def cloud_and_camera():
    xyz = ref.exactly(300, 16, 3)
    cam = ref.quantise((40, -25, 60), look_at=(8, 8, 8), fov_y=35, H=40, W=36)
    return xyz, cam


def test_integer_translation_changes_nothing():
    xyz, cam = cloud_and_camera()
    want = ref.paint(xyz, cam, 48)
    assert (want[1] >= 0).sum() > 50 and (want[2] > 0).any()
    for t in ((5, 0, 0), (-300, 17, 1234), (100000, -100000, 7)):
        moved = ((cam[0][0] + 16 * t[0], cam[0][1] + 16 * t[1], cam[0][2] + 16 * t[2]),) + cam[1:]
        got = ref.paint(xyz + np.array(t), moved, 48)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def rotations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            R = np.zeros((3, 3), dtype=np.int64)
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    return out


def test_the_24_axis_rotations_change_nothing():
    """rotating the cloud and an axis-aligned camera together: integer arithmetic, so the result is the same to the last bit"""
    R24 = rotations()
    assert len(R24) == 24
    xyz = ref.exactly(300, 16, 4) - 8
    cam = ref.quantise((3, -2, 40), front=FRONT, up=UP, focal=37.3, H=41, W=36, near=38.0)      # the near plane cuts the cloud
    assert cam[1] == ((16384, 0, 0), (0, 16384, 0), (0, 0, 16384))
    want = ref.paint(xyz, cam, 40)
    assert (want[2] == ref.OFFSCREEN).any() and (want[2] > 0).any() and (want[3] > 1).any()
    for R in R24:
        turned = (tuple((R @ np.array(cam[0])).tolist()), tuple(tuple((R @ np.array(a)).tolist()) for a in cam[1])) + cam[2:]
        got = ref.paint(xyz @ R.T, turned, 40)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_camera_quantisation(pcc):
    from pcc_amd import render
    cam = render.Camera((0, 0, 10), look_at=(0, 0, 0), fov_y=90, H=100, W=60)
    q = cam.quantised()
    assert q == ((0, 0, 160), ((16384, 0, 0), (0, 16384, 0), (0, 0, 16384)), 800, 16, 100, 60)       # tan 45 = 1: focal 50
    assert (q.pos_q, q.focal_q, q.near_q, q.H, q.W) == ((0, 0, 160), 800, 16, 100, 60)
    for front, up in ref.AXIS_VIEWS:                                     # axis-aligned cameras are exact
        q = render.Camera((1, 2, 3), front=front, up=up, focal=10, H=8, W=8).quantised()
        r = tuple(int(v) for v in np.cross(up, front))
        assert q.axes_q == (tuple(16384 * v for v in r), tuple(16384 * v for v in up), tuple(16384 * v for v in front))
    # a 3-4-5 triangle: front (0.6, 0, 0.8), right = up x front = (0.8, 0, -0.6), up stays
    q = render.Camera((3, 0, 4), look_at=(0, 0, 0), focal=12.5, H=8, W=8, near=0.25).quantised()
    assert q.axes_q == ((13107, 0, -9830), (0, 16384, 0), (9830, 0, 13107)) and q.pos_q == (48, 0, 64) and (q.focal_q, q.near_q) == (200, 4)
    # a tilted up is made orthogonal to front
    assert render.Camera((0, 0, 5), front=(0, 0, 2), up=(0, 1, 1), focal=1, H=8, W=8).quantised().axes_q[1] == (0, 16384, 0)
    assert render.Camera((0, 0, 5), front=FRONT, fov_y=60, H=64, W=8).quantised().focal_q == int(np.rint(16 * 32 / np.tan(np.pi / 6)))
    # the restatement's own conversion agrees on an oblique camera, and from_quantised closes the loop
    cam = render.Camera((300, -200, 500), look_at=ref.CENTRE, fov_y=40, H=128, W=96)
    assert tuple(cam.quantised()) == ref.oblique_camera()
    again = render.Camera.from_quantised(*cam.quantised())
    assert again.quantised() == cam.quantised() and again.H == 128 and abs(again.focal - cam.focal) <= 1 / 32


def test_camera_refusals(pcc):
    from pcc_amd import render
    ok = dict(position=(0, 0, 10), front=FRONT, focal=10, H=8, W=8)
    render.Camera(**ok)
    bad = [dict(look_at=(0, 0, 0)), dict(front=None), dict(fov_y=30), dict(focal=None), dict(up=(0, 0, 1)), dict(up=(0, 0, -3)),
           dict(up=(0, 0, 0)), dict(front=(0, 0, 0)), dict(position=(2 ** 20 + 1, 0, 0)), dict(position=(0, float("nan"), 0)),
           dict(focal=0.01), dict(focal=2 ** 16 + 1), dict(focal=float("inf")), dict(near=0.0), dict(near=-1), dict(H=0), dict(W=8193),
           dict(H=None), dict(H=7.5), dict(focal=None, fov_y=0), dict(focal=None, fov_y=180), dict(position=(0, 0))]
    for kw in bad:
        with pytest.raises(ValueError):
            render.Camera(**dict(ok, **kw))
    with pytest.raises(ValueError):
        render.Camera((0, 0, 10), look_at=(0, 0, 10), focal=10, H=8, W=8)                 # looks at itself
    q = render.Camera(**ok).quantised()
    axes = [list(r) for r in q.axes_q]
    axes[0][0] = 2 ** 14 + 1
    for args in ((q.pos_q, axes, q.focal_q, q.near_q, 8, 8), ((2 ** 24 + 1, 0, 0), q.axes_q, q.focal_q, q.near_q, 8, 8),
                 (q.pos_q, q.axes_q, 0, q.near_q, 8, 8), (q.pos_q, q.axes_q, 2 ** 20 + 1, q.near_q, 8, 8), (q.pos_q, q.axes_q, 16, 0, 8, 8),
                 (q.pos_q, q.axes_q, 16, 16, 8, 0), (q.pos_q, q.axes_q[:2], 16, 16, 8, 8), (q.pos_q, q.axes_q, 16.5, 16, 8, 8)):
        with pytest.raises(ValueError):
            render.Camera.from_quantised(*args)
    assert render.Camera.from_quantised((2 ** 24, 0, 0), q.axes_q, 2 ** 20, 1, 8192, 1).quantised().focal_q == 2 ** 20


def test_operator_refusals_need_no_gpu(pcc):
    """every ValueError of render_camera / camera_visibility is raised before the library is asked for anything"""
    from pcc_amd import render
    cam = render.Camera((0, 0, 10), front=FRONT, focal=10, H=8, W=8)
    cloud = torch.tensor([[0, 0, 0, 0.5, 0.5, 0.5], [1, 2, 3, 0.1, 0.2, 0.3]], dtype=torch.float32)
    for cameras in ([], (), cam, None, [cam, "front"], [ref.oblique_camera()]):
        with pytest.raises(ValueError):
            render.camera_visibility(cloud, cameras)
    with pytest.raises(ValueError):
        render.camera_visibility(cloud + 0.5, [cam])                     # not voxelised
    with pytest.raises(ValueError):
        render.render_camera(cloud + 0.5, cam)
    with pytest.raises(ValueError):
        render.render_camera(cloud, ref.oblique_camera())                # the integers alone are no Camera
    with pytest.raises(ValueError):
        render.render_camera(cloud[:, :3], cam)                          # no colours
    for ps in (0, -1, 16.5, 0.01, float("nan"), None):
        with pytest.raises(ValueError):
            render.render_camera(cloud, cam, point_size=ps)
        with pytest.raises(ValueError):
            render.camera_visibility(cloud, [cam], point_size=ps)
    with pytest.raises(ValueError):
        render.render_camera(cloud, cam, device="cpu")
    with pytest.raises(ValueError):
        render.camera_visibility(cloud, [cam], device="cpu")
    with pytest.raises(ValueError):
        render.render_camera(cloud, cam, background=(0, 0, 256), device="cuda:0")
    far = cloud.clone()
    far[0, 2] = render.COORD_LIMIT + 1
    with pytest.raises(ValueError):
        render.camera_visibility(far, [cam], device="cuda:0")


@pytest.mark.parametrize("full,floor", [(1.0, 0.0), (2.0, 0.25), (0.5, 1.0)])
def test_distance_score_is_the_formula(pcc, full, floor):
    from pcc_amd import q_map
    focal = 175.83
    depth = np.array([16, 255, 256, 257, 45000, 45013, 90026, 2 ** 30 - 1, ref.OFFSCREEN], dtype=np.int64)
    want = np.where(depth == ref.OFFSCREEN, 0.0, np.clip((focal * 256.0 / depth.astype(np.float64)) / full, floor, 1.0))
    assert ref.distance_score(depth, focal, full, floor).tobytes() == want.tobytes()
    for dtype in (torch.int32, torch.int64):
        got = q_map.distance_score(torch.from_numpy(depth).to(dtype), focal, full=full, floor=floor)
        assert got.dtype == torch.float64 and got.numpy().tobytes() == want.tobytes()
    assert got[-1] == 0.0 and got[0] == 1.0
    # a voxel seen at exactly `full` pixels scores 1, at half of it a half
    assert q_map.distance_score(torch.tensor([256 * 100, 256 * 200, 256 * 400]), 100.0).tolist() == [1.0, 0.5, 0.25]
    for kw in (dict(focal=0), dict(full=0), dict(floor=-0.1), dict(floor=1.5)):
        with pytest.raises(ValueError):
            q_map.distance_score(torch.tensor([256]), **dict(dict(focal=10.0), **kw))
    with pytest.raises(ValueError):
        q_map.distance_score(torch.tensor([256.0]), 10.0)
    with pytest.raises(ValueError):
        q_map.distance_score(torch.tensor([0]), 10.0)
    n = 5
    cmap = types.SimpleNamespace(n=n, device=torch.device("cpu"), coords=torch.zeros((n, 4), dtype=torch.int32))
    d5 = torch.from_numpy(depth[:n]).to(torch.int32)
    Q = q_map.distance_map(cmap, d5, focal, 0.4, 0.8, full=full, floor=floor)
    s = ref.distance_score(depth[:n], focal, full, floor)
    assert Q.F.dtype == torch.float32 and Q.F.numpy().tobytes() == np.stack([0.4 * s, 0.8 * s], axis=1).astype(np.float32).tobytes()
    with pytest.raises(ValueError):
        q_map.distance_map(cmap, d5[:4], focal, 0.4, 0.8)


# ---- what the GPU cases' inputs must exercise, shown for the restatement alone ----
def test_oblique_case_has_occlusion_losers_and_off_screen_rows():
    rows, cam = ref.oblique_case()
    _, _, behind, won, depth = ref.paint(rows, cam)
    n = len(rows)
    seen = behind < ref.OFFSCREEN
    assert int(((behind > 0) & seen).sum()) >= n // 10
    assert int((seen & (won == 0)).sum()) >= 1 and int((~seen).sum()) >= 1
    in_range = (np.abs(rows) <= ref.COORD_LIMIT).all(axis=1)
    assert (~seen & in_range).any() and (~in_range).any()               # clipped by the image, and beyond the coordinate range
    assert len({tuple(a) for a in cam[1]} & {(16384, 0, 0), (0, 16384, 0), (0, 0, 16384)}) == 0      # really oblique


def test_tie_case_has_equal_keys_on_one_pixel():
    xyz, cam = ref.tie_case()
    pr = [ref.project(p, cam) for p in xyz]
    assert pr[0][3] == pr[1][3] and pr[0][1] == pr[1][1]
    cols0, cols1 = set(range(pr[0][0], pr[0][0] + pr[0][2])), set(range(pr[1][0], pr[1][0] + pr[1][2]))
    assert cols0 & cols1 and 0 <= min(cols0 & cols1) < cam[5] and 0 <= pr[0][1] < cam[4]
    _, _, behind, won, _ = ref.paint(xyz, cam)
    assert behind[0] == behind[1] == 0 and won[0] > won[1] > 0          # the lower row took the shared pixels
    assert behind[4] == 3 and won[4] == 0                               # the voxel three behind them is covered


def test_clip_case_cuts_splats_at_every_edge_and_corner():
    xyz, cam, cuts = ref.clip_case()
    assert {ref.project(p, cam)[2] for p in xyz} == {16}
    assert len(cuts) == 8 and all(mask.any() for mask in cuts.values())
    _, _, behind, won, _ = ref.paint(xyz, cam)
    off = behind == ref.OFFSCREEN
    assert off.any() and not off.all() and all((~off[mask]).all() for mask in cuts.values())
    assert 0 < int(won.sum()) < cam[4] * cam[5]                          # voxels 25 pixels apart drawn 16 wide: holes between them


def test_inside_camera_has_rows_on_both_sides_of_the_near_plane():
    xyz = ref.exactly(1000, ref.BOX, 1000 + 1000)
    cam = ref.inside_camera()
    drawn = np.array([ref.project(p, cam) is not None for p in xyz])
    assert 100 < int(drawn.sum()) < 900
    sizes = {ref.project(p, cam)[2] for p in xyz[drawn]}
    assert len(sizes) >= 4                                               # perspective: the splat grows towards the camera
    assert {ref.project(p, ref.far_camera())[2] for p in xyz} == {1}
    assert {ref.project(p, ref.near_camera())[2] for p in xyz} == {16}
