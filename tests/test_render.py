"""render.render_view (csrc/render.hip, pcc_render_view) on the GPU: image bytes equal to the painter's-loop restatement
(tests/_view_reference.py) on every case — the projection is all integer, so equality is the bound."""
import numpy as np
import pytest
import torch

import _view_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRONT, SIDE = ((0, 0, 1), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0))
RED, BLUE = (255, 0, 0), (0, 0, 255)


def gpu_render(cloud, view, H, W, **kw):
    from pcc_amd import render
    img = render.render_view(torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32)).to(DEV), view[0], view[1], H, W, **kw)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (H, W, 3) and img.is_cuda
    return img.cpu().numpy()


def check(cloud, view, H, W, frame=None, point_size=None, background=(255, 255, 255)):
    """GPU image == reference image -> the image"""
    want = ref.render_cloud(cloud, view[0], view[1], H, W, frame=frame, point_size=point_size, background=background)
    got = gpu_render(cloud, view, H, W, frame=frame, point_size=point_size, background=background)
    assert np.array_equal(got, want), "%d pixels differ" % int((got != want).any(axis=2).sum())
    return got


def random_cloud(n, grid, seed):
    rng = np.random.default_rng(seed)
    xyz = np.unique(rng.integers(0, grid, size=(n, 3)), axis=0)
    rng.shuffle(xyz)
    rgb = rng.integers(0, 256, size=(xyz.shape[0], 3)) / 255.0
    return np.concatenate([xyz, rgb], axis=1).astype(np.float32)


def exactly(n, grid, seed):
    c = random_cloud(2 * n, grid, seed)
    assert c.shape[0] >= n
    return c[:n]


@pytest.fixture(scope="module")
def cloud19k():
    c = random_cloud(20000, 64, 11)             # about 19 k unique voxels of a 64^3 grid
    assert 18500 < c.shape[0] < 20000
    return c


def test_empty_cloud_is_background(pcc):
    empty = np.zeros((0, 6), dtype=np.float32)
    assert (gpu_render(empty, FRONT, 9, 13) == 255).all()
    got = gpu_render(empty, SIDE, 5, 4, background=(1, 2, 3), frame=(0, 0, 0, 0, 1, 0, 0))
    assert (got == np.array([1, 2, 3], dtype=np.uint8)).all()


def test_one_voxel(pcc):
    one = np.array([[7, -3, 2, 0.2, 0.4, 0.6]], dtype=np.float32)
    img = check(one, FRONT, 5, 5)                           # scale 5: the voxel fills the image
    assert (img == np.array([51, 102, 153], dtype=np.uint8)).all()
    img = check(one, SIDE, 5, 5, frame=(2, 2, -3, -3, 1, 2, 2), point_size=1)
    assert (img[2, 2] == (51, 102, 153)).all() and (img.reshape(-1, 3) == 255).all(axis=1).sum() == 24
    check(one, FRONT, 6, 7, background=(0, 0, 0), point_size=3)


def test_nearer_voxel_wins_on_one_ray(pcc):
    two = np.array([[4, 4, 1, 1, 0, 0], [4, 4, 9, 0, 0, 1]], dtype=np.float32)      # same (x, y): blue is nearer to a +z camera
    for c in (two, two[::-1]):
        assert (check(c, FRONT, 3, 3) == BLUE).all()
        assert (check(c, ((0, 0, -1), (0, 1, 0)), 3, 3) == RED).all()                 # from behind: red


def test_equal_depth_tie_goes_to_the_lower_canonical_row(pcc):
    two = np.array([[0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 1]], dtype=np.float32)
    frame = (0, 1, 0, 0, 1, 1, 1)
    for c in (two, two[::-1]):
        img = check(c, FRONT, 4, 4, frame=frame, point_size=2)
        assert (img[1:3, 1:3] == RED).all() and (img[1:3, 3] == BLUE).all()          # columns 2 is shared: red, the smaller (x, y, z)
    up_down = np.array([[0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 0, 1]], dtype=np.float32)   # neighbours along v: the shared row
    for c in (up_down, up_down[::-1]):
        check(c, FRONT, 5, 4, frame=(0, 0, 0, 1, 1, 1, 1), point_size=2)


def solid():
    """an L-shaped slab with a post, no symmetry under any axis permutation or flip; three colours by region"""
    pts = []
    for x in range(6):
        for y in range(4):
            for z in range(2):
                if x < 2 or y < 1:
                    pts.append((x, y, z, 1, 0, 0) if x >= 3 else (x, y, z, 0, 1, 0))
    pts += [(0, 3, z, 0, 0, 1) for z in range(2, 6)]
    return np.array(pts, dtype=np.float32)


SIGNED = [tuple(s * int(k == a) for k in range(3)) for a in range(3) for s in (1, -1)]
PAIRS = [(f, u) for f in SIGNED for u in SIGNED if sum(a * b for a, b in zip(f, u)) == 0]


def test_all_24_views_of_an_asymmetric_solid(pcc):
    assert len(PAIRS) == 24
    c = solid()
    seen = set()
    for view in PAIRS:
        seen.add(check(c, view, 19, 23, point_size=2).tobytes())
        check(c, view, 19, 23)
    assert len(seen) == 24                                   # no two views of it look alike


@pytest.mark.parametrize("n", [255, 256, 257])
def test_point_counts_around_a_workgroup(pcc, n):
    c = exactly(n, 16, n)
    check(c, FRONT, 40, 36)
    check(c, SIDE, 16, 16, point_size=3)


def test_frame_of_another_cloud_clips_pixel_by_pixel(pcc):
    """framed on a small box in the middle of a larger cloud: points fall outside, and squares of 5 pixels at scale 3 cross
    every border, negative pixel positions included"""
    big = random_cloud(6000, 24, 5)
    inner = big[(np.abs(big[:, :3] - 11.5) < 4).all(axis=1)]
    for view in (FRONT, SIDE, ((0, -1, 0), (0, 0, 1))):
        xyz, _ = ref.canonical(inner)
        frame = ref.frame_of(xyz, view[0], view[1], 22, 26, scale=3)
        assert frame[5] < 3 and frame[6] < 3
        img = check(big, view, 22, 26, frame=frame, point_size=5)
        drawn = (img != 255).any(axis=2)
        assert drawn[0].any() and drawn[-1].any() and drawn[:, 0].any() and drawn[:, -1].any()
        from pcc_amd import render
        assert render.view_frame(inner, view[0], view[1], 22, 26, scale=3) == frame
    # far outside: nothing is drawn, nothing wraps round
    assert (check(big, FRONT, 8, 8, frame=(1000, 1001, 0, 1, 1, 0, 0)) == 255).all()
    assert (check(big, FRONT, 8, 8, frame=(0, 1, -2000, -1999, 1, 0, 0)) == 255).all()


@pytest.mark.parametrize("H,W", [(1, 1), (37, 53), (64, 64)])
def test_image_sizes(pcc, H, W):
    c = random_cloud(3000, 40, 9)
    check(c, FRONT, H, W)
    check(c, SIDE, H, W, point_size=2)


@pytest.mark.parametrize("scale,point_size", [(1, 1), (1, 3), (2, 2), (2, 5)])
def test_19k_cloud_is_exact_and_reproducible(pcc, cloud19k, scale, point_size):
    from pcc_amd import render
    H, W = 64 * scale + 7, 64 * scale + 10
    frame = render.view_frame(cloud19k, SIDE[0], SIDE[1], H, W, scale=scale)
    first = check(cloud19k, SIDE, H, W, frame=frame, point_size=point_size)
    perm = np.random.default_rng(1).permutation(cloud19k.shape[0])
    assert np.array_equal(gpu_render(cloud19k[perm], SIDE, H, W, frame=frame, point_size=point_size), first)
    assert np.array_equal(gpu_render(cloud19k, SIDE, H, W, frame=frame, point_size=point_size), first)


@pytest.mark.parametrize("shift", [(129900, 129900, 129900), (-130000, -130000, -130000), (129900, -130000, 0)])
def test_coordinates_at_the_limit(pcc, shift):
    """translated to +-PCC_COORD_LIMIT (130,000): the same picture as at the origin, from both sides of the depth axis"""
    from pcc_amd import render
    c = random_cloud(4000, 64, 3)
    moved = c.copy()
    moved[:, :3] += np.array(shift, dtype=np.float32)
    assert np.abs(moved[:, :3]).max() <= 130000 and np.array_equal(moved[:, :3], np.rint(moved[:, :3]))
    for view in (FRONT, SIDE, ((0, 0, -1), (0, 1, 0))):
        img = check(moved, view, 70, 66, point_size=2)
        assert np.array_equal(img, gpu_render(c, view, 70, 66, point_size=2))
    beyond = moved.copy()
    beyond[0, 0] = 130001 if shift[0] > 0 else -130001
    with pytest.raises(ValueError):
        render.render_view(torch.from_numpy(beyond).to(DEV), FRONT[0], FRONT[1], 8, 8)


def c_entry(pcc, rows, rgb, view, frame, point_size, H, W, background=(255, 255, 255)):
    """pcc_render_view itself on rows (batch, x, y, z) and byte colours AS GIVEN (no sort) -> (rc, image); the image holds
    the bytes 7 before the call"""
    from pcc_amd import _lib
    L = pcc.lib()
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
    n = rows.shape[0]
    vecs = [np.ascontiguousarray(a, dtype=np.int32) for a in ref.axes(view[0], view[1])]
    coords, rgb8 = torch.from_numpy(rows).to(DEV), torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(DEV)
    bg = np.asarray(background, dtype=np.uint8)
    nbytes = int(L.pcc_render_scratch_bytes(H, W))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    image = torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)
    u_min, _, _, v_max, scale, ox, oy = frame
    torch.cuda.synchronize()
    rc = L.pcc_render_view(coords.data_ptr(), rgb8.data_ptr(), n, vecs[0].ctypes.data, vecs[1].ctypes.data, vecs[2].ctypes.data, u_min, v_max,
                           ox, oy, scale, point_size, H, W, bg.ctypes.data, scratch.data_ptr(), nbytes, image.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return rc, image.cpu().numpy()


def test_frames_anywhere_in_int32(pcc):
    """u_min, v_max, ox and oy are the caller's and may be anywhere in int32: the pixel positions are worked out and clipped in
    64 bits before they are narrowed.  Five points at scale 64 with squares of 16 in a 72 x 72 image, through the entry."""
    xyz = np.array([(0, 0, 0), (0, 0, 2), (1, 0, 0), (0, 1, 2), (1, 1, -3)], dtype=np.int64)
    rgb = np.array([(250, 0, 0), (0, 250, 0), (0, 0, 250), (250, 250, 0), (0, 250, 250)], dtype=np.uint8)
    rows = np.concatenate([np.zeros((5, 1), dtype=np.int64), xyz], axis=1)
    H = W = 72
    # the intermediates (u + 2^25) 64 and (2^25 + 1 - v) 64 are about 2^31 and cancel against ox, oy: columns 64 u, rows 64 (1 - v)
    frame = (-2 ** 25, 0, 0, 2 ** 25 + 1, 64, -2 ** 31, -2 ** 31)
    want = ref.render(xyz, rgb, FRONT[0], FRONT[1], H, W, frame, point_size=16, background=(1, 2, 3))
    rc, got = c_entry(pcc, rows, rgb, FRONT, frame, 16, H, W, background=(1, 2, 3))
    assert rc == 0 and np.array_equal(got, want), "%d pixels differ" % int((got != want).any(axis=2).sum())
    # by hand: (0, 1, 2) whole at the top left, (1, 1, -3) cut to 8 columns, (0, 0, 2) over (0, 0, 0) cut to 8 rows, (1, 0, 0) to 8 x 8
    assert (got[0:16, 0:16] == rgb[3]).all() and (got[0:16, 64:72] == rgb[4]).all()
    assert (got[64:72, 0:16] == rgb[1]).all() and (got[64:72, 64:72] == rgb[2]).all()
    assert int((got != np.array([1, 2, 3], dtype=np.uint8)).any(axis=2).sum()) == 256 + 128 + 128 + 64
    # the corners of int32: every row is far off-screen, and nothing wraps round
    for frame in ((2 ** 31 - 1, 0, 0, -2 ** 31, 64, 2 ** 31 - 1, -2 ** 31), (-2 ** 31, 0, 0, 2 ** 31 - 1, 64, -2 ** 31, 2 ** 31 - 1)):
        want = ref.render(xyz, rgb, FRONT[0], FRONT[1], H, W, frame, point_size=16)
        rc, got = c_entry(pcc, rows, rgb, FRONT, frame, 16, H, W)
        assert rc == 0 and np.array_equal(got, want) and (got == 255).all()
