"""render.visibility (csrc/render.hip, pcc_view_visibility) on the GPU: both outputs EQUAL to the painter's-loop restatement
(tests/_visibility_reference.py) on every case — depths and counts are integers, so equality is the bound."""
import numpy as np
import pytest
import torch

import _view_reference as vref
import _visibility_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRONT, SIDE, BACK = ((0, 0, 1), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0))
SIGNED = [tuple(s * int(k == a) for k in range(3)) for a in range(3) for s in (1, -1)]
PAIRS = [(f, u) for f in SIGNED for u in SIGNED if sum(a * b for a, b in zip(f, u)) == 0]
LIMIT = 130000


def gpu_vis(xyz, views, H, W, **kw):
    from pcc_amd import render
    xyz = np.asarray(xyz).reshape(-1, 3)
    behind, won = render.visibility(torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.int32)).to(DEV), list(views), H, W, **kw)
    for t in (behind, won):
        assert t.dtype == torch.int32 and tuple(t.shape) == (xyz.shape[0],) and t.is_cuda
    return behind.cpu().numpy().astype(np.int64), won.cpu().numpy().astype(np.int64)


def check(xyz, views, H, W, frames=None, point_size=None):
    """GPU outputs == reference outputs -> (behind, won)"""
    want_b, want_w = ref.visibility(xyz, views, H, W, frames=frames, point_size=point_size)
    got_b, got_w = gpu_vis(xyz, views, H, W, frames=frames, point_size=point_size)
    assert np.array_equal(got_b, want_b), "behind: %d rows differ" % int((got_b != want_b).sum())
    assert np.array_equal(got_w, want_w), "won: %d rows differ" % int((got_w != want_w).sum())
    assert (got_b >= 0).all() and (got_b[got_w > 0] == 0).all()
    return got_b, got_w


def exactly(n, grid, seed):
    """n distinct voxels of a grid^3 box in random row order"""
    rng = np.random.default_rng(seed)
    xyz = np.unique(rng.integers(0, grid, size=(2 * n + 8, 3)), axis=0)
    rng.shuffle(xyz)
    assert xyz.shape[0] >= n
    return xyz[:n].astype(np.int64)


def c_entry(pcc, rows, view, frame, point_size, H, W, accumulate=0, fill=None, axes=None, short=0):
    """pcc_view_visibility itself on rows (batch, x, y, z) AS GIVEN (no sort) -> (rc, behind, won); ``fill``: what the outputs
    hold before the call; ``axes``: (right, up, front) in place of the view's; ``short``: bytes taken off the scratch size"""
    from pcc_amd import _lib
    L = pcc.lib()
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
    n = rows.shape[0]
    r, u, f = axes if axes is not None else vref.axes(view[0], view[1])
    vecs = [np.ascontiguousarray(a, dtype=np.int32) for a in (r, u, f)]
    coords = torch.from_numpy(rows).to(DEV)
    behind = torch.full((n,), 0 if fill is None else fill[0], dtype=torch.int32, device=DEV)
    won = torch.full((n,), 0 if fill is None else fill[1], dtype=torch.int32, device=DEV)
    nbytes = max(int(L.pcc_visibility_scratch_bytes(H, W)), 8)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    u_min, _, _, v_max, scale, ox, oy = frame
    torch.cuda.synchronize()
    rc = L.pcc_view_visibility(coords.data_ptr(), n, vecs[0].ctypes.data, vecs[1].ctypes.data, vecs[2].ctypes.data, u_min, v_max, ox, oy,
                               scale, point_size, H, W, scratch.data_ptr(), nbytes - short, accumulate, behind.data_ptr(), won.data_ptr(),
                               _lib.stream())
    torch.cuda.synchronize()
    return rc, behind.cpu().numpy().astype(np.int64), won.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1000])
def test_point_counts_around_a_workgroup(pcc, n):
    xyz = exactly(n, 24, 1000 + n)
    # the 24^3 box framed by hand (a cloud of one or two voxels would frame itself at a scale beyond the renderer's 64)
    check(xyz, [FRONT], 128, 96, frames=[(0, 23, 0, 23, 4, 0, 16)])
    b, w = check(xyz, [SIDE], 30, 28, frames=[(0, 23, 0, 23, 1, 2, 3)], point_size=3)              # scale 1, overlapping squares
    if n >= 255:
        assert (b > 0).any() and (w == 0).any()
    if n:
        assert (b < ref.OFFSCREEN).all()
    # the C entry takes n == 0 with null arrays and launches nothing
    if n == 0:
        L = pcc.lib()
        vecs = [np.ascontiguousarray(a, dtype=np.int32) for a in vref.axes(FRONT[0], FRONT[1])]
        zbuf = torch.empty(8 * 8 * 8, dtype=torch.uint8, device=DEV)
        assert L.pcc_view_visibility(None, 0, vecs[0].ctypes.data, vecs[1].ctypes.data, vecs[2].ctypes.data, 0, 0, 0, 0, 1, 1, 8, 8,
                                     zbuf.data_ptr(), 8 * 8 * 8, 0, None, None, None) == 0
        torch.cuda.synchronize()


def test_all_24_views(pcc):
    assert len(PAIRS) == 24
    xyz = exactly(257, 24, 24)
    seen = set()
    for view in PAIRS:
        b, w = check(xyz, [view], 50, 52, point_size=3)           # scale 2
        seen.add(b.tobytes() + w.tobytes())
    assert len(seen) >= 6                                        # at least the six fronts tell themselves apart


@pytest.mark.parametrize("scale", [1, 2, 3])
def test_scales_and_point_sizes(pcc, scale):
    from pcc_amd import render
    xyz = exactly(1000, 24, 7 + scale)
    H, W = 24 * scale + 9, 24 * scale + 4
    for view in (FRONT, SIDE):
        frame = vref.frame_of(xyz, view[0], view[1], H, W, scale=scale)
        assert render.view_frame(torch.from_numpy(xyz), view[0], view[1], H, W, scale=scale) == frame
        for ps in (1, scale, scale + 1, 16):
            b, w = check(xyz, [view], H, W, frames=[frame], point_size=ps)
            if ps == 16:                                         # wide overlap: points that tie the front depth and lose every pixel
                assert ((b == 0) & (w == 0)).any()


def test_clipping_at_each_edge_and_off_screen(pcc):
    """the cloud spans 24 voxels = 74 pixels at scale 3 with squares of 5; hand-made frames push it over one edge at a time"""
    xyz = exactly(1000, 24, 31)
    H, W = 100, 90
    lo_u, hi_v = 0, 23                                            # FRONT: u = x, v = y
    for name, ox, oy in (("left", -7, 10), ("right", 30, 10), ("top", 5, -8), ("bottom", 5, 40)):
        frame = (lo_u, 23, 0, hi_v, 3, ox, oy)
        b, w = check(xyz, [FRONT], H, W, frames=[frame], point_size=5)
        off = b == ref.OFFSCREEN
        assert off.any() and not off.all(), name
        assert (w[off] == 0).all(), name
        # a point cut in part is still seen: fewer than 25 pixels inside, behind finite
        col, row = (xyz[:, 0] - lo_u) * 3 + ox, (hi_v - xyz[:, 1]) * 3 + oy
        part = ~off & ((col < 0) | (col + 5 > W) | (row < 0) | (row + 5 > H))
        assert part.any() and (b[part] < ref.OFFSCREEN).all(), name
    for frame in ((1000, 1001, 0, 1, 1, 0, 0), (0, 1, -2000, -1999, 1, 0, 0)):
        b, w = check(xyz, [FRONT], 8, 8, frames=[frame])
        assert (b == ref.OFFSCREEN).all() and (w == 0).all()


def test_frames_anywhere_in_int32(pcc):
    """u_min, v_max, ox and oy are the caller's and may be anywhere in int32: the pixel positions are worked out and clipped in
    64 bits before they are narrowed.  Five points at scale 64 with squares of 16 in a 72 x 72 image, through the entry."""
    xyz = np.array([(0, 0, 0), (0, 0, 2), (1, 0, 0), (0, 1, 2), (1, 1, -3)], dtype=np.int64)
    rows = np.concatenate([np.zeros((5, 1), dtype=np.int64), xyz], axis=1)
    H = W = 72
    # the intermediates (u + 2^25) 64 and (2^25 + 1 - v) 64 are about 2^31 and cancel against ox, oy: columns 64 u, rows 64 (1 - v)
    frame = (-2 ** 25, 0, 0, 2 ** 25 + 1, 64, -2 ** 31, -2 ** 31)
    want_b, want_w = ref.view_visibility(xyz, FRONT[0], FRONT[1], H, W, frame, point_size=16)
    rc, b, w = c_entry(pcc, rows, FRONT, frame, 16, H, W, fill=(-7, -7))
    assert rc == 0 and np.array_equal(b, want_b) and np.array_equal(w, want_w)
    # by hand: every splat lands; (0, 0, 0) lies 2 behind (0, 0, 2); the right column and the bottom row of splats are cut to 8
    assert b.tolist() == [2, 0, 0, 0, 0] and w.tolist() == [0, 16 * 8, 8 * 8, 16 * 16, 8 * 16]
    # the corners of int32: every row is far off-screen, and nothing wraps round
    for frame in ((2 ** 31 - 1, 0, 0, -2 ** 31, 64, 2 ** 31 - 1, -2 ** 31), (-2 ** 31, 0, 0, 2 ** 31 - 1, 64, -2 ** 31, 2 ** 31 - 1)):
        want_b, want_w = ref.view_visibility(xyz, FRONT[0], FRONT[1], H, W, frame, point_size=16)
        rc, b, w = c_entry(pcc, rows, FRONT, frame, 16, H, W, fill=(-7, -7))
        assert rc == 0 and np.array_equal(b, want_b) and np.array_equal(w, want_w)
        assert (b == ref.OFFSCREEN).all() and (w == 0).all()


def test_depth_range(pcc):
    two = np.array([[0, 0, -LIMIT], [0, 0, LIMIT]], dtype=np.int64)
    b, w = check(two, [FRONT], 1, 1)
    assert b.tolist() == [2 * LIMIT, 0] and w.tolist() == [0, 1]
    b, w = check(two, [BACK], 1, 1)
    assert b.tolist() == [0, 2 * LIMIT] and w.tolist() == [1, 0]
    b, w = check(two, [FRONT, BACK], 1, 1)
    assert b.tolist() == [0, 0] and w.tolist() == [1, 1]
    # rows beyond the range, straight to the entry: they draw nothing (the far point stays 2 LIMIT behind, not more) and are off-screen
    rows = np.array([[0, 0, 0, -LIMIT], [0, 0, 0, LIMIT], [0, 0, 0, LIMIT + 1], [0, -LIMIT - 1, 0, 0]])
    frame = (0, 0, 0, 0, 1, 0, 0)
    rc, b, w = c_entry(pcc, rows, FRONT, frame, 1, 1, 1, fill=(5, 5))
    assert rc == 0 and b.tolist() == [2 * LIMIT, 0, ref.OFFSCREEN, ref.OFFSCREEN] and w.tolist() == [0, 1, 0, 0]
    want = ref.view_visibility(rows[:, 1:], FRONT[0], FRONT[1], 1, 1, frame, 1)
    assert np.array_equal(b, want[0]) and np.array_equal(w, want[1])
    # accumulate: the minimum with / the sum onto what the arrays hold; an off-screen row leaves both as they are
    rc, b, w = c_entry(pcc, rows, FRONT, frame, 1, 1, 1, accumulate=1, fill=(7, 5))
    assert rc == 0 and b.tolist() == [7, 0, 7, 7] and w.tolist() == [5, 6, 5, 5]


def test_two_parallel_planes(pcc):
    g = np.stack(np.meshgrid(np.arange(9), np.arange(7), indexing="ij"), axis=-1).reshape(-1, 2)
    near = np.concatenate([g, np.full((len(g), 1), 8)], axis=1)
    far = np.concatenate([g[g[:, 0] < 6], np.full((int((g[:, 0] < 6).sum()), 1), 3)], axis=1)    # covered everywhere by the near one
    xyz = np.concatenate([near, far]).astype(np.int64)
    nn = len(near)
    area = vref.frame_of(xyz, FRONT[0], FRONT[1], 40, 48)[4] ** 2                             # no overlap: scale^2 pixels each
    b, w = check(xyz, [FRONT], 40, 48)
    assert (b[:nn] == 0).all() and (b[nn:] == 5).all() and (w[nn:] == 0).all() and (w[:nn] == area).all()
    b, w = check(xyz, [FRONT, BACK], 40, 48)
    assert (b == 0).all() and (w[nn:] == area).all()
    # three views folded in one call == elementwise min / sum of three single-view calls
    views = [FRONT, SIDE, ((0, -1, 0), (0, 0, 1))]
    cloud = np.concatenate([xyz, exactly(300, 9, 3)])
    cloud = np.unique(cloud, axis=0)
    b3, w3 = check(cloud, views, 40, 48, point_size=5)
    singles = [gpu_vis(cloud, [v], 40, 48, point_size=5) for v in views]
    assert np.array_equal(b3, np.minimum.reduce([s[0] for s in singles])) and np.array_equal(w3, sum(s[1] for s in singles))


def test_row_order_invariance(pcc):
    xyz = exactly(1000, 24, 77)
    b, w = check(xyz, [FRONT, SIDE], 60, 56, point_size=4)
    perm = np.random.default_rng(8).permutation(len(xyz))
    bp, wp = gpu_vis(xyz[perm], [FRONT, SIDE], 60, 56, point_size=4)
    assert np.array_equal(bp, b[perm]) and np.array_equal(wp, w[perm])
    assert ((b == 0) & (w == 0)).any()                           # ties were there to be broken


@pytest.mark.parametrize("point_size", [None, 3])
def test_agrees_with_the_renderer(pcc, point_size):
    """colours unique per point, a background no point has: won[i] is the number of pixels of render_view's image in point i's
    colour"""
    from pcc_amd import render
    xyz = exactly(1000, 24, 5)
    idx = np.arange(len(xyz))
    rgb = np.stack([idx & 255, idx >> 8, np.ones_like(idx)], axis=1)
    cloud = torch.from_numpy(np.concatenate([xyz, rgb / 255.0], axis=1).astype(np.float32)).to(DEV)
    H, W = 60, 52                                                # scale 2
    img = render.render_view(cloud, FRONT[0], FRONT[1], H, W, point_size=point_size).cpu().numpy().astype(np.int64)
    background = (img == 255).all(axis=2)
    shown = img[~background]
    assert (shown[:, 2] == 1).all()
    counts = np.bincount(shown[:, 0] + 256 * shown[:, 1], minlength=len(xyz))
    b, w = gpu_vis(xyz, [FRONT], H, W, point_size=point_size)
    assert np.array_equal(w, counts) and int(w.sum()) == int((~background).sum()) > 0


@pytest.mark.parametrize("H,W", [(160, 96), (40, 40)])
def test_config1_shell(pcc, H, W):
    from pcc_amd import synthetic as syn
    xyz = syn.sphere_shell(**syn.CONFIG1)[:, :3].astype(np.int64)
    b, w = check(xyz, [FRONT], H, W)
    assert (int((b == 0).sum()), int((b <= 2).sum()), int((b == ref.OFFSCREEN).sum())) == (788, 2012, 0)
    b2, _ = check(xyz, [FRONT, BACK], H, W)
    assert int((b2 <= 2).sum()) == 3992
    again = gpu_vis(xyz, [FRONT], H, W)                          # reproducible: identical bytes
    assert again[0].tobytes() == b.tobytes() and again[1].tobytes() == w.tobytes()


def test_reproducible_with_overlap(pcc):
    xyz = exactly(1000, 24, 12)
    first = gpu_vis(xyz, [SIDE, FRONT], 64, 64, point_size=16)
    second = gpu_vis(xyz, [SIDE, FRONT], 64, 64, point_size=16)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_c_entry_refusals_write_nothing(pcc):
    from pcc_amd import _lib
    L = pcc.lib()
    rows = np.array([[0, 1, 2, 3], [0, 2, 2, 1]])
    frame, fill = (0, 3, 0, 3, 2, 0, 0), (41, 43)
    r, u, f = vref.axes(FRONT[0], FRONT[1])
    cases = {
        "a non-axis vector": dict(axes=(np.array([1, 1, 0]), u, f)),
        "a vector of length two": dict(axes=(2 * r, u, f)),
        "right != up x front": dict(axes=(-r, u, f)),
        "scale 0": dict(frame=(0, 3, 0, 3, 0, 0, 0)),
        "scale 65": dict(frame=(0, 3, 0, 3, 65, 0, 0)),
        "point_size 17": dict(point_size=17),
        "point_size 0": dict(point_size=0),
        "H 0": dict(H=0),
        "W 8193": dict(W=8193),
        "scratch one byte short": dict(short=1),
    }
    for name, kw in cases.items():
        args = dict(frame=frame, point_size=2, H=8, W=8)
        args.update(kw)
        rc, b, w = c_entry(pcc, rows, FRONT, args.pop("frame"), args.pop("point_size"), args.pop("H"), args.pop("W"), fill=fill, **args)
        assert rc == _lib.PCC.ERR_ARG, name
        assert b"pcc_view_visibility" in L.pcc_last_error(), name
        assert (b == fill[0]).all() and (w == fill[1]).all(), name
    assert L.pcc_visibility_scratch_bytes(0, 8) == 0 and L.pcc_visibility_scratch_bytes(8, 8193) == 0
    assert L.pcc_visibility_scratch_bytes(8, 8) == 8 * 8 * 8 == L.pcc_render_scratch_bytes(8, 8)
    rc, b, w = c_entry(pcc, rows, FRONT, frame, 2, 8, 8, fill=fill)                   # the same call, accepted: overwrites
    assert rc == 0 and b.tolist() == [0, 0] and w.tolist() == [4, 4]


def test_visibility_map_on_a_coordinate_map(pcc):
    from pcc_amd import q_map, render
    xyz = exactly(500, 12, 4)
    coords = torch.from_numpy(np.concatenate([np.zeros((len(xyz), 1), dtype=np.int64), xyz], axis=1)).to(torch.int32).to(DEV)
    cmap = pcc.CoordMap(coords, 1, nbatch=1)
    behind, _ = render.visibility(cmap.coords[:, 1:4], ["front"], 48, 48)
    want_b, _ = ref.visibility(xyz, [FRONT], 48, 48)
    assert np.array_equal(behind.cpu().numpy(), want_b)
    Q = q_map.visibility_map(cmap, behind, 0.4, 0.8, tolerance=1, falloff=4, floor=0.25)
    s = ref.score(want_b, 1, 4, 0.25)
    assert Q.F.is_cuda and Q.F.cpu().numpy().tobytes() == np.stack([0.4 * s, 0.8 * s], axis=1).astype(np.float32).tobytes()
