"""pcc_render_camera and pcc_camera_visibility (csrc/render.hip) on the GPU, through the C entries: image bytes, behind, won and
depth EQUAL to the painter's-loop restatement (tests/_camera_reference.py) on every case — all outputs are integers and bytes,
so equality is the bound.  Rows go to the entries as given (the row index is the tie rule), output buffers are filled with
sentinels first.  tests/test_camera_reference.py shows, for the restatement alone, that these inputs exercise what they are for."""
import numpy as np
import pytest
import torch

import _camera_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (7, 200, 90)
SENTINEL = -77


def colours(n, seed=0):
    return np.random.default_rng(seed).integers(0, 255, size=(n, 3)).astype(np.uint8)      # 255 is left to the sentinel fill


def camera_arrays(cam):
    pos_q, axes_q, focal_q, near_q, H, W = cam
    return np.ascontiguousarray(pos_q, dtype=np.int32), np.ascontiguousarray(axes_q, dtype=np.int32).reshape(9), focal_q, near_q, H, W


def c_render(pcc, rows4, rgb8, cam, ps_q=16, short=0, null_cloud=False):
    """pcc_render_camera on rows (batch, x, y, z) AS GIVEN -> (rc, image [H, W, 3]); the image holds 255s before the call"""
    from pcc_amd import _lib
    L = pcc.lib()
    pos, axes, focal_q, near_q, H, W = camera_arrays(cam)
    rows4 = np.ascontiguousarray(rows4, dtype=np.int32).reshape(-1, 4)
    n = rows4.shape[0]
    coords = torch.from_numpy(rows4).to(DEV)
    rgb = torch.from_numpy(np.ascontiguousarray(rgb8, dtype=np.uint8).reshape(-1, 3)).to(DEV)
    bg = np.asarray(BG, dtype=np.uint8)
    hh, ww = min(max(H, 1), 8192), min(max(W, 1), 8192)                  # refused sizes still get real buffers
    image = torch.full((hh, ww, 3), 255, dtype=torch.uint8, device=DEV)
    nbytes = hh * ww * 8
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = L.pcc_render_camera(None if null_cloud else coords.data_ptr(), None if null_cloud else rgb.data_ptr(), n, pos.ctypes.data,
                             axes.ctypes.data, focal_q, near_q, H, W, ps_q, bg.ctypes.data, scratch.data_ptr(), nbytes - short,
                             image.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return rc, image.cpu().numpy()


def c_vis(pcc, rows4, cam, ps_q=16, accumulate=0, fill=(SENTINEL, SENTINEL, SENTINEL), short=0, buffers=None):
    """pcc_camera_visibility on rows AS GIVEN -> (rc, behind, won, depth) as int64 arrays; ``buffers``: the three device tensors
    of an earlier call to fold into"""
    from pcc_amd import _lib
    L = pcc.lib()
    pos, axes, focal_q, near_q, H, W = camera_arrays(cam)
    rows4 = np.ascontiguousarray(rows4, dtype=np.int32).reshape(-1, 4)
    n = rows4.shape[0]
    coords = torch.from_numpy(rows4).to(DEV)
    if buffers is None:
        buffers = [torch.full((n,), v, dtype=torch.int32, device=DEV) for v in fill]
    hh, ww = min(max(H, 1), 8192), min(max(W, 1), 8192)
    nbytes = hh * ww * 8
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = L.pcc_camera_visibility(coords.data_ptr(), n, pos.ctypes.data, axes.ctypes.data, focal_q, near_q, H, W, ps_q, scratch.data_ptr(),
                                 nbytes - short, accumulate, buffers[0].data_ptr(), buffers[1].data_ptr(), buffers[2].data_ptr(),
                                 _lib.stream())
    torch.cuda.synchronize()
    return (rc,) + tuple(b.cpu().numpy().astype(np.int64) for b in buffers) + (buffers,)


def check(pcc, xyz, cam, point_size=1.0, batch=0):
    """both entries == the restatement on rows as given -> (image, behind, won, depth)"""
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    n = xyz.shape[0]
    ps_q = ref.ps_q_of(point_size)
    rgb8 = colours(n, seed=n)
    rows4 = np.concatenate([np.full((n, 1), batch, dtype=np.int64), xyz], axis=1)
    _, winner, want_b, want_w, want_d = ref.paint(xyz, cam, ps_q)
    want_img = ref.image_of(winner, rgb8, BG)
    rc, img = c_render(pcc, rows4, rgb8, cam, ps_q)
    assert rc == 0 and img.shape == want_img.shape
    assert np.array_equal(img, want_img), "image: %d pixels differ" % int((img != want_img).any(axis=2).sum())
    rc, b, w, d, _ = c_vis(pcc, rows4, cam, ps_q)
    assert rc == 0
    assert np.array_equal(b, want_b), "behind: %d rows differ" % int((b != want_b).sum())
    assert np.array_equal(w, want_w), "won: %d rows differ" % int((w != want_w).sum())
    assert np.array_equal(d, want_d), "depth: %d rows differ" % int((d != want_d).sum())
    assert (b >= 0).all() and (b[w > 0] == 0).all() and (w[b == ref.OFFSCREEN] == 0).all()
    assert int(w.sum()) == int((winner >= 0).sum()) == int((img != np.array(BG, dtype=np.uint8)).any(axis=2).sum())
    return img, b, w, d


FRONT_30 = ref.axis_camera((0, 0, 1), (0, 1, 0), 60.0, 50.0, 30, 28)     # the 24^3 box about 20 pixels wide


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1000])
def test_point_counts_around_a_workgroup(pcc, n):
    xyz = ref.exactly(n, ref.BOX, 1000 + n)
    check(pcc, xyz, ref.oblique_camera())
    img, b, w, d = check(pcc, xyz, FRONT_30, point_size=3)
    if n >= 255:
        assert ((b > 0) & (b < ref.OFFSCREEN)).any() and (w == 0).any() and (w > 1).any()
    if n == 0:                                                           # null arrays: every pixel is background, nothing is launched
        rc, img = c_render(pcc, np.zeros((0, 4)), np.zeros((0, 3)), FRONT_30, null_cloud=True)
        assert rc == 0 and (img == np.array(BG, dtype=np.uint8)).all()
        L = pcc.lib()
        pos, axes, focal_q, near_q, H, W = camera_arrays(FRONT_30)
        zbuf = torch.empty(H * W * 8, dtype=torch.uint8, device=DEV)
        assert L.pcc_camera_visibility(None, 0, pos.ctypes.data, axes.ctypes.data, focal_q, near_q, H, W, 16, zbuf.data_ptr(), H * W * 8, 0,
                                       None, None, None, None) == 0
        torch.cuda.synchronize()


@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (30, 28), (128, 96)])
def test_image_sizes(pcc, H, W):
    xyz = ref.exactly(257, ref.BOX, 5)
    check(pcc, xyz, ref.oblique_camera(H, W))
    # the box wider than the image at every size: splats cut at all four edges
    img, b, w, d = check(pcc, xyz, ref.axis_camera((0, 0, 1), (0, 1, 0), 60.0, 3.0 * max(H, W), H, W), point_size=3)
    assert (b == ref.OFFSCREEN).any() and (w > 0).any()


def test_the_six_axis_directions(pcc):
    xyz = ref.exactly(257, ref.BOX, 24)
    seen = set()
    for front, up in ref.AXIS_VIEWS:
        img, b, w, d = check(pcc, xyz, ref.axis_camera(front, up, 50.0, 45.0, 30, 28), point_size=2)
        seen.add(img.tobytes())
    assert len(seen) == 6


def test_clipping_at_each_edge_and_corner(pcc):
    """the near camera draws every voxel 16 pixels wide and the box's core far wider than the image: splats are cut at the four
    edges and at the four corners, and most lie outside altogether"""
    xyz, cam, cuts = ref.clip_case()
    img, b, w, d = check(pcc, xyz, cam)
    off = b == ref.OFFSCREEN
    assert off.any() and not off.all() and (d[off] == ref.OFFSCREEN).all()
    for name, mask in cuts.items():
        assert mask.any() and (b[mask] < ref.OFFSCREEN).all(), name


@pytest.mark.parametrize("point_size", [0.5, 1, 3])
def test_oblique_inside_far_and_near_cameras(pcc, point_size):
    rows, cam = ref.oblique_case()
    img, b, w, d = check(pcc, rows, cam, point_size, batch=3)            # a batch column != 0 is ignored; two rows are out of range
    out_of_range = (np.abs(rows) > ref.COORD_LIMIT).any(axis=1)
    assert out_of_range.sum() == 2 and (b[out_of_range] == ref.OFFSCREEN).all() and (d[out_of_range] == ref.OFFSCREEN).all()
    xyz = ref.exactly(1000, ref.BOX, 2000)
    img, b, w, d = check(pcc, xyz, ref.inside_camera(), point_size)
    assert (b == ref.OFFSCREEN).any() and (b == 0).any() and ((b > 0) & (b < ref.OFFSCREEN)).any()
    img, b, w, d = check(pcc, xyz, ref.far_camera(), point_size)
    assert w.max() == 1 and (b > 0).sum() > 500                          # single pixels, most of the box hidden
    if point_size == 1:
        img, b, w, d = check(pcc, xyz[:257], ref.near_camera(30, 28), point_size)
        assert w.max() <= 256


def test_accumulate_over_two_cameras(pcc):
    rows, cam1 = ref.oblique_case()
    cam2 = ref.axis_camera((-1, 0, 0), (0, 0, 1), 50.0, 45.0, 30, 28)
    n = len(rows)
    rows4 = np.concatenate([np.zeros((n, 1), dtype=np.int64), rows], axis=1)
    one = ref.paint(rows, cam1)[2:]
    two = ref.paint(rows, cam2)[2:]
    rc, b, w, d, buffers = c_vis(pcc, rows4, cam1)
    assert rc == 0 and all(np.array_equal(g, x) for g, x in zip((b, w, d), one))
    rc, b, w, d, _ = c_vis(pcc, rows4, cam2, accumulate=1, buffers=buffers)
    assert rc == 0
    assert np.array_equal(b, np.minimum(one[0], two[0])) and np.array_equal(w, one[1] + two[1]) and np.array_equal(d, np.minimum(one[2], two[2]))
    assert (b < one[0]).any() and (w > one[1]).any()
    # onto what the arrays hold, whatever it is; a row that is not drawn leaves all three as they are
    rc, b, w, d, _ = c_vis(pcc, rows4, cam2, accumulate=1, fill=(3, 5, 9000))
    assert np.array_equal(b, np.minimum(3, two[0])) and np.array_equal(w, 5 + two[1]) and np.array_equal(d, np.minimum(9000, two[2]))


def test_ties_do_not_depend_on_the_input_order(pcc):
    """through render.render_camera / camera_visibility, which put the rows in canonical order first"""
    from pcc_amd import render
    xyz, q = ref.tie_case()
    cam = render.Camera.from_quantised(*q)
    rgb = colours(len(xyz), 9).astype(np.float32) / 255.0
    cloud = np.concatenate([xyz.astype(np.float32), rgb], axis=1)
    want_img = ref.render_camera(cloud, q)
    want = ref.camera_visibility(xyz, [q])
    assert want[1][0] > want[1][1] > 0 and want[0][4] > 0
    for rows in (cloud, cloud[::-1].copy()):
        t = torch.from_numpy(rows).to(DEV)
        assert np.array_equal(render.render_camera(t, cam).cpu().numpy(), want_img)
    got = [g.cpu().numpy() for g in render.camera_visibility(torch.from_numpy(xyz).to(DEV), [cam])]
    back = [g.cpu().numpy() for g in render.camera_visibility(torch.from_numpy(xyz[::-1].copy()).to(DEV), [cam])]
    for g, r, x in zip(got, back, want):
        assert np.array_equal(g, x) and np.array_equal(r[::-1], x)
    # the entry itself takes the rows as they come: reversed rows hand the shared pixels to the other voxel
    rows4 = np.concatenate([np.zeros((len(xyz), 1), dtype=np.int64), xyz], axis=1)
    _, _, w_fwd, _, _ = c_vis(pcc, rows4, q)
    _, _, w_rev, _, _ = c_vis(pcc, rows4[::-1], q)
    assert np.array_equal(w_rev, ref.paint(xyz[::-1], q)[3]) and not np.array_equal(w_rev[::-1], w_fwd)


def test_two_runs_are_bitwise_identical(pcc):
    rows, cam = ref.oblique_case()
    n = len(rows)
    rows4 = np.concatenate([np.zeros((n, 1), dtype=np.int64), rows], axis=1)
    rgb8 = colours(n, 1)
    for c, ps_q in ((cam, 16), (ref.near_camera(), 48)):
        first = (c_render(pcc, rows4, rgb8, c, ps_q)[1],) + c_vis(pcc, rows4, c, ps_q)[1:4]
        second = (c_render(pcc, rows4, rgb8, c, ps_q)[1],) + c_vis(pcc, rows4, c, ps_q)[1:4]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))


def test_refusals_write_nothing(pcc):
    from pcc_amd import _lib
    L = pcc.lib()
    rows4 = np.array([[0, 11, 11, 5], [0, 12, 11, 5]])
    rgb8 = colours(2)
    good = FRONT_30
    pos_q, axes_q, focal_q, near_q, H, W = good

    def with_axis(k, v):
        a = [list(r) for r in axes_q]
        a[k // 3][k % 3] = v
        return (pos_q, tuple(tuple(r) for r in a), focal_q, near_q, H, W)

    cases = {
        "scratch one byte short": dict(short=1),
        "focal_q 0": dict(cam=(pos_q, axes_q, 0, near_q, H, W)),
        "focal_q 2^20 + 1": dict(cam=(pos_q, axes_q, 2 ** 20 + 1, near_q, H, W)),
        "an axis entry of 2^14 + 1": dict(cam=with_axis(0, 2 ** 14 + 1)),
        "an axis entry of -2^14 - 1": dict(cam=with_axis(8, -2 ** 14 - 1)),
        "ps_q 0": dict(ps_q=0),
        "ps_q 257": dict(ps_q=257),
        "H 0": dict(cam=(pos_q, axes_q, focal_q, near_q, 0, W)),
        "W 8193": dict(cam=(pos_q, axes_q, focal_q, near_q, H, 8193)),
        "near_q 0": dict(cam=(pos_q, axes_q, focal_q, 0, H, W)),
        "pos_q beyond 2^24": dict(cam=((2 ** 24 + 1, 0, 0), axes_q, focal_q, near_q, H, W)),
    }
    for name, kw in cases.items():
        args = dict(cam=good, ps_q=16, short=0)
        args.update(kw)
        rc, img = c_render(pcc, rows4, rgb8, args["cam"], args["ps_q"], short=args["short"])
        assert rc == _lib.PCC.ERR_ARG and b"pcc_render_camera" in L.pcc_last_error(), name
        assert (img == 255).all(), name
        rc, b, w, d, _ = c_vis(pcc, rows4, args["cam"], args["ps_q"], short=args["short"])
        assert rc == _lib.PCC.ERR_ARG and b"pcc_camera_visibility" in L.pcc_last_error(), name
        assert (b == SENTINEL).all() and (w == SENTINEL).all() and (d == SENTINEL).all(), name
    # null pointers
    pos, axes, focal_q, near_q, H, W = camera_arrays(good)
    z = torch.empty(H * W * 8, dtype=torch.uint8, device=DEV)
    out = torch.full((3, 2), SENTINEL, dtype=torch.int32, device=DEV)
    c = torch.from_numpy(np.ascontiguousarray(rows4, dtype=np.int32)).to(DEV)
    vis = lambda **kw: L.pcc_camera_visibility(*[kw.get(k, v) for k, v in (
        ("coords", c.data_ptr()), ("n", 2), ("pos", pos.ctypes.data), ("axes", axes.ctypes.data), ("focal", focal_q), ("near", near_q),
        ("H", H), ("W", W), ("ps", 16), ("z", z.data_ptr()), ("zb", H * W * 8), ("acc", 0), ("b", out[0].data_ptr()),
        ("w", out[1].data_ptr()), ("d", out[2].data_ptr()), ("s", None))])
    for key in ("coords", "pos", "axes", "z", "b", "w", "d"):
        assert vis(**{key: None}) == _lib.PCC.ERR_ARG, key
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert vis() == 0
    torch.cuda.synchronize()
    want = ref.paint(rows4[:, 1:], good)
    assert all(np.array_equal(out[k].cpu().numpy(), want[2 + k]) for k in range(3))
    rc, img = c_render(pcc, rows4, rgb8, good)                           # the same call, accepted
    assert rc == 0 and np.array_equal(img, ref.image_of(want[1], rgb8, BG))
