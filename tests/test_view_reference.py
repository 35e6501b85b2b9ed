"""The numpy restatements of the view renderer and view metrics (tests/_view_reference.py) against hand-derived cases, and
the host-only parts of pcc_amd.render / io.write_png / the two C entries: nothing here needs a GPU."""
import ctypes
import math

import numpy as np
import pytest

import _view_reference as ref

RED, GREEN, BLUE, WHITE = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
# voxels (0,0,0) red, (0,0,5) green, (2,1,0) blue
CLOUD = np.array([[0, 0, 0, 1, 0, 0], [0, 0, 5, 0, 1, 0], [2, 1, 0, 0, 0, 1]], dtype=np.float32)


def _expect(H, W, pixels):
    img = np.full((H, W, 3), 255, dtype=np.uint8)
    for (r, c), colour in pixels.items():
        img[r, c] = colour
    return img


def test_reference_renderer_front_view_by_hand():
    """front +z, up +y, 4 x 5, scale 1: u = x in 0..2, v = y in 0..1, ox = oy = 1; green (z = 5) hides red (z = 0)"""
    got = ref.render_cloud(CLOUD, (0, 0, 1), (0, 1, 0), 4, 5)
    assert np.array_equal(got, _expect(4, 5, {(2, 1): GREEN, (1, 3): BLUE}))
    assert np.array_equal(ref.render_cloud(CLOUD[::-1], (0, 0, 1), (0, 1, 0), 4, 5), got)      # any input order


def test_reference_renderer_side_view_by_hand():
    """front -x, up +y, 4 x 8: right = +z, u = z in 0..5, scale 1, ox = oy = 1; nothing hidden"""
    got = ref.render_cloud(CLOUD, (-1, 0, 0), (0, 1, 0), 4, 8)
    assert np.array_equal(got, _expect(4, 8, {(1, 1): BLUE, (2, 1): RED, (2, 6): GREEN}))


def test_reference_renderer_tie_and_clipping():
    """equal depth, point_size 2 at scale 1: the lower canonical row keeps the shared pixels; squares that cross the
    border are clipped pixel by pixel"""
    two = np.array([[0, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 1]], dtype=np.float32)
    frame = (0, 1, 0, 0, 1, 1, 1)                                   # u_min, u_max, v_min, v_max, scale, ox, oy
    want = _expect(4, 4, {(1, 1): RED, (1, 2): RED, (2, 1): RED, (2, 2): RED, (1, 3): BLUE, (2, 3): BLUE})
    for c in (two, two[::-1]):
        assert np.array_equal(ref.render_cloud(c, (0, 0, 1), (0, 1, 0), 4, 4, frame=frame, point_size=2), want)
    frame = (0, 1, 0, 0, 1, -1, -1)                                 # red's square starts at (-1, -1): one pixel of it is visible
    got = ref.render_cloud(two, (0, 0, 1), (0, 1, 0), 2, 2, frame=frame, point_size=2)
    assert np.array_equal(got, _expect(2, 2, {(0, 0): RED, (0, 1): BLUE}))


def test_reference_metrics_equal_images_and_one_window():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(12, 9, 3), dtype=np.uint8)
    m = ref.view_metrics(a, a.copy())
    assert m["ssim"] == 1.0 and m["psnr"] == math.inf and m["y_mse"] == 0.0
    # a 7 x 7 pair is one window: the scalar formula on that window, channel by channel
    a, b = rng.integers(0, 256, size=(7, 7, 3), dtype=np.uint8), rng.integers(0, 256, size=(7, 7, 3), dtype=np.uint8)
    ya, yb = ref.yuv(a), ref.yuv(b)
    s = []
    for k in range(3):
        x, y = ya[..., k].ravel(), yb[..., k].ravel()
        ux, uy = x.sum() / 49, y.sum() / 49
        vx, vy, vxy = ((x - ux) ** 2).sum() / 48, ((y - uy) ** 2).sum() / 48, ((x - ux) * (y - uy)).sum() / 48
        s.append((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux ** 2 + uy ** 2 + 1e-4) * (vx + vy + 9e-4)))
    m = ref.view_metrics(a, b)
    assert m["ssim"] == pytest.approx(np.mean(s), abs=1e-12)
    mse = ((ya - yb) ** 2).sum() / (3 * 49)
    assert m["psnr"] == pytest.approx(10 * math.log10(m["data_range"] ** 2 / mse), abs=1e-12)
    # the colour conversion: white is (1, 0, 0) up to rounding, pure blue has the largest U and a negative V
    w = ref.yuv(np.array([[WHITE, BLUE]], dtype=np.uint8))
    assert w[0, 0, 0] == pytest.approx(1.0, abs=1e-15) and abs(w[0, 0, 1]) < 1e-8 and abs(w[0, 0, 2]) < 1e-8
    assert w[0, 1, 0] == 0.114 and w[0, 1, 1] == 0.43601035 and w[0, 1, 2] == -0.10001026


def test_view_axes_and_presets(pcc):
    from pcc_amd import render
    assert render.view_axes((0, 0, 1), (0, 1, 0)) == ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    assert render.view_axes((-1, 0, 0), (0, 1, 0)) == ((0, 0, 1), (0, 1, 0), (-1, 0, 0))
    assert render.view_axes([0.0, -1.0, 0.0], np.array([0, 0, 1])) == ((1, 0, 0), (0, 0, 1), (0, -1, 0))
    n = 0
    signed = [tuple(s * int(k == a) for k in range(3)) for a in range(3) for s in (1, -1)]
    for f in signed:
        for u in signed:
            if sum(x * y for x, y in zip(f, u)) == 0:
                r, uu, ff = render.view_axes(f, u)
                rr, _, _ = ref.axes(f, u)
                assert r == tuple(int(v) for v in rr) and uu == u and ff == f
                n += 1
            else:
                with pytest.raises(ValueError):
                    render.view_axes(f, u)
    assert n == 24
    for bad in ((0, 0, 2), (1, 1, 0), (0, 0, 0), (0, 0.5, 0), (0, 1), "front", (0, 0, 1, 0)):
        with pytest.raises(ValueError):
            render.view_axes(bad, (0, 1, 0))
        with pytest.raises(ValueError):
            render.view_axes((1, 0, 0), bad)
    assert render.VIEWS == {"front": ((0, 0, 1), (0, 1, 0)), "side": ((-1, 0, 0), (0, 1, 0))}
    assert render.VIEWS_MVUB == {"front": ((0, -1, 0), (0, 0, 1)), "side": ((-1, 0, 0), (0, 0, 1))}


def test_view_frame_arithmetic(pcc):
    from pcc_amd import render
    assert render.view_frame(CLOUD, (0, 0, 1), (0, 1, 0), 4, 5) == (0, 2, 0, 1, 1, 1, 1)
    assert render.view_frame(CLOUD, (-1, 0, 0), (0, 1, 0), 4, 8) == (0, 5, 0, 1, 1, 1, 1)
    # the largest scale at which the box fits: 3 x 2 voxels in 20 x 10 pixels -> min(20 // 3, 10 // 2) = 5
    assert render.view_frame(CLOUD, (0, 0, 1), (0, 1, 0), 10, 20) == (0, 2, 0, 1, 5, (20 - 15) // 2, 0)
    # a box that does not fit keeps scale 1 and a negative, floored offset; a given scale is used as it is
    assert render.view_frame(CLOUD, (-1, 0, 0), (0, 1, 0), 1, 3) == (0, 5, 0, 1, 1, -2, -1)
    assert render.view_frame(CLOUD, (0, 0, 1), (0, 1, 0), 4, 5, scale=2) == (0, 2, 0, 1, 2, -1, 0)
    # negated axes negate and swap the extents: front +x, up -z -> right = up x front = -y
    rng = np.random.default_rng(0)
    pts = rng.integers(-40, 90, size=(200, 3))
    for f, u in (((1, 0, 0), (0, 0, -1)), ((0, -1, 0), (0, 0, 1)), ((0, 0, -1), (1, 0, 0))):
        assert render.view_frame(pts.astype(np.float32), f, u, 333, 517) == ref.frame_of(pts, f, u, 333, 517)
        assert render.view_frame(pts.astype(np.float32), f, u, 64, 64, scale=3) == ref.frame_of(pts, f, u, 64, 64, scale=3)
    with pytest.raises(ValueError):
        render.view_frame(CLOUD + 0.25, (0, 0, 1), (0, 1, 0), 4, 5)


def test_data_range_rule_and_metric_arithmetic(pcc):
    from pcc_amd import render
    assert render.data_range_of(0.0) == 1.0 and render.data_range_of(0.3) == 1.0
    assert render.data_range_of(-1e-9) == 2.0 and render.data_range_of(-0.1) == 2.0
    H, W = 10, 9
    sums = [0.9, 0.09, 0.009, 12.0, 6.0, 3.0, 0.0, 1.0]                     # crop 4 x 3 = 12
    m = render.metrics_from_sums(sums, H, W)
    assert m["y_mse"] == 0.9 / 90 and m["u_mse"] == 0.09 / 90 and m["v_mse"] == 0.009 / 90
    assert m["ssim"] == pytest.approx((1.0 + 0.5 + 0.25) / 3, abs=1e-15)
    assert m["psnr"] == pytest.approx(10 * math.log10(1.0 / (0.999 / 270)), abs=1e-12)
    neg = render.metrics_from_sums(sums[:6] + [-0.05, 1.0], H, W)
    assert neg["psnr"] == pytest.approx(m["psnr"] + 10 * math.log10(4.0), abs=1e-12)          # data range 2
    assert render.metrics_from_sums(sums[:6] + [-0.05, 1.0], H, W, data_range=1.0)["psnr"] == m["psnr"]
    assert render.metrics_from_sums([0.0] * 3 + sums[3:], H, W)["psnr"] == math.inf


def test_write_png_round_trip(pcc, tmp_path):
    import torch
    from pcc_amd import io
    rng = np.random.default_rng(5)
    for shape in ((1, 1, 3), (5, 7, 3), (64, 33, 3)):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        p = tmp_path / ("a%d.png" % shape[0])
        io.write_png(str(p), img)
        assert np.array_equal(ref.decode_png(p.read_bytes()), img)
    io.write_png(str(tmp_path / "t.png"), torch.from_numpy(img))
    assert np.array_equal(ref.decode_png((tmp_path / "t.png").read_bytes()), img)
    for bad in (img.astype(np.float32), img[..., 0], img[..., :2]):
        with pytest.raises(ValueError):
            io.write_png(str(tmp_path / "bad.png"), bad)


def test_render_entry_refuses_before_any_launch(pcc):
    """every refusal of pcc_render_view: a negative status and a message, with no GPU and with pointers that are never read"""
    L = pcc.lib()
    i3 = lambda *v: np.array(v, dtype=np.int32)
    bg = np.array([255, 255, 255], dtype=np.uint8)
    fake = ctypes.c_void_p(4096)                       # non-null, never dereferenced: the call must refuse first
    good = dict(n=10, right=i3(1, 0, 0), up=i3(0, 1, 0), front=i3(0, 0, 1), scale=1, ps=1, H=16, W=16, coords=fake, rgb=fake,
                scratch=fake, nbytes=16 * 16 * 8, image=fake, bg=bg.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda v: v.ctypes.data if isinstance(v, np.ndarray) else v
        rc = L.pcc_render_view(a["coords"], a["rgb"], a["n"], ptr(a["right"]), ptr(a["up"]), ptr(a["front"]), 0, 0, 0, 0, a["scale"],
                               a["ps"], a["H"], a["W"], a["bg"], a["scratch"], a["nbytes"], a["image"], None)
        return rc, L.pcc_last_error().decode()

    cases = [
        (dict(front=i3(0, 0, 2)), "unit"), (dict(up=i3(0, 1, 1)), "unit"), (dict(right=i3(0, 0, 0)), "unit"),
        (dict(up=i3(0, 0, 1), right=i3(1, 0, 0)), "orthogonal"), (dict(right=i3(0, 1, 0)), "orthogonal"),
        (dict(right=i3(-1, 0, 0)), "up x front"),
        (dict(scale=0), "scale"), (dict(scale=65), "scale"), (dict(ps=0), "point_size"), (dict(ps=17), "point_size"),
        (dict(H=0), "H and W"), (dict(W=0), "H and W"), (dict(H=8193), "H and W"), (dict(W=8193), "H and W"),
        (dict(n=2 ** 32 - 1), "points"), (dict(n=-1), "points"),
        (dict(coords=None), "null"), (dict(rgb=None), "null"), (dict(scratch=None), "z-buffer"), (dict(image=None), "image"),
        (dict(nbytes=16 * 16 * 8 - 1), "scratch"), (dict(right=None), "axes"), (dict(bg=None), "background"),
    ]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and "pcc_render_view" in msg and word in msg, (kw, rc, msg)
    assert L.pcc_render_scratch_bytes(16, 16) == 16 * 16 * 8 and L.pcc_render_scratch_bytes(8192, 8192) == 8 * 8192 * 8192
    assert L.pcc_render_scratch_bytes(0, 16) == 0 and L.pcc_render_scratch_bytes(16, 8193) == 0


def test_image_compare_entry_refuses_before_any_launch(pcc):
    L = pcc.lib()
    fake = ctypes.c_void_p(4096)
    tile = L.pcc_image_compare_tile()
    assert tile >= 8
    tiles = lambda h, w: -(-h // tile) * -(-w // tile)
    for h, w in ((7, 7), (tile, tile), (tile + 1, tile), (130, 67), (8192, 8192)):
        assert L.pcc_image_compare_scratch_bytes(h, w) == tiles(h, w) * 64
    assert L.pcc_image_compare_scratch_bytes(6, 40) == 0 and L.pcc_image_compare_scratch_bytes(40, 8193) == 0
    need = L.pcc_image_compare_scratch_bytes(40, 40)
    cases = [((fake, fake, 6, 40, fake, need, fake), "7 x 7"), ((fake, fake, 40, 6, fake, need, fake), "7 x 7"),
             ((fake, fake, 40, 8193, fake, 1 << 40, fake), "at most"),
             ((None, fake, 40, 40, fake, need, fake), "null"), ((fake, None, 40, 40, fake, need, fake), "null"),
             ((fake, fake, 40, 40, None, need, fake), "null"), ((fake, fake, 40, 40, fake, need, None), "null"),
             ((fake, fake, 40, 40, fake, need - 1, fake), "scratch")]
    for args, word in cases:
        rc = L.pcc_image_compare(*args, None)
        msg = L.pcc_last_error().decode()
        assert rc < 0 and "pcc_image_compare" in msg and word in msg, (args, rc, msg)
