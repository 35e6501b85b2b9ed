"""Plain numpy restatements of the view renderer and the view metrics (pcc_amd.render): what tests/test_render.py,
tests/test_view_metrics.py and tests/test_view_harness.py hold the GPU operators to.  Written from the operators'
specification, not from their code: a painter's loop instead of a z-buffer, sliding windows instead of tiles.
No scipy, no imaging package."""
import math
import struct
import zlib

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

# scikit-image's yuv_from_rgb (recalled, not pinned: the package is not a dependency)
YUV_FROM_RGB = ((0.299, 0.587, 0.114), (-0.14714119, -0.28886916, 0.43601035), (0.61497538, -0.51496512, -0.10001026))


def axes(front, up):
    """-> (right, up, front) integer vectors, right = up x front"""
    f, u = np.asarray(front, dtype=np.int64), np.asarray(up, dtype=np.int64)
    return np.cross(u, f), u, f


def canonical(cloud):
    """[N, 6] float cloud -> (xyz int64 [N, 3], rgb uint8 [N, 3]) in ascending (x, y, z) order, colours as
    clamp(rint(float32(c) * 255), 0, 255)"""
    cloud = np.asarray(cloud)
    xyz = np.rint(cloud[:, :3]).astype(np.int64)
    rgb = np.clip(np.rint(cloud[:, 3:6].astype(np.float32) * np.float32(255.0)), 0, 255).astype(np.uint8)
    order = np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0]))
    return xyz[order], rgb[order]


def frame_of(xyz, front, up, H, W, scale=None):
    """(u_min, u_max, v_min, v_max, scale, ox, oy) of a cloud's bounding box"""
    r, u, _ = axes(front, up)
    uu, vv = xyz @ r, xyz @ u
    u_min, u_max, v_min, v_max = int(uu.min()), int(uu.max()), int(vv.min()), int(vv.max())
    wu, wv = u_max - u_min + 1, v_max - v_min + 1
    if scale is None:
        scale = max(1, min(W // wu, H // wv))
    return u_min, u_max, v_min, v_max, scale, (W - wu * scale) // 2, (H - wv * scale) // 2


def render(xyz, rgb, front, up, H, W, frame, point_size=None, background=(255, 255, 255)):
    """Painter's loop over rows given in canonical order: far to near and, among equal depth, the higher row first; every
    point paints its square, clipped to the image, and later paint overwrites."""
    r, u, f = axes(front, up)
    u_min, _, _, v_max, scale, ox, oy = frame
    ps = scale if point_size is None else point_size
    img = np.empty((H, W, 3), dtype=np.uint8)
    img[:] = np.asarray(background, dtype=np.uint8)
    n = xyz.shape[0]
    if n == 0:
        return img
    uu, vv, dd = xyz @ r, xyz @ u, xyz @ f
    order = np.lexsort((-np.arange(n), dd))              # ascending depth; among equal depth descending row
    for i in order:
        c0, r0 = (int(uu[i]) - u_min) * scale + ox, (v_max - int(vv[i])) * scale + oy
        c1, r1 = c0 + ps, r0 + ps
        if c1 <= 0 or r1 <= 0 or c0 >= W or r0 >= H:
            continue
        img[max(r0, 0):min(r1, H), max(c0, 0):min(c1, W)] = rgb[i]
    return img


def render_cloud(cloud, front, up, H, W, frame=None, point_size=None, background=(255, 255, 255)):
    """render() of an [N, 6] float cloud in any row order; frame=None frames the cloud itself"""
    xyz, rgb = canonical(cloud)
    if frame is None:
        frame = frame_of(xyz, front, up, H, W)
    return render(xyz, rgb, front, up, H, W, frame, point_size, background)


def yuv(img):
    """uint8 [H, W, 3] -> float64 [H, W, 3]: f = byte / 255.0, channel = (f_r m0 + f_g m1) + f_b m2, elementwise"""
    f = img.astype(np.float64) / 255.0
    out = np.empty_like(f)
    for k, (m0, m1, m2) in enumerate(YUV_FROM_RGB):
        out[..., k] = (f[..., 0] * m0 + f[..., 1] * m1) + f[..., 2] * m2
    return out


def ssim_map(x, y):
    """the SSIM map of structural_similarity(win_size=7, data_range=1.0, gaussian_weights=False,
    use_sample_covariance=True) on its crop: [H - 6, W - 6] float64 for one channel"""
    mean = lambda a: sliding_window_view(a, (7, 7)).mean(axis=(-1, -2))
    ux, uy, uxx, uyy, uxy = mean(x), mean(y), mean(x * x), mean(y * y), mean(x * y)
    cov_norm = 49.0 / 48.0
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = 1e-4, 9e-4
    return ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def view_metrics(ref_img, img, data_range=None):
    """{"psnr", "ssim", "y_mse", "u_mse", "v_mse", "data_range"} of two uint8 [H, W, 3] images"""
    a, b = yuv(np.asarray(ref_img)), yuv(np.asarray(img))
    err = (a - b) ** 2
    mse = float(err.mean())
    if data_range is None:
        data_range = 1.0 if a.min() >= 0 else 2.0
    ssim = float(np.mean([ssim_map(a[..., k], b[..., k]).mean() for k in range(3)]))
    psnr = math.inf if mse == 0 else 10.0 * math.log10(data_range ** 2 / mse)
    chan = [float(err[..., k].mean()) for k in range(3)]
    return {"psnr": psnr, "ssim": ssim, "y_mse": chan[0], "u_mse": chan[1], "v_mse": chan[2], "data_range": data_range}


def decode_png(raw):
    """a PNG as write_png writes it (8-bit RGB, filter 0 on every line) -> uint8 [H, W, 3]; checks every chunk's CRC"""
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [c[0] for c in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)
