"""The reference of the screen-space operators against itself, and what needs no GPU: tests/_sample_reference.py's two
formulations of the back-projection (per point and per pixel) are EQUAL on every case the GPU tests use; the Python entry points
refuse bad arguments before the GPU is touched; io.read_png reads what io.write_png writes and one hand-made PNG per colour type
and filter."""
import struct
import zlib

import numpy as np
import pytest
import torch

import _sample_reference as sr
import _view_reference as vref


@pytest.mark.parametrize("name", sorted(sr.cases()))
def test_two_formulations_agree(name):
    case = sr.cases()[name]
    H, W = sr.case_size(case)
    for k, tolerance in enumerate(sr.TOLERANCES):
        image = sr.random_image(H, W, 4 if k % 2 == 0 else 1, 100 + k, extreme=k == 3)
        a = sr.case_sample(case, image, tolerance)
        b = sr.case_sample(case, image, tolerance, sr.sample_per_pixel)
        for x, y, what in zip(a, b, ("total", "count", "peak")):
            assert np.array_equal(x, y), (name, tolerance, what)
        total, count, peak = a
        assert (total[count == 0] == 0).all() and (peak[count == 0] == sr.NONE).all() and (peak[count > 0] > sr.NONE).all()
        assert (count <= 256).all()


def test_own_pixels_are_the_winner_plane():
    """with own pixels the per-point result is a scatter of the image over the index plane of ``buffers``"""
    case = sr.cases()["off_screen"]
    H, W = sr.case_size(case)
    image = sr.random_image(H, W, 2, 9)
    total, count, _ = sr.case_sample(case, image, None)
    index, depth = sr.camera_buffers(case["xyz"], case["cam"])
    want_t, want_c = np.zeros_like(total), np.zeros_like(count)
    shown = index >= 0
    np.add.at(want_t, index[shown], image[shown].astype(np.int64))
    np.add.at(want_c, index[shown], 1)
    assert np.array_equal(total, want_t) and np.array_equal(count, want_c)
    assert ((depth == sr.OFFSCREEN) == ~shown).all() and shown.any() and (~shown).any()


def test_two_views_fold():
    box = sr.cases()["view_size_1"]["xyz"]
    images = [sr.random_image(40, 44, 3, 1), sr.random_image(40, 44, 3, 2)]
    both = sr.sample_views(box, [sr.FRONT, sr.SIDE], images, 40, 44, tolerance=1)
    one = [sr.sample_views(box, [v], [im], 40, 44, tolerance=1) for v, im in zip((sr.FRONT, sr.SIDE), images)]
    assert np.array_equal(both[0], one[0][0] + one[1][0]) and np.array_equal(both[1], one[0][1] + one[1][1])
    assert np.array_equal(both[2], np.maximum(one[0][2], one[1][2]))


def test_python_refusals_before_the_gpu(pcc):
    """a float image, a size that is not the view's, too many channels, a bad tolerance, a bad list: ValueError from the argument
    checks, which run before a device is asked for"""
    from pcc_amd import render
    cloud = np.array([[0, 0, 0], [1, 2, 3]], dtype=np.int32)
    good = np.zeros((8, 9), dtype=np.uint8)
    cam = render.Camera((0, 0, 50), look_at=(0, 0, 0), fov_y=30, H=8, W=9)
    for images in ([good.astype(np.float32)], [np.zeros((9, 8), dtype=np.uint8)], [np.zeros((8, 9, 5), dtype=np.int32)],
                   [np.zeros((8, 9, 0), dtype=np.int32)], [good, good], good, [np.zeros((8, 9, 1, 1), dtype=np.int32)],
                   [np.full((8, 9), 2 ** 31, dtype=np.int64)], [torch.zeros((8, 9), dtype=torch.float64)]):
        with pytest.raises(ValueError):
            render.sample_views(cloud, ["front"], images, 8, 9)
        with pytest.raises(ValueError):
            render.sample_cameras(cloud, [cam], images)
    for tolerance in (-1, 1.5, "2", 2 ** 31):
        with pytest.raises(ValueError):
            render.sample_views(cloud, ["front"], [good], 8, 9, tolerance=tolerance)
        with pytest.raises(ValueError):
            render.sample_cameras(cloud, [cam], [good], tolerance=tolerance)
    with pytest.raises(ValueError):
        render.sample_views(cloud, [], [], 8, 9)
    with pytest.raises(ValueError):
        render.sample_views(cloud, ["front"], [good], 0, 9)
    with pytest.raises(ValueError):
        render.sample_views(cloud, ["front"], [good], 8, 9, frames=[(0, 1, 2)])
    with pytest.raises(ValueError):
        render.sample_cameras(cloud, cam, [good])
    with pytest.raises(ValueError):
        render.sample_cameras(cloud, [], [])
    with pytest.raises(ValueError):
        render.sample_cameras(cloud, [cam], [good], point_size=0)
    with pytest.raises(ValueError):
        render.sample_views(cloud.astype(np.float32) + 0.5, ["front"], [good], 8, 9)
    with pytest.raises(ValueError):
        render.camera_buffers(cloud, "front")
    with pytest.raises(ValueError):
        render.view_buffers(cloud, (0, 0, 1), (0, 0, 1), 8, 9)
    with pytest.raises(ValueError):
        render.view_buffers(cloud, (0, 0, 1), (0, 1, 0), 8, 9, device="cpu")


# ---- PNG ----
def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def encode_png(img, colour, filters, extra=b"", idat_parts=1):
    """a hand-made PNG of uint8 [H, W, bpp] with filter type filters[y % len] on line y, written from the PNG specification"""
    h, w, bpp = img.shape
    raw = bytearray()
    for y in range(h):
        kind = filters[y % len(filters)]
        raw.append(kind)
        line = img[y].reshape(-1).astype(int)
        prev = img[y - 1].reshape(-1).astype(int) if y else np.zeros(w * bpp, dtype=int)
        for x in range(w * bpp):
            a = line[x - bpp] if x >= bpp else 0
            b = prev[x]
            c = prev[x - bpp] if x >= bpp else 0
            pred = (0, a, b, (a + b) // 2, _paeth(a, b, c), 0)[kind]          # 5: no such filter, for the refusal test
            raw.append((line[x] - pred) & 255)
    z = zlib.compress(bytes(raw))
    cut = [len(z) * k // idat_parts for k in range(idat_parts + 1)]
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour, 0, 0, 0)) + extra
            + b"".join(_chunk(b"IDAT", z[cut[k]:cut[k + 1]]) for k in range(idat_parts)) + _chunk(b"IEND", b""))


def test_read_png_reads_what_write_png_writes(pcc, tmp_path):
    from pcc_amd import io
    rng = np.random.default_rng(0)
    for h, w in ((1, 1), (7, 5), (33, 40)):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        path = str(tmp_path / ("%dx%d.png" % (h, w)))
        io.write_png(path, img)
        back = io.read_png(path)
        assert back.dtype == np.uint8 and np.array_equal(back, img)
        with open(path, "rb") as f:
            raw = f.read()
        assert np.array_equal(io.read_png(raw), img) and np.array_equal(vref.decode_png(raw), img)


@pytest.mark.parametrize("colour,bpp", [(0, 1), (4, 2), (2, 3), (6, 4)])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_read_png_colour_types_and_filters(pcc, colour, bpp, kind):
    from pcc_amd import io
    img = np.random.default_rng(10 * colour + kind).integers(0, 256, size=(6, 7, bpp), dtype=np.uint8)
    back = io.read_png(encode_png(img, colour, [kind]))
    assert back.shape == ((6, 7) if bpp == 1 else (6, 7, bpp)) and np.array_equal(back.reshape(6, 7, bpp), img)


def test_read_png_mixed_filters_chunks_and_refusals(pcc):
    from pcc_amd import io
    img = np.random.default_rng(3).integers(0, 256, size=(11, 9, 3), dtype=np.uint8)
    text = _chunk(b"tEXt", b"Comment\x00hand-made")
    assert np.array_equal(io.read_png(encode_png(img, 2, [4, 3, 2, 1, 0], extra=text, idat_parts=3)), img)
    good = encode_png(img, 2, [0])
    for bad in (good[:-20], b"JFIF" + good[4:], good[:40] + bytes([good[40] ^ 1]) + good[41:],
                encode_png(img, 3, [0], extra=_chunk(b"PLTE", bytes(range(30)))),                 # palette
                encode_png(img, 2, [0], extra=_chunk(b"ABCD", b"")),                              # unknown critical chunk
                encode_png(img, 2, [5]),                                                          # no such filter
                good.replace(struct.pack(">IIBBBBB", 9, 11, 8, 2, 0, 0, 0), struct.pack(">IIBBBBB", 9, 11, 8, 2, 0, 0, 1)),
                b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 9, 11, 16, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(b"")) + _chunk(b"IEND", b"")):
        with pytest.raises(ValueError):
            io.read_png(bad)
