"""render.view_buffers / camera_buffers (csrc/render.hip, pcc_view_buffers / pcc_camera_buffers) on the GPU: the index and depth
planes EQUAL the painter's-loop restatement (tests/_sample_reference.py), and the renderers' images are rgb8[index]."""
import numpy as np
import pytest
import torch

import _camera_reference as cref
import _sample_reference as sr
import _view_reference as vref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (7, 200, 90)
SIGNED = [tuple(s * int(k == a) for k in range(3)) for a in range(3) for s in (1, -1)]
PAIRS = [(f, u) for f in SIGNED for u in SIGNED if sum(a * b for a, b in zip(f, u)) == 0]


def cloud_of(xyz, seed=0):
    rgb = np.random.default_rng(seed).integers(0, 256, size=(len(xyz), 3)).astype(np.float32) / np.float32(255.0)
    return np.concatenate([np.asarray(xyz, dtype=np.float32).reshape(-1, 3), rgb], axis=1)


def planes(got):
    index, depth = got
    assert index.dtype == torch.int32 and depth.dtype == torch.int32 and index.is_cuda and index.shape == depth.shape
    return index.cpu().numpy().astype(np.int64), depth.cpu().numpy().astype(np.int64)


def image_from(index, cloud):
    rgb8 = cref.colours_to_bytes(cloud[:, 3:6])
    img = np.empty(index.shape + (3,), dtype=np.uint8)
    img[:] = np.asarray(BG, dtype=np.uint8)
    img[index >= 0] = rgb8[index[index >= 0]]
    return img


def check_view(xyz, view, H, W, frame=None, point_size=None):
    from pcc_amd import render
    cloud = cloud_of(xyz)
    t = torch.from_numpy(cloud).to(DEV)
    index, depth = planes(render.view_buffers(t, view[0], view[1], H, W, frame=frame, point_size=point_size))
    want_i, want_d = sr.view_buffers(xyz, view[0], view[1], H, W, frame=frame, point_size=point_size)
    assert np.array_equal(index, want_i), "index: %d pixels differ" % int((index != want_i).sum())
    assert np.array_equal(depth, want_d), "depth: %d pixels differ" % int((depth != want_d).sum())
    img = render.render_view(t, view[0], view[1], H, W, frame=frame, point_size=point_size, background=BG).cpu().numpy()
    assert np.array_equal(img, image_from(index, cloud))
    return index, depth


def check_camera(xyz, cam, point_size=1.0):
    from pcc_amd import render
    cloud = cloud_of(xyz)
    t = torch.from_numpy(cloud).to(DEV)
    camera = render.Camera.from_quantised(*cam)
    index, depth = planes(render.camera_buffers(t, camera, point_size=point_size))
    want_i, want_d = sr.camera_buffers(xyz, cam, point_size=point_size)
    assert np.array_equal(index, want_i), "index: %d pixels differ" % int((index != want_i).sum())
    assert np.array_equal(depth, want_d), "depth: %d pixels differ" % int((depth != want_d).sum())
    img = render.render_camera(t, camera, point_size=point_size, background=BG).cpu().numpy()
    assert np.array_equal(img, image_from(index, cloud))
    return index, depth


def test_all_24_axis_pairs(pcc):
    assert len(PAIRS) == 24
    xyz = cref.exactly(257, 24, 24)
    seen = set()
    for view in PAIRS:
        index, depth = check_view(xyz, view, 50, 52, point_size=3)               # scale 2: overlapping squares
        assert (index >= 0).any() and (index < 0).any()
        assert ((depth == sr.OFFSCREEN) == (index < 0)).all()
        seen.add(index.tobytes())
    assert len(seen) == 24


def test_view_sizes_and_scales(pcc):
    xyz = cref.exactly(1000, 24, 5)
    check_view(xyz, sr.FRONT, 81, 76, frame=vref.frame_of(xyz, *sr.FRONT, 81, 76, scale=3), point_size=1)
    check_view(xyz, sr.SIDE, 57, 52, frame=vref.frame_of(xyz, *sr.SIDE, 57, 52, scale=2), point_size=16)
    check_view(xyz, sr.FRONT, 100, 90, frame=(0, 23, 0, 23, 3, -30, 40), point_size=5)      # pushed over the left and bottom edges
    check_view(xyz, sr.FRONT, 1, 1, frame=(0, 23, 0, 23, 1, -11, -12), point_size=3)
    check_view(xyz - 20, sr.FRONT, 33, 257)                                                 # negative depths, more than one block of pixels


def test_cameras(pcc):
    xyz = cref.exactly(1000, cref.BOX, 11)
    for front, up in cref.AXIS_VIEWS:
        index, _ = check_camera(xyz, cref.axis_camera(front, up, 60.0, 80.0, 40, 36))
        assert (index >= 0).any() and (index < 0).any()
    oblique = sr.cases()["off_screen"]                                                      # with voxels far outside the image
    check_camera(oblique["xyz"], oblique["cam"])
    check_camera(xyz, cref.inside_camera(), point_size=2.0)
    index, depth = check_camera(xyz, cref.far_camera())
    assert (index >= 0).sum() > 0 and depth[index >= 0].min() > 256 * 19000
    check_camera(xyz[:300], cref.near_camera())
    rows, cam, _ = cref.clip_case()
    check_camera(rows, cam)
    rows, cam = cref.tie_case()
    check_camera(rows, cam)


def test_row_order_does_not_matter(pcc):
    from pcc_amd import render
    xyz = cref.exactly(600, 24, 3)
    cloud = cloud_of(xyz)
    perm = np.random.default_rng(4).permutation(len(xyz))
    inverse = np.argsort(perm)
    cam = render.Camera.from_quantised(*cref.oblique_camera(60, 52))
    for fn in (lambda c: render.view_buffers(c, *sr.FRONT, 50, 52, point_size=3), lambda c: render.camera_buffers(c, cam)):
        i0, d0 = planes(fn(torch.from_numpy(cloud).to(DEV)))
        i1, d1 = planes(fn(torch.from_numpy(cloud[perm]).to(DEV)))
        assert np.array_equal(d0, d1)
        assert np.array_equal(i0, np.where(i1 >= 0, perm[np.maximum(i1, 0)], -1))           # the same voxel under either numbering
        assert np.array_equal(np.where(i0 >= 0, inverse[np.maximum(i0, 0)], -1), i1)


def test_empty_cloud_is_all_background(pcc):
    from pcc_amd import render
    empty = torch.zeros((0, 6), dtype=torch.float32, device=DEV)
    index, depth = planes(render.view_buffers(empty, *sr.FRONT, 9, 70))
    assert index.shape == (9, 70) and (index == -1).all() and (depth == sr.OFFSCREEN).all()
    index, depth = planes(render.camera_buffers(empty, render.Camera.from_quantised(*cref.oblique_camera(33, 31))))
    assert index.shape == (33, 31) and (index == -1).all() and (depth == sr.OFFSCREEN).all()


def test_c_entry_refusals_write_nothing(pcc):
    from pcc_amd import _lib
    L = pcc.lib()
    H, W, n = 16, 12, 5
    rows = np.zeros((n, 4), dtype=np.int32)
    rows[:, 1:] = cref.exactly(n, 8, 1)
    coords = torch.from_numpy(rows).to(DEV)
    vecs = [np.ascontiguousarray(a, dtype=np.int32) for a in vref.axes(*sr.FRONT)]
    pos, axes_q, focal_q, near_q, _, _ = cref.axis_camera((0, 0, 1), (0, 1, 0), 60.0, 80.0, H, W)
    pos, axes_q = np.asarray(pos, dtype=np.int32), np.asarray(axes_q, dtype=np.int32).reshape(9)
    nbytes = int(L.pcc_render_scratch_bytes(H, W))
    assert nbytes == H * W * 8
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    index = torch.full((H, W), -77, dtype=torch.int32, device=DEV)
    depth = torch.full((H, W), -77, dtype=torch.int32, device=DEV)

    def view(coords_p=coords.data_ptr(), axes=vecs, scale=1, ps=1, h=H, w=W, scratch_p=scratch.data_ptr(), size=nbytes,
             index_p=index.data_ptr(), depth_p=depth.data_ptr(), count=n):
        return L.pcc_view_buffers(coords_p, count, axes[0].ctypes.data if axes[0] is not None else None, axes[1].ctypes.data,
                                  axes[2].ctypes.data, 0, 7, 0, 0, scale, ps, h, w, scratch_p, size, index_p, depth_p, _lib.stream())

    def camera(coords_p=coords.data_ptr(), pos_p=pos.ctypes.data, focal=focal_q, near=near_q, ps_q=16, h=H, w=W,
               scratch_p=scratch.data_ptr(), size=nbytes, index_p=index.data_ptr(), depth_p=depth.data_ptr()):
        return L.pcc_camera_buffers(coords_p, n, pos_p, axes_q.ctypes.data, focal, near, h, w, ps_q, scratch_p, size, index_p, depth_p,
                                    _lib.stream())

    skew = [vecs[0], vecs[1], np.array([0, 1, 0], dtype=np.int32)]
    long_axis = [vecs[0], vecs[1], np.array([0, 0, 2], dtype=np.int32)]
    left_handed = [-vecs[0], vecs[1], vecs[2]]
    bad = [view(coords_p=None), view(axes=[None, vecs[1], vecs[2]]), view(axes=skew), view(axes=long_axis), view(axes=left_handed),
           view(scale=0), view(scale=65), view(ps=0), view(ps=17), view(h=0), view(w=8193), view(scratch_p=None), view(size=nbytes - 1),
           view(index_p=None), view(depth_p=None), view(count=-1),
           camera(coords_p=None), camera(pos_p=None), camera(focal=0), camera(focal=(1 << 20) + 1), camera(near=0), camera(ps_q=0),
           camera(ps_q=257), camera(h=0), camera(w=8193), camera(scratch_p=None), camera(size=nbytes - 1), camera(index_p=None),
           camera(depth_p=None)]
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in bad), bad
    assert (index == -77).all() and (depth == -77).all()
    assert view() == 0 and camera() == 0
    torch.cuda.synchronize()
    assert (index != -77).all() and (depth != -77).all()
    # n == 0 with a null cloud is valid: all background
    assert view(coords_p=None, count=0) == 0
    torch.cuda.synchronize()
    assert (index == -1).all() and (depth == sr.OFFSCREEN).all()
