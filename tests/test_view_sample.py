"""render.sample_views / sample_cameras (csrc/render.hip, pcc_view_sample / pcc_camera_sample) on the GPU: total, count and peak
EQUAL the painter's-loop restatement (tests/_sample_reference.py) on every case — they are integers, so equality is the bound —
and tie to the operators that already exist: ``won``, ``behind`` and the index plane."""
import numpy as np
import pytest
import torch

import _camera_reference as cref
import _sample_reference as sr
import _view_reference as vref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sr.cases()

# the reference's own tallies per case and tolerance (own, 0, 3, 2^31 - 2): (rows with count > 0, rows with count == 0).  Pinned so
# that a case cannot pass by being all-empty or all-full: both are nonzero wherever the case is meant to have both.
TALLIES = {
    "clip": [(296, 1240), (296, 1240), (326, 1210), (326, 1210)],
    "tie": [(4, 1), (4, 1), (5, 0), (5, 0)],
    "off_screen": [(79, 625), (111, 593), (207, 497), (700, 4)],
    "near_plane": [(40, 560), (40, 560), (55, 545), (67, 533)],
    "camera_1x1": [(1, 299), (3, 297), (14, 286), (91, 209)],
    "view_size_1": [(481, 519), (481, 519), (584, 416), (1000, 0)],
    "view_size_16": [(61, 939), (67, 933), (191, 809), (1000, 0)],
    "view_off_screen": [(245, 755), (245, 755), (301, 699), (516, 484)],
    "view_1x1": [(1, 999), (1, 999), (6, 994), (16, 984)],
}


def gpu_sample(case, image, tolerance, xyz=None):
    from pcc_amd import render
    xyz = case["xyz"] if xyz is None else xyz
    cloud = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.int32)).to(DEV)
    if case["kind"] == "camera":
        got = render.sample_cameras(cloud, [render.Camera.from_quantised(*case["cam"])], [image], point_size=case["point_size"],
                                    tolerance=tolerance)
    else:
        got = render.sample_views(cloud, [case["view"]], [image], case["H"], case["W"], frames=[case["frame"]],
                                  point_size=case["point_size"], tolerance=tolerance)
    total, count, peak = got
    C = 1 if image.ndim == 2 else image.shape[2]
    assert total.dtype == torch.int64 and count.dtype == torch.int32 and peak.dtype == torch.int32 and total.is_cuda
    assert tuple(total.shape) == (len(xyz), C) and tuple(count.shape) == (len(xyz),) and tuple(peak.shape) == (len(xyz), C)
    return tuple(t.cpu().numpy().astype(np.int64) for t in got)


def gpu_visibility(case):
    from pcc_amd import render
    cloud = torch.from_numpy(np.ascontiguousarray(case["xyz"], dtype=np.int32)).to(DEV)
    if case["kind"] == "camera":
        out = render.camera_visibility(cloud, [render.Camera.from_quantised(*case["cam"])], point_size=case["point_size"])
    else:
        out = render.visibility(cloud, [case["view"]], case["H"], case["W"], frames=[case["frame"]], point_size=case["point_size"])
    return out[0].cpu().numpy().astype(np.int64), out[1].cpu().numpy().astype(np.int64)


def gpu_index(case):
    from pcc_amd import render
    cloud = torch.from_numpy(np.ascontiguousarray(case["xyz"], dtype=np.int32)).to(DEV)
    if case["kind"] == "camera":
        return render.camera_buffers(cloud, render.Camera.from_quantised(*case["cam"]), point_size=case["point_size"])[0]
    return render.view_buffers(cloud, *case["view"], case["H"], case["W"], frame=case["frame"], point_size=case["point_size"])[0]


def equal(got, want, what):
    for g, w, name in zip(got, want, ("total", "count", "peak")):
        assert np.array_equal(g, w), "%s: %s differs in %d places" % (what, name, int((g != w).sum()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_equal_to_the_reference(pcc, name):
    """every case at the four tolerances with four channels, one channel, and values at +-(2^31 - 1)"""
    case = CASES[name]
    H, W = sr.case_size(case)
    image, extreme = sr.random_image(H, W, 4, 40), sr.random_image(H, W, 4, 41, extreme=True)
    behind, won = gpu_visibility(case)
    index = gpu_index(case)
    for k, tolerance in enumerate(sr.TOLERANCES):
        want = sr.case_sample(case, image, tolerance)
        assert sr.tallies(want[1]) == TALLIES[name][k], (name, tolerance, sr.tallies(want[1]))
        got = gpu_sample(case, image, tolerance)
        equal(got, want, "%s tolerance %r, 4 channels" % (name, tolerance))
        equal(gpu_sample(case, image[:, :, 0], tolerance), (want[0][:, :1], want[1], want[2][:, :1]), "%s tolerance %r, 1 channel" % (name, tolerance))
        equal(gpu_sample(case, extreme, tolerance), sr.case_sample(case, extreme, tolerance), "%s tolerance %r, extreme" % (name, tolerance))
        total, count, peak = got
        assert (total[count == 0] == 0).all() and (peak[count == 0] == sr.NONE).all()
        # the ties to the operators that exist
        if tolerance is None:
            assert np.array_equal(count, won)
            shown = index >= 0
            scatter = torch.zeros((len(case["xyz"]), 4), dtype=torch.int64, device=DEV)
            scatter.index_add_(0, index[shown].long(), torch.from_numpy(image).to(DEV)[shown].long())
            assert np.array_equal(total, scatter.cpu().numpy())
        else:
            assert np.array_equal(count > 0, behind <= tolerance)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_counts_around_a_workgroup(pcc, n):
    xyz = cref.exactly(n, 24, 500 + n)
    case = dict(kind="view", xyz=xyz, view=sr.SIDE, H=30, W=28, frame=(0, 23, 0, 23, 1, 2, 3), point_size=3)
    for C in (1, 2, 3, 4):
        image = sr.random_image(30, 28, C, n + C)
        equal(gpu_sample(case, image, 1), sr.case_sample(case, image, 1), "n %d, %d channels" % (n, C))


def test_image_kinds(pcc):
    """bool, uint8 and int64 images, as arrays and as tensors on either device, are the same image as int32"""
    case = CASES["view_size_1"]
    H, W = sr.case_size(case)
    mask = sr.random_image(H, W, 1, 3)[:, :, 0] > 0
    want = sr.case_sample(case, mask.astype(np.int32), 0)
    for image in (mask, mask.astype(np.uint8), mask.astype(np.int64), torch.from_numpy(mask), torch.from_numpy(mask).to(DEV),
                  torch.from_numpy(mask.astype(np.int16)).to(DEV)[:, :, None]):
        equal(gpu_sample(case, image, 0), want, "%s %s" % (type(image).__name__, image.dtype))


def test_two_views_accumulate(pcc):
    from pcc_amd import render
    xyz = CASES["view_size_1"]["xyz"]
    cloud = torch.from_numpy(xyz.astype(np.int32)).to(DEV)
    H, W = 40, 44
    images = [sr.random_image(H, W, 3, 1), sr.random_image(H, W, 3, 2)]
    views = [sr.FRONT, sr.SIDE]
    for tolerance in (None, 1):
        both = [t.cpu().numpy().astype(np.int64) for t in render.sample_views(cloud, views, images, H, W, tolerance=tolerance)]
        one = [[t.cpu().numpy().astype(np.int64) for t in render.sample_views(cloud, [v], [im], H, W, tolerance=tolerance)]
               for v, im in zip(views, images)]
        assert np.array_equal(both[0], one[0][0] + one[1][0]) and np.array_equal(both[1], one[0][1] + one[1][1])
        assert np.array_equal(both[2], np.maximum(one[0][2], one[1][2]))
        equal(both, sr.sample_views(xyz, views, images, H, W, tolerance=tolerance), "two views")
        assert (one[0][1] > 0).any() and (one[0][1] == 0).any()
    cams = [cref.oblique_camera(60, 52), cref.axis_camera((1, 0, 0), (0, 1, 0), 60.0, 80.0, 40, 36)]
    images = [sr.random_image(60, 52, 2, 3), sr.random_image(40, 36, 2, 4)]
    got = render.sample_cameras(cloud, [render.Camera.from_quantised(*c) for c in cams], images, tolerance=2)
    equal([t.cpu().numpy().astype(np.int64) for t in got], sr.sample_cameras(xyz, cams, images, tolerance=2), "two cameras")


def test_permuting_the_rows_permutes_the_outputs(pcc):
    for name in ("off_screen", "view_size_16"):
        case = CASES[name]
        H, W = sr.case_size(case)
        image = sr.random_image(H, W, 2, 8)
        perm = np.random.default_rng(9).permutation(len(case["xyz"]))
        for tolerance in (None, 3):
            a = gpu_sample(case, image, tolerance)
            b = gpu_sample(case, image, tolerance, xyz=case["xyz"][perm])
            equal(b, [x[perm] for x in a], name)


def test_empty_cloud(pcc):
    from pcc_amd import render
    empty = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    total, count, peak = render.sample_views(empty, ["front"], [np.zeros((8, 9, 2), dtype=np.int32)], 8, 9)
    assert tuple(total.shape) == (0, 2) and tuple(count.shape) == (0,) and tuple(peak.shape) == (0, 2)


def c_entry(pcc, rows, case, picture, tolerance, accumulate, fill, over=None):
    """pcc_view_sample / pcc_camera_sample themselves on rows (batch, x, y, z) AS GIVEN -> (rc, total, count, peak); ``fill``: what
    the three outputs hold before the call; ``over``: arguments replaced (null pointers, a short scratch, bad values)"""
    from pcc_amd import _lib
    L = pcc.lib()
    n = rows.shape[0]
    H, W = sr.case_size(case)
    C = picture.shape[2]
    coords = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(DEV)
    img = torch.from_numpy(np.ascontiguousarray(picture, dtype=np.int32)).to(DEV)
    total = torch.from_numpy(np.ascontiguousarray(fill[0], dtype=np.int64)).to(DEV)
    count = torch.from_numpy(np.ascontiguousarray(fill[1], dtype=np.int32)).to(DEV)
    peak = torch.from_numpy(np.ascontiguousarray(fill[2], dtype=np.int32)).to(DEV)
    nbytes = int(L.pcc_render_scratch_bytes(H, W))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    a = dict(coords=coords.data_ptr(), n=n, H=H, W=W, scratch=scratch.data_ptr(), nbytes=nbytes, image=img.data_ptr(), channels=C,
             tolerance=sr_tolerance(tolerance), total=total.data_ptr(), count=count.data_ptr(), peak=peak.data_ptr())
    a.update(over or {})
    torch.cuda.synchronize()
    if case["kind"] == "camera":
        pos, axes_q, focal_q, near_q, _, _ = case["cam"]
        pos, axes_q = np.asarray(pos, dtype=np.int32), np.asarray(axes_q, dtype=np.int32).reshape(9)
        rc = L.pcc_camera_sample(a["coords"], a["n"], pos.ctypes.data, axes_q.ctypes.data, a.get("focal", focal_q), near_q, a["H"], a["W"],
                                 cref.ps_q_of(case["point_size"]), a["scratch"], a["nbytes"], accumulate, a["image"], a["channels"],
                                 a["tolerance"], a["total"], a["count"], a["peak"], _lib.stream())
    else:
        vecs = [np.ascontiguousarray(v, dtype=np.int32) for v in vref.axes(*case["view"])]
        u_min, _, _, v_max, scale, ox, oy = case["frame"]
        rc = L.pcc_view_sample(a["coords"], a["n"], vecs[0].ctypes.data, vecs[1].ctypes.data, vecs[2].ctypes.data, u_min, v_max, ox, oy,
                               a.get("scale", scale), case["point_size"], a["H"], a["W"], a["scratch"], a["nbytes"], accumulate, a["image"],
                               a["channels"], a["tolerance"], a["total"], a["count"], a["peak"], _lib.stream())
    torch.cuda.synchronize()
    return rc, total.cpu().numpy(), count.cpu().numpy().astype(np.int64), peak.cpu().numpy().astype(np.int64)


def sr_tolerance(tolerance):
    return -1 if tolerance is None else tolerance


def sorted_rows(xyz):
    rows = np.zeros((len(xyz), 4), dtype=np.int32)
    rows[:, 1:] = np.asarray(xyz)[sr.canonical_order(xyz)]
    return rows


@pytest.mark.parametrize("name", ["off_screen", "view_off_screen"])
def test_c_entry_accumulates_and_refuses(pcc, name):
    case = CASES[name]
    if name == "off_screen":                        # the entry itself also takes rows beyond the coordinate range: they draw nothing
        case = dict(case, xyz=cref.oblique_case(n=700)[0])
        assert (np.abs(case["xyz"]) > sr.COORD_LIMIT).any()
    H, W = sr.case_size(case)
    image = sr.random_image(H, W, 3, 12)
    rows = sorted_rows(case["xyz"])
    n = rows.shape[0]
    order = sr.canonical_order(case["xyz"])
    want = [x[order] for x in sr.case_sample(case, image, 3)]
    rng = np.random.default_rng(13)
    fill = (rng.integers(-2 ** 40, 2 ** 40, size=(n, 3)), rng.integers(0, 1000, size=n), rng.integers(-1500, 1500, size=(n, 3)))
    # accumulate == 0 overwrites whatever was there
    rc, total, count, peak = c_entry(pcc, rows, case, image, 3, 0, fill)
    assert rc == 0
    equal((total, count, peak), want, "overwrite")
    # accumulate != 0 adds to the totals and counts and keeps the larger peak; a row nothing counted for keeps what it held
    rc, total, count, peak = c_entry(pcc, rows, case, image, 3, 1, fill)
    assert rc == 0
    equal((total, count, peak), (fill[0] + want[0], fill[1] + want[1], np.maximum(fill[2], want[2])), "accumulate")
    assert (want[1] == 0).any() and np.array_equal(peak[want[1] == 0], fill[2][want[1] == 0])
    # refusals, before any launch: nothing is written
    bad = [dict(coords=None), dict(total=None), dict(count=None), dict(peak=None), dict(image=None), dict(scratch=None),
           dict(nbytes=H * W * 8 - 1), dict(channels=0), dict(channels=5), dict(tolerance=-2), dict(H=0), dict(W=8193), dict(n=-1),
           dict(focal=0) if case["kind"] == "camera" else dict(scale=0)]
    for over in bad:
        rc, total, count, peak = c_entry(pcc, rows, case, image, 3, 0, fill, over)
        assert rc == -1, over
        assert np.array_equal(total, fill[0]) and np.array_equal(count, fill[1]) and np.array_equal(peak, fill[2]), over
    # n == 0 with null arrays launches nothing
    rc, _, _, _ = c_entry(pcc, rows, case, image, 3, 0, fill, dict(coords=None, n=0, total=None, count=None, peak=None))
    assert rc == 0
