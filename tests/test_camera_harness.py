"""The camera views through the Python interface: render.render_camera / camera_visibility on the CONFIG1 shell EQUAL to the
restatement (tests/_camera_reference.py) for an array and for a GPU tensor, harness.evaluate_view_dependent with ``camera``
(the fixture of tests/test_visibility_harness.py: seeded model, the same shell) judged by the camera's images, unchanged rows
with ``camera=None``, and the quality maps built from the outputs.  The seeded weights have no rate-distortion meaning, so
nothing is asserted about the order of rates or qualities between the rows."""
import math

import numpy as np
import pytest
import torch

import _camera_reference as ref
import _view_reference as vref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 160, 96
Q_A, Q_G = 0.8, 0.4
CAMERA = dict(position=(60.0, 45.0, 110.0), look_at=(15.5, 15.5, 15.5), fov_y=30.0, H=H, W=W)        # the shell about 85 pixels across
SIDE = dict(position=(-90.0, 15.5, 15.5), look_at=(15.5, 15.5, 15.5), fov_y=30.0, H=64, W=64)


@pytest.fixture(scope="module")
def shell(pcc):
    from pcc_amd import synthetic as syn
    return syn.sphere_shell(**syn.CONFIG1)


@pytest.fixture(scope="module")
def wanted(shell):
    """the restatement's answers, computed once"""
    q, q2 = ref.quantise(**CAMERA), ref.quantise(**SIDE)
    xyz = shell[:, :3].astype(np.int64)
    return {"q": q, "q2": q2, "image": ref.render_camera(shell, q), "one": ref.camera_visibility(xyz, [q]),
            "two": ref.camera_visibility(xyz, [q, q2]), "wide": ref.camera_visibility(xyz, [q], point_size=3)}


def test_python_api_equals_the_reference(pcc, shell, wanted):
    from pcc_amd import render
    cam, cam2 = render.Camera(**CAMERA), render.Camera(**SIDE)
    assert tuple(cam.quantised()) == wanted["q"] and tuple(cam2.quantised()) == wanted["q2"]
    perm = np.random.default_rng(3).permutation(len(shell))
    for cloud in (shell, torch.from_numpy(shell).to(DEV), torch.from_numpy(shell[perm]).to(DEV)):
        img = render.render_camera(cloud, cam)
        assert img.dtype == torch.uint8 and tuple(img.shape) == (H, W, 3) and img.is_cuda
        assert np.array_equal(img.cpu().numpy(), wanted["image"])
    shown = (wanted["image"] != 255).any(axis=2)
    assert 3000 < int(shown.sum()) < H * W // 2
    for cloud, order in ((shell[:, :3], None), (torch.from_numpy(shell).to(DEV), None), (torch.from_numpy(shell[perm, :3]).to(DEV), perm)):
        for cams, key, kw in (([cam], "one", {}), ([cam, cam2], "two", {}), ([cam], "wide", {"point_size": 3})):
            got = render.camera_visibility(cloud, cams, **kw)
            for g, want in zip(got, wanted[key]):
                assert g.dtype == torch.int32 and g.is_cuda and tuple(g.shape) == (len(shell),)
                assert np.array_equal(g.cpu().numpy(), want if order is None else want[order])
    b, w, d = wanted["one"]
    assert (b < ref.OFFSCREEN).all() and 1000 < int((b == 0).sum()) < 4000 and (b > 10).any() and int(w.sum()) == int(shown.sum())
    assert (wanted["two"][0] <= b).all() and (wanted["two"][0] < b).any()
    # another background, an empty cloud
    img = render.render_camera(shell, cam, background=(1, 2, 3)).cpu().numpy()
    assert np.array_equal(img[shown], wanted["image"][shown]) and (img[~shown] == np.array([1, 2, 3], dtype=np.uint8)).all()
    assert (render.render_camera(np.zeros((0, 6), dtype=np.float32), cam).cpu().numpy() == 255).all()
    assert [tuple(t.shape) for t in render.camera_visibility(np.zeros((0, 3), dtype=np.float32), [cam])] == [(0,)] * 3


def test_quality_maps_accept_the_outputs(pcc, shell, wanted):
    from pcc_amd import q_map, render
    cam = render.Camera(**CAMERA)
    xyz = shell[:, :3].astype(np.int64)
    coords = torch.from_numpy(np.concatenate([np.zeros((len(xyz), 1), dtype=np.int64), xyz], axis=1)).to(torch.int32).to(DEV)
    cmap = pcc.CoordMap(coords, 1, nbatch=1)
    rows = cmap.coords[:, 1:4]
    behind, won, depth = render.camera_visibility(rows, [cam])
    want_b, _, want_d = ref.camera_visibility(rows.cpu().numpy(), [wanted["q"]])
    assert np.array_equal(behind.cpu().numpy(), want_b) and np.array_equal(depth.cpu().numpy(), want_d)
    import _visibility_reference as visref
    Q = q_map.visibility_map(cmap, behind, Q_G, Q_A, tolerance=1, falloff=4, floor=0.25)
    s = visref.score(want_b, 1, 4, 0.25)
    assert Q.F.is_cuda and Q.F.cpu().numpy().tobytes() == np.stack([Q_G * s, Q_A * s], axis=1).astype(np.float32).tobytes()
    full = 1.25 * cam.focal * 256.0 / float(want_d.min())                # the nearest voxel scores 0.8, the rest less
    Q = q_map.distance_map(cmap, depth, cam.focal, Q_G, Q_A, full=full, floor=0.1)
    s = ref.distance_score(want_d, cam.focal, full, 0.1)
    assert 0.5 < s.min() < s.max() <= 0.8 + 1e-12
    assert Q.F.is_cuda and Q.F.cpu().numpy().tobytes() == np.stack([Q_G * s, Q_A * s], axis=1).astype(np.float32).tobytes()


@pytest.fixture(scope="module")
def run(pcc, shell, tmp_path_factory):
    from pcc_amd import render
    from pcc_amd import synthetic as syn
    from pcc_amd.harness import evaluate_view_dependent
    model = syn.make_model(seed=0, device=DEV)
    model.update()
    data = {"src": {"points": torch.from_numpy(shell[None, :, :3]), "colors": torch.from_numpy(shell[None, :, 3:])}}
    cam = render.Camera(**CAMERA)
    details = {}
    rows = evaluate_view_dependent("exp", model, data, Q_A, Q_G, DEV, str(tmp_path_factory.mktemp("camera")), details=details,
                                   camera=cam, visibility={}, facing={})
    return {"rows": rows, "details": details, "model": model, "data": data, "camera": cam}


def test_camera_rows(run, shell, wanted):
    rows, details = run["rows"], run["details"]
    assert list(rows) == ["uniform", "view", "roi", "facing", "visible"]
    for key, row in rows.items():
        assert set(row) == {"bpp", "q_a", "q_g", "key", "psnr", "ssim"} and row["key"] == key
        assert math.isfinite(row["bpp"]) and row["bpp"] > 0 and math.isfinite(row["psnr"]) and math.isfinite(row["ssim"])
        assert -1.0 <= row["ssim"] <= 1.0
    # judged by the camera's images: the source's is the restatement's, every reconstruction's is the restatement's of that cloud
    assert np.array_equal(details["source"][1].cpu().numpy(), wanted["image"])
    for key in rows:
        rec, img = details[key]
        want = ref.render_camera(rec.cpu().numpy(), wanted["q"])
        assert tuple(img.shape) == (H, W, 3) and np.array_equal(img.cpu().numpy(), want)
        m = vref.view_metrics(wanted["image"], want)
        assert abs(rows[key]["ssim"] - m["ssim"]) <= 1e-9 and abs(rows[key]["psnr"] - m["psnr"]) <= 1e-9
    # the coded visibility map is camera_visibility's of the camera itself
    behind, score = details["visibility"]
    import _visibility_reference as visref
    assert np.array_equal(behind.cpu().numpy(), wanted["one"][0])
    assert score.cpu().numpy().tobytes() == visref.score(wanted["one"][0], 2, 8, 0.0).tobytes()


def test_camera_options_and_refusals(run, wanted, tmp_path):
    from pcc_amd import render
    from pcc_amd.harness import evaluate_view_dependent
    args = ("exp2", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path))
    details = {}
    rows = evaluate_view_dependent(*args, camera=run["camera"], details=details,
                                   visibility={"cameras": [run["camera"], render.Camera(**SIDE)], "tolerance": 0, "falloff": 0})
    assert list(rows) == ["uniform", "view", "roi", "visible"]
    assert np.array_equal(details["visibility"][0].cpu().numpy(), wanted["two"][0])
    for key in ("uniform", "view", "roi"):                               # the default gradient and region follow the camera alone
        assert rows[key] == run["rows"][key]
    for bad in (dict(camera=run["camera"], visibility={"views": ["front"]}), dict(camera=run["camera"], visibility={"cameras": []}),
                dict(camera="front"), dict(visibility={"cameras": [run["camera"]]})):
        with pytest.raises(ValueError):
            evaluate_view_dependent(*args, **bad)


def test_without_a_camera_nothing_changes(run, tmp_path):
    from pcc_amd.harness import evaluate_view_dependent
    args = ("exp3", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path))
    kw = dict(view="front", H=H, W=W, visibility={"views": ["front"]})
    plain, none = {}, {}
    a = evaluate_view_dependent(*args, details=plain, **kw)
    b = evaluate_view_dependent(*args, details=none, camera=None, **kw)
    assert list(a) == ["uniform", "view", "roi", "visible"] and a == b
    for key in ("source", "uniform", "view", "roi", "visible"):
        assert torch.equal(plain[key][1], none[key][1])
    assert torch.equal(plain["visibility"][0], none["visibility"][0])
