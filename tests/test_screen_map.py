"""Screen-space quality maps end to end: q_map.image_score / image_map / box_image / gaze_image against numpy restatements
(tests/_sample_reference.py; byte-equal in float64), and harness.evaluate_view_dependent with ``screen`` on the fixture of
tests/test_visibility_harness.py (seeded model, the CONFIG1 shell, 160 x 96, front view).  The coded map is held to the
painter's-loop reference, the region metrics to the numpy masked metrics on the painter's-loop images within 1e-9 (the bound of
tests/test_view_metrics.py).  The seeded weights have no rate-distortion meaning: nothing is asserted about which row scores
better."""
import math

import numpy as np
import pytest
import torch

import _camera_reference as cref
import _sample_reference as sr
import _view_reference as vref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 160, 96
Q_A, Q_G = 0.8, 0.4
FRONT = ((0, 0, 1), (0, 1, 0))
BOX = (40, 110, 20, 60)
TODAY = {"bpp", "q_a", "q_g", "key", "psnr", "ssim"}


def test_image_score_and_makers_match_numpy(pcc):
    from pcc_amd import q_map
    rng = np.random.default_rng(0)
    n = 500
    count = rng.integers(0, 5, size=n).astype(np.int32)
    total = rng.integers(-2000, 300 * 256, size=(n, 3)).astype(np.int64)
    peak = np.where(count[:, None] > 0, rng.integers(-50, 400, size=(n, 3)), sr.NONE).astype(np.int32)
    assert (count == 0).any() and (peak > 255).any() and (peak[count > 0] < 0).any()
    for reduce in ("max", "mean"):
        for channel, scale, floor in ((0, 255, 0.0), (2, 100, 0.25), (1, 1000.5, 1.0)):
            got = q_map.image_score(torch.from_numpy(total), torch.from_numpy(count), torch.from_numpy(peak), reduce, channel, scale, floor)
            want = sr.image_score(total, count, peak, reduce, channel, scale, floor)
            assert got.dtype == torch.float64 and got.numpy().tobytes() == want.tobytes()
            assert float(got.min()) >= floor and float(got.max()) <= 1.0 and (got.numpy()[count == 0] == floor).all()
    for bad in (dict(reduce="sum"), dict(scale=0), dict(floor=1.5), dict(channel=3)):
        with pytest.raises(ValueError):
            q_map.image_score(torch.from_numpy(total), torch.from_numpy(count), torch.from_numpy(peak), **bad)
    with pytest.raises(ValueError):
        q_map.image_score(torch.from_numpy(total).double(), torch.from_numpy(count), torch.from_numpy(peak))
    with pytest.raises(ValueError):
        q_map.image_score(torch.from_numpy(total), torch.from_numpy(count[:-1]), torch.from_numpy(peak))
    for box in ((2, 5, 1, 4), (-3, 4, 5, 99), (0, 0, 0, 0), (6, 2, 1, 4), (0, 9, 0, 11)):
        got = q_map.box_image(9, 11, box)
        assert got.dtype == np.uint8 and np.array_equal(got, sr.box_image(9, 11, box))
    for gaze, radius, falloff in (((4, 5), 2, 3), ((-2.5, 3.25), 1.5, 6.0), ((4, 5), 3, 0), ((0, 0), 0, 1)):
        got = q_map.gaze_image(9, 11, gaze, radius, falloff)
        assert got.dtype == np.uint8 and np.array_equal(got, sr.gaze_image(9, 11, gaze, radius, falloff))
    assert set(np.unique(q_map.gaze_image(30, 30, (15, 15), 4, 8))) > {0, 255}


def test_image_map_on_a_coordinate_map(pcc):
    from pcc_amd import q_map, render
    xyz = cref.exactly(700, 24, 5)
    coords = torch.cat([torch.zeros((700, 1), dtype=torch.int32), torch.from_numpy(xyz.astype(np.int32))], dim=1).to(DEV)
    cmap = pcc.CoordMap(coords, 1, nbatch=1)
    rows = cmap.coords[:, 1:4]
    image = q_map.gaze_image(50, 52, (20, 30), 5, 12)
    sampled = render.sample_views(rows, [FRONT], [image], 50, 52, tolerance=2)
    got = q_map.image_map(cmap, *sampled, 0.4, 0.8, reduce="mean", floor=0.1)
    want_s = sr.image_score(*sr.sample_views(rows.cpu().numpy(), [FRONT], [image], 50, 52, tolerance=2), reduce="mean", floor=0.1)
    want = np.stack([0.4 * want_s, 0.8 * want_s], axis=1).astype(np.float32)
    assert got.F.dtype == torch.float32 and got.F.cpu().numpy().tobytes() == want.tobytes()
    assert len(set(want_s.tolist())) > 3
    with pytest.raises(ValueError):
        q_map.image_map(cmap, sampled[0][:-1], sampled[1][:-1], sampled[2][:-1], 0.4, 0.8)


@pytest.fixture(scope="module")
def run(pcc, tmp_path_factory):
    from pcc_amd import synthetic as syn
    from pcc_amd.harness import evaluate_view_dependent
    model = syn.make_model(seed=0, device=DEV)
    model.update()
    pts = syn.sphere_shell(**syn.CONFIG1)
    data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
    kw = dict(view="front", H=H, W=W, gradient=(2, 4.0, 28.0), roi=(0, 16))
    plain = evaluate_view_dependent("exp", model, data, Q_A, Q_G, DEV, str(tmp_path_factory.mktemp("plain")), **kw)
    none = evaluate_view_dependent("exp", model, data, Q_A, Q_G, DEV, str(tmp_path_factory.mktemp("none")), screen=None, **kw)
    details = {}
    rows = evaluate_view_dependent("exp", model, data, Q_A, Q_G, DEV, str(tmp_path_factory.mktemp("screen")), details=details,
                                   screen={"box": BOX}, **kw)
    return {"rows": rows, "plain": plain, "none": none, "details": details, "model": model, "data": data, "pts": pts}


def test_screen_none_is_todays_dict(run):
    assert list(run["plain"]) == list(run["none"]) == ["uniform", "view", "roi"]
    for key, row in run["plain"].items():
        assert set(row) == TODAY and run["none"][key] == row, key


def test_rows_with_a_box(run):
    rows, plain = run["rows"], run["plain"]
    assert list(rows) == ["uniform", "view", "roi", "screen"]
    for key in plain:
        assert set(rows[key]) == TODAY | {"psnr_roi", "ssim_roi"}
        assert {k: rows[key][k] for k in TODAY} == plain[key], key
    row = rows["screen"]
    assert set(row) == TODAY | {"psnr_roi", "ssim_roi"} and row["key"] == "screen" and row["q_a"] == Q_A and row["q_g"] == Q_G
    assert math.isfinite(row["bpp"]) and row["bpp"] > 0 and math.isfinite(row["psnr"]) and -1.0 <= row["ssim"] <= 1.0


def test_the_coded_map_is_the_reference(run):
    total, count, peak, score = run["details"]["screen"]
    xyz = run["pts"][:, :3].astype(np.int64)
    want = sr.sample_views(xyz, [FRONT], [sr.box_image(H, W, BOX)], H, W, tolerance=2)
    assert sr.tallies(want[1]) == (2012, 2892)
    for got, w in zip((total, count, peak), want):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), w)
    want_score = sr.image_score(*want)
    assert (int((want_score == 1).sum()), int((want_score == 0).sum())) == (740, 4164)
    assert score.dtype == torch.float64 and score.cpu().numpy().tobytes() == want_score.tobytes()


def test_region_metrics_match_the_reference(run):
    front, up = FRONT
    xyz, _ = vref.canonical(run["pts"])
    frame = vref.frame_of(xyz, front, up, H, W)
    want_ref = vref.render_cloud(run["pts"], front, up, H, W, frame=frame)
    assert np.array_equal(run["details"]["source"][1].cpu().numpy(), want_ref)
    mask = sr.box_image(H, W, BOX) > 0
    for key, row in run["rows"].items():
        rec, img = run["details"]["screen_row" if key == "screen" else key]
        want_img = vref.render_cloud(rec.cpu().numpy(), front, up, H, W, frame=frame)
        assert np.array_equal(img.cpu().numpy(), want_img), key
        m = sr.masked_metrics(want_ref, want_img, mask)
        print("screen harness %-8s bpp %.4f  psnr %.6f  psnr_roi %.6f (ref %.6f)  ssim_roi %.9f (ref %.9f)"
              % (key, row["bpp"], row["psnr"], row["psnr_roi"], m["psnr"], row["ssim_roi"], m["ssim"]))
        assert math.isfinite(m["psnr"]) and math.isfinite(m["ssim"])
        assert abs(row["psnr_roi"] - m["psnr"]) <= 1e-9 and abs(row["ssim_roi"] - m["ssim"]) <= 1e-9, key


def test_camera_gaze_image_and_anchor_rows(run, tmp_path):
    """the other two ways to give the image, through a camera, with anchor rows: every row carries the region columns, and they
    are the masked metrics of the row's own images"""
    from pcc_amd import q_map, render
    from pcc_amd.harness import evaluate_view_dependent
    camera = render.Camera((15.5, 15.5, 120.0), look_at=(15.5, 15.5, 15.5), fov_y=25, H=96, W=80)
    cam = tuple(camera.quantised())
    gaze = (48, 40, 8, 16)
    details = {}
    rows = evaluate_view_dependent("exp3", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), gradient=(2, 4.0, 28.0), roi=(0, 16),
                                   camera=camera, details=details, anchor={"match": False, "qstep": 8.0 / 255.0},
                                   screen={"gaze": gaze, "tolerance": None, "reduce": "mean", "floor": 0.25})
    assert list(rows) == ["uniform", "view", "roi", "screen", "anchor_uniform", "anchor_view", "anchor_roi", "anchor_screen"]
    image = sr.gaze_image(96, 80, gaze[:2], gaze[2], gaze[3])
    xyz = run["pts"][:, :3].astype(np.int64)
    want = sr.sample_cameras(xyz, [cam], [image], tolerance=None)
    assert min(sr.tallies(want[1])) > 0
    for got, w in zip(details["screen"][:3], want):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), w)
    assert details["screen"][3].cpu().numpy().tobytes() == sr.image_score(*want, reduce="mean", floor=0.25).tobytes()
    ref_img = details["source"][1].cpu().numpy()
    for key, row in rows.items():
        m = sr.masked_metrics(ref_img, details["screen_row" if key == "screen" else key][1].cpu().numpy(), image > 0)
        assert abs(row["psnr_roi"] - m["psnr"]) <= 1e-9 and abs(row["ssim_roi"] - m["ssim"]) <= 1e-9, key
    # the same image given as an array is the same map
    details2 = {}
    evaluate_view_dependent("exp4", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), camera=camera, details=details2,
                            screen={"image": q_map.gaze_image(96, 80, gaze[:2], gaze[2], gaze[3]), "tolerance": None, "reduce": "mean",
                                    "floor": 0.25})
    assert all(torch.equal(a, b) for a, b in zip(details["screen"], details2["screen"]))


def test_refusals(run, tmp_path):
    from pcc_amd.harness import evaluate_view_dependent
    for screen in ({}, {"box": BOX, "gaze": (1, 2, 3, 4)}, {"box": BOX, "falloff": 3}, {"image": np.zeros((W, H), dtype=np.uint8)},
                   {"image": np.zeros((H, W, 3), dtype=np.uint8)}):
        with pytest.raises(ValueError):
            evaluate_view_dependent("exp5", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), view="front", H=H, W=W, screen=screen)
