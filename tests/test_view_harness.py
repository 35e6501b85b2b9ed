"""harness.evaluate_view_dependent on the 32^3-class synthetic frame with the seeded model (as tests/test_frontend.py): the
three rows of the view-dependent experiment, their images against the painter's-loop renderer on the decoded clouds, and
their metrics against the numpy restatement (tolerances: tests/test_view_metrics.py).  The seeded weights have no
rate-distortion meaning, so nothing is asserted about the order of rates or qualities between the rows."""
import math
import os

import numpy as np
import pytest
import torch

import _view_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 160, 96
Q_A, Q_G = 0.8, 0.4


@pytest.fixture(scope="module")
def run(pcc, tmp_path_factory):
    from pcc_amd import synthetic as syn
    from pcc_amd.harness import evaluate_view_dependent
    model = syn.make_model(seed=0, device=DEV)
    model.update()
    pts = syn.sphere_shell(**syn.CONFIG1)
    data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
    base = str(tmp_path_factory.mktemp("view_dep"))
    details = {}
    rows = evaluate_view_dependent("exp", model, data, Q_A, Q_G, DEV, base, view="front", H=H, W=W, gradient=(2, 4.0, 28.0),
                                   roi=(0, 16), save_images=True, details=details)
    return {"rows": rows, "details": details, "base": base, "model": model, "data": data, "pts": pts}


def test_three_keyed_rows(run):
    rows = run["rows"]
    assert list(rows) == ["uniform", "view", "roi"]
    for key, row in rows.items():
        assert set(row) == {"bpp", "q_a", "q_g", "key", "psnr", "ssim"}
        assert row["key"] == key and row["q_a"] == Q_A and row["q_g"] == Q_G
        assert math.isfinite(row["bpp"]) and row["bpp"] > 0 and math.isfinite(row["psnr"]) and math.isfinite(row["ssim"])
        assert -1.0 <= row["ssim"] <= 1.0


def test_uniform_row_rate_is_evaluate_frames(run, tmp_path):
    from pcc_amd.harness import evaluate_frame
    row = evaluate_frame("exp", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), resolution=31)
    assert run["rows"]["uniform"]["bpp"] == row["bpp"]


def test_source_against_itself(run):
    from pcc_amd import render
    src, ref_img = run["details"]["source"]
    assert np.array_equal(src.cpu().numpy(), run["pts"])
    m = render.view_metrics(ref_img, ref_img.clone())
    assert m["ssim"] == 1.0 and m["psnr"] == math.inf


def test_images_and_metrics_match_the_reference(run):
    from pcc_amd import render
    front, up = render.VIEWS["front"]
    xyz, _ = ref.canonical(run["pts"])
    frame = ref.frame_of(xyz, front, up, H, W)
    assert frame[4] == 3                                       # 31 voxels across: scale 3 in 96 x 160
    want_ref = ref.render_cloud(run["pts"], front, up, H, W, frame=frame)
    assert np.array_equal(run["details"]["source"][1].cpu().numpy(), want_ref)
    assert (want_ref != 255).any()
    for key in ("uniform", "view", "roi"):
        rec, img = run["details"][key]
        want = ref.render_cloud(rec.cpu().numpy(), front, up, H, W, frame=frame)       # in the SOURCE's frame
        assert np.array_equal(img.cpu().numpy(), want), key
        m = ref.view_metrics(want_ref, want)
        row = run["rows"][key]
        print("view harness %-8s bpp %.4f psnr %.6f (ref %.6f) ssim %.9f (ref %.9f)" % (key, row["bpp"], row["psnr"], m["psnr"],
                                                                                     row["ssim"], m["ssim"]))
        assert abs(row["ssim"] - m["ssim"]) <= 1e-9 and abs(row["psnr"] - m["psnr"]) <= 1e-9


def test_saved_pngs_decode_to_the_rendered_bytes(run):
    img_dir = os.path.join(run["base"], "exp", "renders_view")
    names = {"source": "ref_front.png"}
    names.update({k: "%s_a%s_g%s_front.png" % (k, Q_A, Q_G) for k in ("uniform", "view", "roi")})
    assert sorted(os.listdir(img_dir)) == sorted(names.values())
    for key, name in names.items():
        with open(os.path.join(img_dir, name), "rb") as f:
            assert np.array_equal(ref.decode_png(f.read()), run["details"][key][1].cpu().numpy()), name


def test_maps_default_to_the_frames_extent_and_views_by_pair(run, tmp_path):
    """gradient / roi left to the harness, a (front, up) pair instead of a preset, no images written"""
    from pcc_amd.harness import evaluate_view_dependent
    rows = evaluate_view_dependent("exp3", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), view=((-1, 0, 0), (0, 1, 0)), H=64, W=48)
    assert list(rows) == ["uniform", "view", "roi"] and all(math.isfinite(r["psnr"]) for r in rows.values())
    assert rows["uniform"]["bpp"] == run["rows"]["uniform"]["bpp"]
    assert not os.path.exists(os.path.join(str(tmp_path), "exp3", "renders_view"))
    with pytest.raises(ValueError):
        evaluate_view_dependent("exp3", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), view="top")
