"""harness.evaluate_view_dependent with ``visibility``: the fixture of tests/test_view_harness.py (seeded model, the CONFIG1
shell, 160 x 96, front view) with the fourth row "visible".  The map that was coded is held to the numpy restatement
(tests/_visibility_reference.py), the row's image to the painter's-loop renderer on the decoded cloud and its metrics to the
numpy metrics (the bound of tests/test_view_harness.py).  The seeded weights have no rate-distortion meaning, so nothing is
asserted about the order of rates or qualities between the rows."""
import math
import os

import numpy as np
import pytest
import torch

import _view_reference as vref
import _visibility_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 160, 96
Q_A, Q_G = 0.8, 0.4
FRONT = ((0, 0, 1), (0, 1, 0))


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
    base = str(tmp_path_factory.mktemp("visible"))
    details = {}
    rows = evaluate_view_dependent("exp", model, data, Q_A, Q_G, DEV, base, save_images=True, details=details,
                                   visibility={"views": ["front"]}, **kw)
    return {"rows": rows, "plain": plain, "details": details, "base": base, "model": model, "data": data, "pts": pts}


def test_fourth_row(run):
    rows, plain = run["rows"], run["plain"]
    assert list(plain) == ["uniform", "view", "roi"]
    assert list(rows) == ["uniform", "view", "roi", "visible"]
    for key in plain:
        assert rows[key] == plain[key], key
    row = rows["visible"]
    assert set(row) == set(rows["uniform"]) == {"bpp", "q_a", "q_g", "key", "psnr", "ssim"}
    assert row["key"] == "visible" and row["q_a"] == Q_A and row["q_g"] == Q_G
    assert math.isfinite(row["bpp"]) and row["bpp"] > 0 and math.isfinite(row["psnr"]) and math.isfinite(row["ssim"])
    assert -1.0 <= row["ssim"] <= 1.0


def test_the_coded_map_is_the_reference(run):
    behind, score = run["details"]["visibility"]
    xyz = run["pts"][:, :3].astype(np.int64)
    want_b, _ = ref.visibility(xyz, [FRONT], H, W)
    assert behind.dtype == torch.int32 and np.array_equal(behind.cpu().numpy(), want_b)
    assert (int((want_b == 0).sum()), int((want_b <= 2).sum())) == (788, 2012)
    assert score.dtype == torch.float64 and score.cpu().numpy().tobytes() == ref.score(want_b, 2, 8, 0.0).tobytes()


def test_image_and_metrics_match_the_reference(run):
    front, up = FRONT
    xyz, _ = vref.canonical(run["pts"])
    frame = vref.frame_of(xyz, front, up, H, W)
    want_ref = vref.render_cloud(run["pts"], front, up, H, W, frame=frame)
    assert np.array_equal(run["details"]["source"][1].cpu().numpy(), want_ref)
    rec, img = run["details"]["visible"]
    want = vref.render_cloud(rec.cpu().numpy(), front, up, H, W, frame=frame)            # in the SOURCE's frame
    assert np.array_equal(img.cpu().numpy(), want)
    m = vref.view_metrics(want_ref, want)
    row = run["rows"]["visible"]
    print("view harness visible  bpp %.4f (uniform %.4f) psnr %.6f (ref %.6f) ssim %.9f (ref %.9f)"
          % (row["bpp"], run["rows"]["uniform"]["bpp"], row["psnr"], m["psnr"], row["ssim"], m["ssim"]))
    assert abs(row["ssim"] - m["ssim"]) <= 1e-9 and abs(row["psnr"] - m["psnr"]) <= 1e-9


def test_saved_png_of_the_row(run):
    name = "visible_a%s_g%s_front.png" % (Q_A, Q_G)
    img_dir = os.path.join(run["base"], "exp", "renders_view")
    assert name in os.listdir(img_dir) and len(os.listdir(img_dir)) == 5
    with open(os.path.join(img_dir, name), "rb") as f:
        assert np.array_equal(vref.decode_png(f.read()), run["details"]["visible"][1].cpu().numpy())


def test_options_and_refusals(run, tmp_path):
    """views default to the judged view; tolerance, falloff and floor reach the score; an unknown key or an empty list of views
    is refused before anything is coded"""
    from pcc_amd.harness import evaluate_view_dependent
    details = {}
    evaluate_view_dependent("exp2", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), view="front", H=H, W=W, details=details,
                            visibility={"tolerance": 0, "falloff": 0, "floor": 0.25})
    behind, score = details["visibility"]
    assert torch.equal(behind, run["details"]["visibility"][0])
    assert score.cpu().numpy().tobytes() == ref.score(behind.cpu().numpy(), 0, 0, 0.25).tobytes()
    assert sorted(set(score.tolist())) == [0.25, 1.0]
    with pytest.raises(ValueError):
        evaluate_view_dependent("exp2", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), visibility={"view": ["front"]})
    with pytest.raises(ValueError):
        evaluate_view_dependent("exp2", run["model"], run["data"], Q_A, Q_G, DEV, str(tmp_path), visibility={"views": []})
