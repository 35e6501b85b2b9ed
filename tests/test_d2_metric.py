"""PointCloudMetric.compute_d2 (point-to-plane PSNR) against the numpy restatement (tests/_normals_reference.py: reference_d2).

With the GPU's own normals the two differ only in the order of float64 sums (1e-9 relative); with numpy.linalg.eigh's normals
also by the normals' agreement (|n x n_ref| <= 1e-9 on this shell, tests/test_normals.py), far inside 1e-6 relative."""
import math

import numpy as np
import pytest
import torch

import _normals_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = 31
KEYS = ("AB_d2_mse", "AB_d2_psnr", "BA_d2_mse", "BA_d2_psnr", "sym_d2_mse", "sym_d2_psnr")


@pytest.fixture(scope="module")
def source(pcc):
    from pcc_amd import estimate_normals, synthetic as syn
    src = syn.sphere_shell(grid=32, radius=11, half_width=0.875)
    assert src.shape == (2816, 6)
    xyz = src[:, :3].astype(np.int64)
    count, moments = ref.ball_moments(xyz, np.zeros(len(xyz), np.int64), 3)
    ref_normals, _, _ = ref.reference_normals(count, moments)
    gpu_normals = estimate_normals(torch.from_numpy(src).to(DEV), radius=3)[0].cpu().numpy()
    return src, ref_normals, gpu_normals


def reconstruction(src, which):
    from pcc_amd import synthetic as syn
    if which == "same":
        return src.copy()
    if which == "moved":                                           # a seeded tenth of the points one voxel along x
        rec = src.copy()
        rows = np.random.default_rng(5).choice(len(rec), len(rec) // 10, replace=False)
        rec[rows, 0] += 1.0
        return rec
    return syn.sphere_shell(grid=32, radius=11.6, half_width=0.875)


def close(a, b, rel):
    if math.isinf(a) or math.isinf(b) or a == 0 or b == 0:
        return a == b
    return abs(a - b) <= rel * abs(b)


@pytest.mark.parametrize("which", ["same", "moved", "bigger"])
def test_d2_against_the_reference(pcc, source, which):
    from pcc_amd.metrics import PointCloudMetric
    src, ref_normals, gpu_normals = source
    rec = reconstruction(src, which)
    metric = PointCloudMetric(src, rec, resolution=RES, device=DEV)
    before, _ = metric.compute_pointcloud_metrics(drop_duplicates=True)
    d2 = metric.compute_d2(radius=3)
    after, _ = metric.compute_pointcloud_metrics(drop_duplicates=True)
    assert before == after and not any("d2" in k for k in after)
    assert tuple(sorted(d2)) == tuple(sorted(KEYS))
    rec_unique = ref.drop_duplicates(rec)
    if which == "moved":
        assert len(rec_unique) < len(rec)                          # some moved points land on occupied voxels
    own = ref.reference_d2(src, rec_unique, gpu_normals, RES)
    other = ref.reference_d2(src, rec_unique, ref_normals, RES)
    for k in KEYS:
        print("%-7s %-12s %.12g  (reference, GPU normals %.12g; reference normals %.12g)  D1 AB/BA mse %.6g / %.6g" % (
            which, k, d2[k], own[k], other[k], before["AB_mse"], before["BA_mse"]))
    for k in KEYS:
        assert close(d2[k], own[k], 1e-9), k
        assert close(d2[k], other[k], 1e-6), k
    assert d2["AB_d2_mse"] <= before["AB_mse"] and d2["BA_d2_mse"] <= before["BA_mse"]
    assert d2["sym_d2_mse"] == max(d2["AB_d2_mse"], d2["BA_d2_mse"]) and d2["sym_d2_psnr"] == min(d2["AB_d2_psnr"], d2["BA_d2_psnr"])
    if which == "same":
        assert d2["sym_d2_mse"] == 0.0 and d2["sym_d2_psnr"] == math.inf and d2["AB_d2_psnr"] == math.inf
    else:
        assert d2["sym_d2_mse"] > 0.0
    if which == "bigger":                                          # a radial shift lies along the normals only in part
        assert d2["AB_d2_psnr"] > before["AB_psnr_mse"] and d2["BA_d2_psnr"] > before["BA_psnr_mse"]
        assert d2["sym_d2_psnr"] > before["sym_psnr_mse"]


def test_invalid_normals_count_their_full_distance(pcc):
    """a source of points on one line has no normals: D2 equals D1"""
    from pcc_amd.metrics import PointCloudMetric
    src = np.zeros((12, 6), np.float32)
    src[:, 0] = np.arange(12)
    rec = src.copy()
    rec[:, 1] += 2.0
    metric = PointCloudMetric(src, rec, resolution=RES, device=DEV)
    d1, _ = metric.compute_pointcloud_metrics(drop_duplicates=True)
    d2 = metric.compute_d2(radius=3)
    assert d2["AB_d2_mse"] == d1["AB_mse"] and d2["BA_d2_mse"] == d1["BA_mse"] and abs(d1["AB_mse"] - 4.0 / 3.0) <= 1e-12
    assert d2["AB_d2_psnr"] == d1["AB_psnr_mse"]


def test_evaluate_frame_row_gains_one_key(pcc, tmp_path):
    """the seeded model on the config-1 frame, as tests/test_view_harness.py"""
    from pcc_amd import synthetic as syn
    from pcc_amd.harness import evaluate_frame
    from pcc_amd.metrics import PointCloudMetric
    model = syn.make_model(seed=0, device=DEV)
    model.update()
    pts = syn.sphere_shell(**syn.CONFIG1)
    data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
    plain = evaluate_frame("exp", model, data, 0.8, 0.4, DEV, str(tmp_path), resolution=RES)
    assert set(plain) == {"q_g", "q_a", "bpp", "t_compress", "t_decompress", "n_source", "n_decoded", "sym_p2p_psnr", "sym_y_psnr",
                          "sym_u_psnr", "sym_v_psnr"}
    with_d2 = evaluate_frame("exp", model, data, 0.8, 0.4, DEV, str(tmp_path), resolution=RES, d2_radius=3)
    assert set(with_d2) == set(plain) | {"sym_d2_psnr"}
    for k in plain:
        if not k.startswith("t_"):
            assert with_d2[k] == plain[k], k
    assert math.isfinite(with_d2["sym_d2_psnr"]) and with_d2["sym_d2_psnr"] >= with_d2["sym_p2p_psnr"]
