"""The public interface of the voxel-grid PCQM stand-in: pcqm.pcqm_voxel, PointCloudMetric.compute_pcqm and the ``pcqm`` rows of
harness.evaluate_frame, on the clouds of tests/_pcqm_reference.py."""
import math

import numpy as np
import pytest
import torch

import _pcqm_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = {"pcqm_voxel"} | {"pcqm_f%d" % i for i in range(1, 9)}


def test_compute_pcqm_equals_pcqm_voxel_and_reuses_the_associations(pcc, monkeypatch):
    from pcc_amd import metrics, pcqm_voxel, sparse
    R, D = ref.shell_pair()
    r, d = torch.from_numpy(R).to(DEV), torch.from_numpy(D).to(DEV)
    direct = pcqm_voxel(r, d, return_features=True)
    metric = metrics.PointCloudMetric(r, d, resolution=31, device=DEV)

    def refuse(*a, **k):
        raise AssertionError("compute_pcqm searched or hashed again")
    monkeypatch.setattr(metrics, "nearest_neighbours", refuse)
    monkeypatch.setattr(sparse.CoordMap, "__init__", refuse)
    got = metric.compute_pcqm(return_features=True)
    monkeypatch.undo()
    assert set(got) == set(direct) == KEYS | {"radius", "neighbourhood", "features"}
    assert (got["radius"], got["neighbourhood"]) == (1, 2)
    for k in KEYS:
        assert got[k] == direct[k] and math.isfinite(got[k]), k
    assert torch.equal(got["features"], direct["features"])
    assert got["pcqm_voxel"] > 0
    # the score is the weighted sum of the pooled features, and follows the restatement
    want, pooled, _ = ref.score(R, D, 1, 2)
    assert abs(got["pcqm_voxel"] - want) <= 1e-12 and all(abs(got["pcqm_f%d" % (i + 1)] - pooled[i]) <= 1e-12 for i in range(8))
    plain = metric.compute_pcqm()
    assert set(plain) == KEYS | {"radius", "neighbourhood"} and plain["pcqm_voxel"] == got["pcqm_voxel"]
    with pytest.raises(TypeError):
        metric.compute_pcqm(device=DEV)


def test_parameters_reach_the_kernel(pcc):
    from pcc_amd import pcqm_voxel
    R, D = ref.shell_pair()
    r, d = torch.from_numpy(R).to(DEV), torch.from_numpy(D).to(DEV)
    only_f1 = pcqm_voxel(r, d, radius=2, neighbourhood=3, weights=(1, 0, 0, 0, 0, 0, 0, 0), k_L=5.0)
    assert (only_f1["radius"], only_f1["neighbourhood"]) == (2, 3) and only_f1["pcqm_voxel"] == only_f1["pcqm_f1"]
    want, pooled, _ = ref.score(R, D, 2, 3, weights=(1, 0, 0, 0, 0, 0, 0, 0), k_L=5.0)
    assert abs(only_f1["pcqm_voxel"] - want) <= 1e-12
    assert only_f1["pcqm_f1"] < pcqm_voxel(r, d, radius=2, neighbourhood=3)["pcqm_f1"]      # a larger k_L damps the contrast
    with pytest.raises(ValueError):
        pcqm_voxel(r, d, weights=(1, 2, 3))
    with pytest.raises(ValueError):
        pcqm_voxel(r + 0.5, d)


def test_default_radii_on_the_gpu(pcc):
    from pcc_amd import pcqm_voxel
    R, D = ref.shell_pair()
    out = pcqm_voxel(R, D)                                                  # arrays are accepted like PointCloudMetric's
    assert (out["radius"], out["neighbourhood"]) == (1, 2)
    far = np.concatenate([R, [[1000.0, 10.0, 10.0, 0.5, 0.5, 0.5]]])         # a cloud with a 1,000-voxel side
    out = pcqm_voxel(far, far)
    assert (out["radius"], out["neighbourhood"]) == (4, 8) and out["pcqm_voxel"] == 0.0


def test_more_colour_noise_scores_worse(pcc):
    """the same geometry with +-4, +-12 and +-36 levels of colour noise; tests/test_pcqm_reference.py holds the restatement to
    the same order"""
    from pcc_amd import pcqm_voxel
    R = ref.shell_pair(0)[0]
    scores = [pcqm_voxel(R, ref.shell_pair(noise)[1])["pcqm_voxel"] for noise in (4, 12, 36)]
    print("pcqm_voxel at +-4 / 12 / 36 levels:", scores)
    assert 0.0 < scores[0] < scores[1] < scores[2]


def test_evaluate_frame_rows_gain_the_nine_keys(pcc, tmp_path):
    """the seeded model on the config-1 frame, as tests/test_d2_metric.py"""
    from pcc_amd import pcqm_voxel, synthetic as syn
    from pcc_amd.harness import compress_model_ours, evaluate_frame
    model = syn.make_model(seed=0, device=DEV)
    model.update()
    pts = syn.sphere_shell(**syn.CONFIG1)
    data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
    plain = evaluate_frame("exp", model, data, 0.8, 0.4, DEV, str(tmp_path), resolution=31)
    row = evaluate_frame("exp", model, data, 0.8, 0.4, DEV, str(tmp_path), resolution=31, pcqm=True)
    assert set(row) == set(plain) | KEYS
    for k in plain:
        if not k.startswith("t_"):
            assert row[k] == plain[k], k
    src, rec, _, _, _ = compress_model_ours("exp", model, data, 0.8, 0.4, DEV, str(tmp_path))
    direct = pcqm_voxel(src, rec)
    assert row["pcqm_voxel"] == direct["pcqm_voxel"] and all(row[k] == direct[k] for k in KEYS)
    assert math.isfinite(row["pcqm_voxel"]) and row["pcqm_voxel"] > 0
