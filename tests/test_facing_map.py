"""q_map.facing_map against the numpy restatement (tests/_normals_reference.py: reference_facing) and the fourth row of
harness.evaluate_view_dependent.  The map is float32: 1e-6 absolute covers its rounding (half an ulp of 1.0 is 6e-8) and the
float64 round-off in front of it."""
import math

import numpy as np
import pytest
import torch

import _normals_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q_A, Q_G = 0.8, 0.4


@pytest.fixture(scope="module")
def shell(pcc):
    from pcc_amd import CoordMap, estimate_normals
    pts = ref.shell(32, 11, 0.875)
    coords = torch.from_numpy(np.concatenate([np.zeros((len(pts), 1), np.int64), pts], axis=1).astype(np.int32)).to(DEV)
    cmap = CoordMap(coords, 1, nbatch=1)
    normals, _ = estimate_normals(coords, radius=3, coord_map=cmap)
    return pts, cmap, normals


@pytest.mark.parametrize("kw", [dict(camera=(40.0, 15.5, -7.0)), dict(direction=(0.0, 0.0, 1.0)), dict(direction=(1.0, -2.0, 0.5), floor=0.3),
                                dict(camera=(15.5, 15.5, 15.5), floor=0.5)])
def test_facing_map_equals_the_reference(pcc, shell, kw):
    from pcc_amd import q_map
    pts, cmap, normals = shell
    got = q_map.facing_map(cmap, normals, Q_G, Q_A, **kw)
    assert got.F.dtype == torch.float32 and got.F.shape == (len(pts), 2) and got.map is cmap
    want = ref.reference_facing(pts, normals.cpu().numpy(), Q_G, Q_A, **kw)
    err = np.abs(got.F.cpu().numpy() - want).max()
    print("facing map", kw, "max error %.3g" % err, "score range %.3f .. %.3f" % (want[:, 1].min() / Q_A, want[:, 1].max() / Q_A))
    assert err <= 1e-6


def test_floor_and_invalid_normals(pcc, shell):
    from pcc_amd import q_map
    pts, cmap, normals = shell
    floor = 0.25
    f = q_map.facing_map(cmap, normals, Q_G, Q_A, direction=(0, 0, 1), floor=floor).F.cpu().numpy()
    assert f[:, 0].min() >= Q_G * floor - 1e-6 and f[:, 0].max() <= Q_G + 1e-6
    assert f[:, 0].min() < Q_G * (floor + 0.05)                     # the equator looks sideways: close to the floor
    some = normals.clone()
    some[::7] = 0.0
    f = q_map.facing_map(cmap, some, Q_G, Q_A, direction=(0, 0, 1), floor=floor).F.cpu().numpy()
    assert np.array_equal(f[::7], np.tile(np.float32([Q_G, Q_A]), (len(f[::7]), 1)))
    want = ref.reference_facing(pts, some.cpu().numpy(), Q_G, Q_A, direction=(0, 0, 1), floor=floor)
    assert np.abs(f - want).max() <= 1e-6
    with pytest.raises(ValueError):
        q_map.facing_map(cmap, normals, Q_G, Q_A)
    with pytest.raises(ValueError):
        q_map.facing_map(cmap, normals, Q_G, Q_A, camera=(0, 0, 0), direction=(0, 0, 1))


def test_view_dependent_harness_gains_a_fourth_row(pcc, tmp_path):
    """the seeded model on the config-1 frame, as tests/test_view_harness.py"""
    from pcc_amd import synthetic as syn
    from pcc_amd.harness import evaluate_view_dependent
    model = syn.make_model(seed=0, device=DEV)
    model.update()
    pts = syn.sphere_shell(**syn.CONFIG1)
    data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
    args = ("exp", model, data, Q_A, Q_G, DEV, str(tmp_path))
    kw = dict(view="front", H=160, W=96, gradient=(2, 4.0, 28.0), roi=(0, 16))
    three = evaluate_view_dependent(*args, **kw)
    details = {}
    four = evaluate_view_dependent(*args, facing={"radius": 3, "direction": (0, 0, 1), "floor": 0.2}, details=details, **kw)
    assert list(three) == ["uniform", "view", "roi"] and list(four) == ["uniform", "view", "roi", "facing"]
    for key in three:
        assert four[key] == three[key]
    row = four["facing"]
    assert set(row) == set(three["uniform"]) and row["key"] == "facing" and row["q_a"] == Q_A and row["q_g"] == Q_G
    assert math.isfinite(row["bpp"]) and row["bpp"] > 0 and math.isfinite(row["psnr"]) and -1.0 <= row["ssim"] <= 1.0
    assert set(details) == {"source", "uniform", "view", "roi", "facing"}
    by_camera = evaluate_view_dependent(*args, facing={"camera": (15.5, 15.5, 200.0)}, **kw)
    assert list(by_camera) == list(four) and math.isfinite(by_camera["facing"]["psnr"])
