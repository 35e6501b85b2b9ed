"""render.view_metrics (csrc/render.hip, pcc_image_compare) on the GPU against the float64 numpy restatement
(tests/_view_reference.py).

Tolerance.  The largest window term carries about 60 float64 operations on values <= 1: about 60 x 1.1e-16 = 7e-15 absolute.
It is divided by a denominator of at least C2 = 9e-4: about 7e-12 on a value of the SSIM map, and no more on a mean of
them.  ``ssim`` is held to 1e-9 absolute (that bound with two orders of margin) and ``psnr`` to 1e-9 dB: the summed squared
error differs between two summation orders by a few 1e-16 relative, i.e. 1e-15 dB.  The per-channel mse are held to 1e-12
relative (tree and pairwise sums of <= 9,000 terms: ~ log2(n) x 1.1e-16).
"""
import math

import numpy as np
import pytest
import torch

import _view_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SSIM_TOL, PSNR_TOL, MSE_RTOL = 1e-9, 1e-9, 1e-12
TILE = 32                                                   # pixels a workgroup owns per side (pcc_image_compare_tile)
SIZES = [(7, 7), (7, 40), (40, 7), (8, 9), (64, 48), (130, 67)]
# one below, at and one above tile + 6 in each dimension: the last window of a tile's apron, the first pixels of the next tile
SIZES += [(h, w) for h in (TILE + 5, TILE + 6, TILE + 7) for w in (TILE + 5, TILE + 6, TILE + 7)]
WORST = {"ssim": 0.0, "psnr": 0.0}


def pairs(H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    noisy = np.clip(a.astype(np.int64) + rng.integers(-12, 13, size=a.shape), 0, 255).astype(np.uint8)
    # render-like: mostly white, a blob of smooth colour, the test image slightly shifted and dimmed
    yy, xx = np.mgrid[0:H, 0:W]
    blob = ((yy - H / 2) ** 2 / (H / 3) ** 2 + (xx - W / 2) ** 2 / (W / 3) ** 2) < 1
    r1 = np.full((H, W, 3), 255, dtype=np.uint8)
    r1[blob] = np.stack([(40 + 5 * yy) % 256, (200 - 3 * xx) % 256, (90 + yy + xx) % 256], axis=2)[blob].astype(np.uint8)
    r2 = np.roll(r1, 1, axis=1)
    r2[blob] = (r2[blob].astype(np.int64) * 15 // 16).astype(np.uint8)
    return {"random": (a, noisy), "render": (r1, r2), "black_white": (np.zeros_like(a), np.full_like(a, 255)),
            "white_black": (np.full_like(a, 255), np.zeros_like(a))}


def gpu(a, b, **kw):
    from pcc_amd import render
    return render.view_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), **kw)


def test_tile_constant(pcc):
    assert pcc.lib().pcc_image_compare_tile() == TILE


@pytest.mark.parametrize("H,W", SIZES)
def test_metrics_match_the_reference(pcc, H, W):
    for name, (a, b) in pairs(H, W, H * 1000 + W).items():
        want, got = ref.view_metrics(a, b), gpu(a, b)
        d_ssim, d_psnr = abs(got["ssim"] - want["ssim"]), abs(got["psnr"] - want["psnr"])
        WORST["ssim"], WORST["psnr"] = max(WORST["ssim"], d_ssim), max(WORST["psnr"], d_psnr)
        print("view_metrics %dx%d %-11s ssim %.15f |d| %.3e   psnr %.12f |d| %.3e   worst so far %.3e / %.3e"
              % (H, W, name, got["ssim"], d_ssim, got["psnr"], d_psnr, WORST["ssim"], WORST["psnr"]))
        assert d_ssim <= SSIM_TOL, (name, got, want)
        assert d_psnr <= PSNR_TOL, (name, got, want)
        for k in ("y_mse", "u_mse", "v_mse"):
            assert got[k] == pytest.approx(want[k], rel=MSE_RTOL, abs=0.0), (name, k)
        # equal images: exactly 1 and inf
        same = gpu(a, a.copy())
        assert same["ssim"] == 1.0 and same["psnr"] == math.inf and same["y_mse"] == same["u_mse"] == same["v_mse"] == 0.0


def test_two_calls_are_bitwise_equal(pcc):
    from pcc_amd import render
    a, b = pairs(130, 67, 1)["random"]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    first = render.image_compare(ta, tb)
    assert len(first) == 8 and all(math.isfinite(v) for v in first)
    for _ in range(3):
        assert [v.hex() for v in render.image_compare(ta, tb)] == [v.hex() for v in first]
    ya = ref.yuv(a)
    assert first[6] == ya.min() and first[7] == ya.max()                     # elementwise values are the reference's, bit for bit


def test_data_range_rule_on_a_saturated_colour(pcc):
    """scikit-image's rule for float images: data range 1 while the reference image's smallest YUV value is >= 0, else the
    range of [-1, 1], 2.  Shades of magenta on black have Y, U, V >= 0; one pure blue pixel has V = -0.10001026."""
    from pcc_amd import render
    rng = np.random.default_rng(2)
    k = rng.integers(0, 256, size=(20, 24), dtype=np.uint8)
    a = np.stack([k, np.zeros_like(k), k], axis=2)
    k2 = np.clip(k.astype(np.int64) + rng.integers(-9, 10, size=k.shape), 0, 255).astype(np.uint8)
    b = np.stack([k2, np.zeros_like(k), k2], axis=2)
    assert render.image_compare(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))[6] >= 0.0
    assert gpu(a, b)["psnr"] == gpu(a, b, data_range=1.0)["psnr"] and ref.view_metrics(a, b)["data_range"] == 1.0
    a[3, 4] = (0, 0, 255)
    assert render.image_compare(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))[6] == -0.10001026
    auto, two, one = gpu(a, b), gpu(a, b, data_range=2.0), gpu(a, b, data_range=1.0)
    assert auto["psnr"] == two["psnr"] and auto["psnr"] == pytest.approx(one["psnr"] + 10 * math.log10(4.0), abs=1e-12)
    assert auto["ssim"] == one["ssim"]                                        # SSIM's data range is fixed at 1
    want = ref.view_metrics(a, b)
    assert want["data_range"] == 2.0 and abs(auto["psnr"] - want["psnr"]) <= PSNR_TOL


def test_refusals_reach_python(pcc):
    from pcc_amd import render
    from pcc_amd._lib import PccError
    small = torch.zeros((6, 9, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(PccError):
        render.view_metrics(small, small)
    ok = torch.zeros((9, 9, 3), dtype=torch.uint8, device=DEV)
    for bad in (ok.float(), ok[..., :2], ok[:8]):
        with pytest.raises(ValueError):
            render.view_metrics(ok, bad)
    with pytest.raises(ValueError):
        render.view_metrics(ok.cpu(), ok.cpu())
