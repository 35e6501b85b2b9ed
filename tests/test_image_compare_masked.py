"""render.view_metrics / image_compare with a mask (csrc/render.hip, pcc_image_compare_masked) on the GPU.

With an all-ones mask the six sums are BITWISE those of the unmasked entry: the same tile kernel adds the same terms in the same
order.  With a real mask the metrics are held to the float64 numpy restatement (tests/_sample_reference.masked_metrics, built on
tests/_view_reference.yuv / ssim_map) within the bound tests/test_view_metrics.py derives and uses: 1e-9 absolute for the SSIM,
1e-9 dB for the PSNR, 1e-12 relative for the per-channel errors.  Masking only removes terms from the sums that bound was
worked out for, so it holds unchanged.  An infinite PSNR (no error inside the mask) must be infinite on both sides."""
import math

import numpy as np
import pytest
import torch

import _sample_reference as sr
import _view_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SSIM_TOL, PSNR_TOL, MSE_RTOL = 1e-9, 1e-9, 1e-12
SIZES = [(7, 7), (8, 9), (32, 32), (37, 38), (39, 70), (64, 48), (96, 160), (130, 67)]      # multiples of the 32-pixel tile and not


def pair(H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-12, 13, size=a.shape), 0, 255).astype(np.uint8)
    return a, b


def masks(H, W, seed):
    rng = np.random.default_rng(seed)
    box = np.zeros((H, W), dtype=bool)
    box[H // 4:H // 4 + max(1, H // 2), W // 3:W // 3 + max(1, W // 2)] = True
    one = np.zeros((H, W), dtype=bool)
    one[H // 2, W // 2] = True
    border = np.zeros((H, W), dtype=bool)
    border[:3], border[-3:], border[:, :3], border[:, -3:] = True, True, True, True
    corner = np.zeros((H, W), dtype=bool)
    corner[H - 1, W - 1] = True
    return {"random": rng.integers(0, 2, size=(H, W)) == 1, "box": box, "one_pixel": one, "border": border, "last_pixel": corner}


def gpu(a, b, **kw):
    from pcc_amd import render
    return render.view_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), **kw)


def close(got, want, what):
    assert set(got) == {"psnr", "ssim", "y_mse", "u_mse", "v_mse"}
    for key in ("psnr", "ssim"):
        if math.isnan(want[key]) or math.isinf(want[key]):
            assert (math.isnan(got[key]) and math.isnan(want[key])) or got[key] == want[key], (what, key, got, want)
        else:
            print("masked metrics %-28s %-4s got %.15g want %.15g |d| %.3e" % (what, key, got[key], want[key], abs(got[key] - want[key])))
            assert abs(got[key] - want[key]) <= (SSIM_TOL if key == "ssim" else PSNR_TOL), (what, key, got, want)
    for key in ("y_mse", "u_mse", "v_mse"):
        if math.isnan(want[key]):
            assert math.isnan(got[key]), (what, key)
        else:
            assert abs(got[key] - want[key]) <= MSE_RTOL * abs(want[key]), (what, key, got, want)


@pytest.mark.parametrize("H,W", SIZES)
def test_all_ones_mask_is_bitwise_the_unmasked_sums(pcc, H, W):
    from pcc_amd import render
    a, b = (torch.from_numpy(x).to(DEV) for x in pair(H, W, H * 1000 + W))
    plain = render.image_compare(a, b)
    for ones in (np.ones((H, W), dtype=bool), np.full((H, W), 255, dtype=np.uint8), torch.full((H, W), 7, dtype=torch.int32, device=DEV)):
        masked = render.image_compare(a, b, mask=ones)
        assert len(masked) == 8
        assert np.asarray(masked, dtype=np.float64).tobytes() == np.asarray(plain, dtype=np.float64).tobytes()
    assert render.image_compare(a, b) == plain                                       # and the unmasked entry is reproducible
    assert render.view_metrics(a, b, mask=np.ones((H, W), dtype=bool)) == render.view_metrics(a, b)


@pytest.mark.parametrize("H,W", SIZES)
def test_masked_metrics_match_the_reference(pcc, H, W):
    a, b = pair(H, W, H * 1000 + W + 1)
    for name, mask in masks(H, W, H + W).items():
        want = sr.masked_metrics(a, b, mask)
        if name in ("border", "last_pixel"):
            assert mask.any() and math.isnan(want["ssim"]) and math.isfinite(want["psnr"])      # masked pixels, no masked window
        elif name == "one_pixel" or (H, W) != (7, 7):
            assert math.isfinite(want["ssim"]), name
        close(gpu(a, b, mask=mask), want, "%dx%d %s" % (H, W, name))
        close(gpu(a, b, mask=torch.from_numpy(mask).to(DEV), data_range=2.0), sr.masked_metrics(a, b, mask, data_range=2.0), "%dx%d %s range 2" % (H, W, name))


def test_no_error_inside_the_mask_is_an_infinite_psnr(pcc):
    a, b = pair(40, 50, 3)
    mask = np.zeros((40, 50), dtype=bool)
    mask[10:20, 5:30] = True
    b = np.where(mask[:, :, None], a, b)
    want = sr.masked_metrics(a, b, mask)
    assert want["psnr"] == math.inf and want["y_mse"] == 0.0
    close(gpu(a, b, mask=mask), want, "equal inside")
    assert math.isfinite(gpu(a, b, mask=~mask)["psnr"])


def test_empty_mask_is_nan(pcc):
    a, b = pair(33, 35, 5)
    got = gpu(a, b, mask=np.zeros((33, 35), dtype=bool))
    assert all(math.isnan(got[k]) for k in ("psnr", "ssim", "y_mse", "u_mse", "v_mse"))


def test_the_data_range_rule_reads_the_whole_reference(pcc):
    """a reference whose only negative U / V values lie OUTSIDE the mask still gets data range 2"""
    a = np.full((20, 24, 3), 128, dtype=np.uint8)                     # grey: U = V = 0 up to rounding
    a[0, 0] = (0, 255, 0)                                             # green: V < 0, outside the mask
    b = a.copy()
    b[10:14, 10:14] = 100
    mask = np.zeros((20, 24), dtype=bool)
    mask[8:16, 8:16] = True
    want = sr.masked_metrics(a, b, mask)
    assert ref.yuv(a).min() < -0.1 and ref.yuv(a)[mask].min() > -1e-6
    close(gpu(a, b, mask=mask), want, "data range")
    assert abs(gpu(a, b, mask=mask)["psnr"] - sr.masked_metrics(a, b, mask, data_range=2.0)["psnr"]) <= PSNR_TOL


def test_mask_none_is_todays_dict(pcc):
    a, b = pair(45, 71, 9)
    want = ref.view_metrics(a, b)
    got = gpu(a, b)
    assert got == gpu(a, b, mask=None) and set(got) == {"psnr", "ssim", "y_mse", "u_mse", "v_mse"}
    close(got, {k: want[k] for k in got}, "unmasked")


def test_refusals(pcc):
    from pcc_amd import _lib, render
    a, b = (torch.from_numpy(x).to(DEV) for x in pair(16, 18, 1))
    for mask in (np.ones((18, 16), dtype=bool), np.ones((16, 18, 1), dtype=bool), np.ones(16 * 18, dtype=bool)):
        with pytest.raises(ValueError):
            render.view_metrics(a, b, mask=mask)
    L = pcc.lib()
    nbytes = int(L.pcc_image_compare_scratch_bytes(16, 18))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((8,), -5.0, dtype=torch.float64, device=DEV)
    m = torch.ones((16, 18), dtype=torch.uint8, device=DEV)
    args = lambda **o: (o.get("ref", a.data_ptr()), b.data_ptr(), o.get("mask", m.data_ptr()), o.get("H", 16), o.get("W", 18),
                        o.get("scratch", scratch.data_ptr()), o.get("nbytes", nbytes), o.get("out", out.data_ptr()), _lib.stream())
    for over in (dict(ref=None), dict(mask=None), dict(H=6), dict(W=8193), dict(scratch=None), dict(nbytes=nbytes - 1), dict(out=None)):
        assert L.pcc_image_compare_masked(*args(**over)) == -1, over
    torch.cuda.synchronize()
    assert (out == -5.0).all()
    assert L.pcc_image_compare_masked(*args()) == 0
    torch.cuda.synchronize()
    assert (out != -5.0).all()
