"""harness.evaluate_anchor with a position scale (the PCA2 stream) on the GPU: the row's fields, a D1 PSNR equal to the one the
restatement's brute-force distances give, D1 rising with the scale, and the clash with ``downsample``.  Frame: the 32^3 sphere
shell (synthetic.CONFIG1)."""
import math

import numpy as np
import pytest
import torch

import _scaled_reference as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = ((1, 8), (1, 4), (1, 2), (3, 4))
RESOLUTION = 31


@pytest.fixture(scope="module")
def frame(pcc):
    syn = pcc.synthetic
    pts = syn.sphere_shell(**syn.CONFIG1)
    return pts, {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}


def reference_d1(pts, scale):
    """-> (number of cells, sym D1 PSNR from brute-force distances in both directions: the worse one, as the metric's sym_psnr_mse)"""
    xyz = sref.with_batch(np.round(pts[:, :3]).astype(np.int64))
    want = sref.quantize_reference(xyz, pts[:, 3:6], *scale)
    recon = np.concatenate([want["cells"][:, :1].astype(np.int64), want["positions"].astype(np.int64)], axis=1)
    _, back, _ = sref.brute_nearest(recon, xyz)
    psnr = [10 * math.log10(RESOLUTION ** 2 / float((d2.astype(np.float64) / 3.0).mean())) for d2 in (want["d2"], back)]
    return want["cells"].shape[0], min(psnr)


def test_rows_with_a_scale(pcc, frame):
    from pcc_amd import harness
    pts, data = frame
    n = pts.shape[0]
    plain = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=RESOLUTION)
    assert "scale" not in plain and "transfer" not in plain
    # the restatement's own numbers rise with the scale on this frame; then the harness's must, and must equal them
    refs = [reference_d1(pts, s) for s in SCALES]
    assert all(b[1] > a[1] for a, b in zip(refs, refs[1:]))
    rows = []
    for scale, (m, d1) in zip(SCALES, refs):
        row = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=RESOLUTION, scale=scale)
        assert set(row) == set(plain) | {"scale", "scale_num", "scale_den", "transfer"}
        assert (row["scale"], row["scale_num"], row["scale_den"], row["transfer"]) == (scale[0] / scale[1], scale[0], scale[1], "nearest")
        assert row["codec"] == "octree+raht" and row["n_source"] == n and row["n_decoded"] == m < n
        assert math.isfinite(row["sym_p2p_psnr"]) and abs(row["sym_p2p_psnr"] - d1) <= 1e-9
        assert math.isfinite(row["sym_y_psnr"]) and row["t_compress"] > 0 and row["t_decompress"] > 0
        print(f"scale {scale[0]}/{scale[1]}: {m} cells of {n} points, {row['bpp']:.4f} bpp, D1 {row['sym_p2p_psnr']:.4f} dB "
              f"(restatement {d1:.4f}), Y {row['sym_y_psnr']:.3f} dB")
        rows.append(row)
    assert all(b["sym_p2p_psnr"] > a["sym_p2p_psnr"] for a, b in zip(rows, rows[1:]))
    assert all(r["bpp"] < plain["bpp"] for r in rows)
    # bits per ORIGINAL point: the whole stream over N
    from pcc_amd import anchor
    stream = anchor.compress(torch.from_numpy(pts).to(DEV), 8 / 255, scale=(1, 2))
    assert rows[2]["bpp"] == len(stream) * 8 / n
    # a float scale, the other transfer, PCO2 geometry
    other = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=RESOLUTION, scale=0.5, transfer="cell", contexts=True)
    assert (other["scale_num"], other["scale_den"], other["transfer"]) == (1, 2, "cell")
    assert other["sym_p2p_psnr"] == rows[2]["sym_p2p_psnr"] and other["n_decoded"] == rows[2]["n_decoded"]


def test_scale_clashes_with_downsample(pcc, frame):
    from pcc_amd import harness
    _, data = frame
    with pytest.raises(ValueError):
        harness.evaluate_anchor(data, 8 / 255, DEV, resolution=RESOLUTION, scale=(1, 2), downsample=2)
    with pytest.raises(ValueError):
        harness.evaluate_anchor(data, 8 / 255, DEV, resolution=RESOLUTION, scale=0.3)
    with pytest.raises(ValueError):
        harness.evaluate_anchor(data, 8 / 255, DEV, resolution=RESOLUTION, scale=0.5, transfer="blend")
