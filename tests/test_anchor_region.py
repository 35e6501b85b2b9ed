"""The anchor codec with a quality map (pcc_amd.anchor: compress(quality=...), compress_to_bytes; the PCR2 attributes of
pcc_amd.raht) end to end on the GPU, and the harness rows built on it: the round trip keeps the voxel order and the 8-bit rule
of the plain stream, the best-quality region decodes to the colours of the uniform stream, the byte search meets its target, and
harness.evaluate_view_dependent gains one anchor row per map.  Clouds: shell_yuv and random_rgb of tests/_raht_reference.py."""
import math
import struct

import numpy as np
import pytest
import torch

import _raht_reference as ref
import _raht_region_reference as reg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def split(stream):
    """PCA1 -> (colorspace byte, geometry, attributes)"""
    assert stream[:4] == b"PCA1"
    space, glen = struct.unpack("<B3xI", stream[4:12])
    return space, stream[12:12 + glen], stream[12 + glen:]


def two_halves(x):
    """quality 1 in the upper half along x, 0.25 in the lower"""
    c = x[:, 0]
    return np.where(c > (c.min() + c.max()) / 2, 1.0, 0.25)


@pytest.mark.parametrize("name", ("shell_yuv", "random_rgb"))
def test_round_trip_with_a_quality_map(pcc, name):
    from pcc_amd import anchor, raht
    x, qstep, space = ref.anchor_cases()[name]
    want = ref.anchor_reference(name)[0]
    n = x.shape[0]
    X = torch.from_numpy(x).to(DEV)
    q = two_halves(x)
    stream = anchor.compress(X, qstep, colorspace=space, quality=torch.from_numpy(q).to(DEV), block_log2=2, span=24)
    plain = anchor.compress(X, qstep, colorspace=space)
    code, geometry, attributes = split(stream)
    assert attributes[:4] == b"PCR2" and split(plain)[2][:4] == b"PCR1" and geometry == split(plain)[1] and code == split(plain)[0]
    # a map of two columns is a Q map: the attribute column counts; a host array is a tensor; one column is a vector
    for same in (np.stack([np.zeros(n), q], axis=1), q[:, None], torch.from_numpy(q)):
        assert anchor.compress(X, qstep, colorspace=space, quality=same, block_log2=2) == stream
    rec = anchor.decompress(stream, DEV)
    assert rec.dtype == torch.float32 and tuple(rec.shape) == (n, 6)
    rec = rec.cpu().numpy()
    xyz = np.round(x[:, :3]).astype(np.int64)
    assert np.array_equal(rec[:, :3].astype(np.int64), xyz[want["perm"]])           # ascending Morton order, as the plain stream
    # the colours are the PCR2 reconstruction under the plain stream's clamp / round rule
    depth, _, _, _, ox, oy, oz, _ = struct.unpack("<BBHi3iI", geometry[4:28])
    p = raht.plan(torch.from_numpy(xyz).to(DEV), origin=(ox, oy, oz), depth=depth)
    dec = raht.decode_attributes(p, attributes, channels=3)
    rgb = anchor.from_coded(dec, space)
    assert np.array_equal(rec[:, 3:], (torch.clamp(torch.round(rgb * 255), 0.0, 255.0) / 255).to(torch.float32).cpu().numpy())
    # the levels are those of the map: 0 where the quality is 1, rint(0.75 * 24) = 18 elsewhere, the minimum per block
    levels = raht.quality_levels(q, 24)
    assert sorted(set(levels.tolist())) == [0, 18]
    block_of_row, n_blocks = reg.blocks_from_keys(want, 2)
    bl = reg.block_levels(want, levels, block_of_row, n_blocks)
    _, _, region = raht.decode_region(p, attributes)
    assert np.array_equal(region.block_level.cpu().numpy(), bl)
    # the rows of the best blocks are the uniform stream's colours, the others are not all
    best = bl[block_of_row] == 0
    plain_rec = anchor.decompress(plain, DEV).cpu().numpy()
    assert best.any() and not best.all()
    assert np.array_equal(rec[best], plain_rec[best]) and not np.array_equal(rec[~best], plain_rec[~best])
    assert len(stream) < len(plain)
    print(f"{name}: {len(plain)} bytes uniform, {len(stream)} with the two-halves map ({struct.unpack('<I', attributes[25:29])[0]} of them levels)")
    # streams that are cut or carry a block size that is none are refused
    at = 12 + len(geometry)
    other = bytearray(stream)
    other[at + 6] = 18
    for bad in (stream[:-5], stream[:at + 20], stream[:at + 30], bytes(other)):
        with pytest.raises(ValueError):
            anchor.decompress(bad, DEV)
    for bad_q in (q[:-1], np.stack([q, q, q], axis=1)):
        with pytest.raises(ValueError):
            anchor.compress(X, qstep, quality=bad_q)
    with pytest.raises(ValueError):
        anchor.compress(X, qstep, quality=q, span=64)


@pytest.mark.parametrize("with_map", (False, True))
def test_compress_to_bytes(pcc, with_map):
    from pcc_amd import anchor
    x, _, space = ref.anchor_cases()["shell_yuv"]
    X = torch.from_numpy(x).to(DEV)
    q = two_halves(x) if with_map else None
    mid = 6 / 255
    target = len(anchor.compress(X, mid, colorspace=space, quality=q))
    data, qstep, reached = anchor.compress_to_bytes(X, target, quality=q, colorspace=space)
    assert reached and len(data) <= target
    # the finest step tried that fits, and what compress writes at it.  The step the target came from fits, and twelve halvings
    # of log(256) leave a bracket of ratio 256^(2^-12) = 1.0014 around the threshold; 1 % allows for a rate that is not
    # monotone to the byte
    assert 0.25 / 255 <= qstep <= mid * 1.01
    assert data == anchor.compress(X, qstep, colorspace=space, quality=q)
    assert split(data)[2][:4] == (b"PCR2" if with_map else b"PCR1")
    print(f"compress_to_bytes: target {target}, reached {len(data)} at qstep {qstep * 255:.4f}/255")
    # a finer budget is met with a coarser step, an ample one with the finest
    tight, q_tight, ok = anchor.compress_to_bytes(X, target - 200, quality=q, colorspace=space)
    assert ok and len(tight) <= target - 200 and q_tight > qstep
    ample, q_ample, ok = anchor.compress_to_bytes(X, 10 ** 7, quality=q, colorspace=space)
    assert ok and q_ample == 0.25 / 255
    data, qstep, reached = anchor.compress_to_bytes(X, 16, quality=q, colorspace=space)
    assert not reached and qstep == 64 / 255 and data == anchor.compress(X, 64 / 255, colorspace=space, quality=q)
    with pytest.raises(ValueError):
        anchor.compress_to_bytes(X, target, quality=q, colourspace="rgb")
    with pytest.raises(ValueError):
        anchor.compress_to_bytes(X, target, quality=q, qstep_lo=1.0, qstep_hi=0.5)


@pytest.fixture(scope="module")
def frame(pcc):
    syn = pcc.synthetic
    pts = syn.sphere_shell(**syn.CONFIG1)
    return pts, {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}


def test_evaluate_anchor_row_with_a_quality_map(pcc, frame):
    from pcc_amd import harness
    pts, data = frame
    q = two_halves(pts)
    plain = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=31)
    row = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=31, quality=q, block_log2=2, span=24)
    assert set(row) == set(plain) and "levels_bytes" in row
    assert plain["levels_bytes"] == 0 and 0 < row["levels_bytes"] < 200
    assert row["codec"] == "octree+raht" and row["qstep"] == 8 / 255 and row["n_source"] == row["n_decoded"] == pts.shape[0]
    assert row["sym_p2p_psnr"] == float("inf") and row["bpp"] < plain["bpp"] and row["sym_y_psnr"] < plain["sym_y_psnr"]
    small = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=31, downsample=2, quality=np.stack([q, q], axis=1))
    assert small["downsample"] == 2.0 and small["n_source"] == small["n_decoded"] < pts.shape[0] and small["levels_bytes"] > 0


def test_view_dependent_rows_gain_an_anchor(pcc, frame, tmp_path):
    """the model fixture of tests/test_view_harness.py: seeded weights on the config-1 shell"""
    from pcc_amd import harness, synthetic as syn
    from pcc_amd.harness import evaluate_view_dependent
    pts, data = frame
    model = syn.make_model(seed=0, device=DEV)
    model.update()
    args = ("exp", model, data, 0.8, 0.4, DEV, str(tmp_path))
    kw = dict(view="front", H=160, W=96, gradient=(2, 4.0, 28.0), roi=(0, 16))
    today = evaluate_view_dependent(*args, **kw)
    none = evaluate_view_dependent(*args, anchor=None, **kw)
    assert list(none) == ["uniform", "view", "roi"] and none == today
    details = {}
    # (the seeded weights spend 3.7 bits per point on this frame, little more than the anchor's lossless PCO1 geometry alone:
    # the matched rows take the cheaper PCO2 geometry and end at steps beyond any 8-bit level)
    rows = evaluate_view_dependent(*args, anchor={"block_log2": 2, "contexts": True}, facing={"radius": 3}, details=details, **kw)
    keys = ["uniform", "view", "roi", "facing"]
    assert list(rows) == keys + ["anchor_" + k for k in keys]
    n = pts.shape[0]
    for k in keys:
        if k != "facing":
            assert rows[k] == today[k]                                   # the model's rows are untouched
        row = rows["anchor_" + k]
        assert set(row) == {"bpp", "q_a", "q_g", "key", "psnr", "ssim", "codec", "qstep", "reached", "levels_bytes"}
        assert row["codec"] == "anchor" and row["key"] == "anchor_" + k and row["reached"] is True
        lo, hi = harness.ANCHOR_MATCH_QSTEPS
        assert row["bpp"] <= rows[k]["bpp"] and lo <= row["qstep"] <= hi
        assert math.isfinite(row["psnr"]) and -1.0 <= row["ssim"] <= 1.0
        rec, img = details["anchor_" + k]
        assert tuple(rec.shape) == (n, 6) and img.shape == details["source"][1].shape
        print("anchor_%-8s bpp %.4f (model %.4f) qstep %.3f/255 psnr %.3f ssim %.5f levels %d B" % (
            k, row["bpp"], rows[k]["bpp"], row["qstep"] * 255, row["psnr"], row["ssim"], row["levels_bytes"]))
    assert rows["anchor_uniform"]["levels_bytes"] == 0 and rows["anchor_roi"]["levels_bytes"] > 0       # PCR1, PCR2
    # without match the rows are coded at the given step
    fixed = evaluate_view_dependent(*args, anchor={"match": False, "qstep": 8 / 255, "span": 12}, **kw)
    assert [fixed["anchor_" + k]["qstep"] for k in ("uniform", "view", "roi")] == [8 / 255] * 3
    assert fixed["anchor_roi"]["bpp"] < fixed["anchor_uniform"]["bpp"]
    for bad in ({"qsteps": 1.0}, {"match": False}):
        with pytest.raises(ValueError):
            evaluate_view_dependent(*args, anchor=bad, **kw)
