"""The anchor codec with lossy geometry by position scaling (pcc_amd.anchor: compress(scale=..., transfer=...), the PCA2 stream)
end to end on the GPU: the header, geometry bytes that code the cells, attribute bytes that code the transferred colours,
decoded positions on the original grid, the transform's distortion bound against the transferred colours, scale 1/1 against the
plain stream, the quality map's per-cell maximum, and the byte search.  Clouds: the anchor cases of tests/_raht_reference.py."""
import struct

import numpy as np
import pytest
import torch

import _raht_reference as ref
import _scaled_reference as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(ref.anchor_cases())
SCALES = ((1, 4), (3, 4))


def split(stream, magic=b"PCA2"):
    """-> (colorspace, num, den, reserved, geometry, attributes)"""
    assert stream[:4] == magic
    space, num, den, zero, glen = struct.unpack("<BBBBI", stream[4:12])
    return space, num, den, zero, stream[12:12 + glen], stream[12 + glen:]


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: "%d_%d" % s)
@pytest.mark.parametrize("name", CASES)
def test_stream_and_round_trip(pcc, name, scale):
    from pcc_amd import anchor, octree, raht, rescale
    x, qstep, space = ref.anchor_cases()[name]
    num, den = scale
    X = torch.from_numpy(x).to(DEV)
    xyz = np.round(x[:, :3]).astype(np.int64)
    want = sref.quantize_reference(sref.with_batch(xyz), x[:, 3:6], num, den)
    m = want["cells"].shape[0]
    for transfer, feats in (("nearest", want["features"]), ("cell", want["own_features"])):
        stream = anchor.compress(X, qstep, colorspace=space, scale=scale, transfer=transfer)
        code, h_num, h_den, zero, geometry, attributes = split(stream)
        assert (code, h_num, h_den, zero) == ({"rgb": 0, "yuv": 1}[space], num, den, 0)
        assert stream == anchor.compress(X, qstep, colorspace=space, scale=num / den, transfer=transfer)
        # the geometry codes the cells, the plan is made of the cells, the attributes are the transferred colours
        cells = torch.from_numpy(want["cells"]).to(DEV)
        assert geometry == octree.encode_coordinates(cells, 1)
        depth, _, _, _, ox, oy, oz, n_head = struct.unpack("<BBHi3iI", geometry[4:28])
        assert n_head == m and [ox, oy, oz] == want["cells"][:, 1:].min(axis=0).tolist()
        p = raht.plan(cells, origin=(ox, oy, oz), depth=depth)
        F = torch.from_numpy(feats).to(DEV)
        assert attributes == raht.encode_attributes(p, anchor.to_coded(F, space), qstep)
        # decoded: the cells' positions on the original grid, in ascending Morton order of the cells
        rec = anchor.decompress(stream, DEV)
        assert rec.dtype == torch.float32 and tuple(rec.shape) == (m, 6)
        perm = p.perm.long().cpu().numpy()
        assert np.array_equal(rec[:, :3].cpu().numpy().astype(np.int64), sref.positions_of(want["cells"][perm, 1:], num, den))
        assert np.array_equal(rec[:, :3].cpu().numpy(), rescale.positions_of(cells[:, 1:], num, den)[perm].to(torch.float32).cpu().numpy())
        # distortion against the transferred colours in the coded space, before the 8-bit rounding: the orthonormal-transform bound
        dec = raht.decode_attributes(p, attributes, channels=3).cpu().numpy()
        a = ref.coded_reference(np.concatenate([np.zeros((m, 3), np.float32), feats], axis=1), space)
        mse = ((dec - a[perm]) ** 2).mean()
        print(f"{name} {num}/{den} {transfer}: {m} cells of {x.shape[0]} points, mse {mse:.6e} (bound {qstep ** 2 / 4:.6e}), "
              f"{len(stream) * 8 / x.shape[0]:.3f} bpp")
        assert mse <= qstep ** 2 / 4 * (1 + 1e-9)
        rgb = anchor.from_coded(torch.from_numpy(dec).to(DEV), space)
        assert np.array_equal(rec[:, 3:].cpu().numpy(), (torch.clamp(torch.round(rgb * 255), 0.0, 255.0) / 255).to(torch.float32).cpu().numpy())
        # with PCO2 geometry the cells are coded with neighbour contexts, and the attributes do not change
        ctx = anchor.compress(X, qstep, colorspace=space, scale=scale, transfer=transfer, contexts=True)
        assert split(ctx)[4] == octree.encode_coordinates(cells, 1, contexts=True) and split(ctx)[5] == attributes
        assert torch.equal(anchor.decompress(ctx, DEV), rec)
    if name.startswith("shell"):
        assert m < x.shape[0]                                  # a dense surface: cells merge


@pytest.mark.parametrize("name", ("shell_yuv", "shell_rgb_fine", "one"))
def test_scale_one_decodes_like_the_plain_stream_and_none_is_pca1(pcc, name):
    from pcc_amd import anchor
    x, qstep, space = ref.anchor_cases()[name]
    X = torch.from_numpy(x).to(DEV)
    plain = anchor.compress(X, qstep, colorspace=space)
    assert plain[:4] == b"PCA1" and plain == anchor.compress(X, qstep, colorspace=space, scale=None, transfer="cell")
    assert plain[4:8] == bytes([{"rgb": 0, "yuv": 1}[space], 0, 0, 0])
    for transfer in ("nearest", "cell"):
        one = anchor.compress(X, qstep, colorspace=space, scale=(1, 1), transfer=transfer)
        assert one[:4] == b"PCA2" and one[5:8] == bytes([1, 1, 0]) and one[8:] == plain[8:]
        assert torch.equal(anchor.decompress(one, DEV), anchor.decompress(plain, DEV))
    # a truncated or mislabelled PCA2 stream is refused
    glen = struct.unpack("<I", one[8:12])[0]
    bad_scale = bytearray(one)
    bad_scale[5] = 0
    above = bytearray(one)
    above[5], above[6] = 5, 4
    for bad in (one[:-3], one[:12 + glen - 2], one[:10], bytes(bad_scale), bytes(above)):
        with pytest.raises(ValueError):
            anchor.decompress(bad, DEV)
    with pytest.raises(ValueError):
        anchor.compress(X, qstep, scale=0.3)
    with pytest.raises(ValueError):
        anchor.compress(X, qstep, scale=0.5, transfer="blend")


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: "%d_%d" % s)
def test_quality_map_takes_the_per_cell_maximum(pcc, scale):
    from pcc_amd import anchor
    x, qstep, space = ref.anchor_cases()["shell_yuv"]
    n = x.shape[0]
    X = torch.from_numpy(x).to(DEV)
    want = sref.quantize_reference(sref.with_batch(np.round(x[:, :3]).astype(np.int64)), x[:, 3:6], *scale)
    # quality 1 in the upper half along x, 0.25 or 0.5 at random in the lower: cells of mixed points, where the maximum counts
    q = np.where(x[:, 0] > (x[:, 0].min() + x[:, 0].max()) / 2, 1.0, np.random.default_rng(4).choice([0.25, 0.5], size=n))
    cell_q = np.zeros(len(want["cells"]))
    np.maximum.at(cell_q, want["row"], q)
    assert (cell_q > 0).all() and len(set(cell_q.tolist())) >= 2 and (cell_q != q[want["first"]]).any()
    stream = anchor.compress(X, qstep, colorspace=space, quality=q, block_log2=2, span=24, scale=scale)
    # the cell cloud coded on its own, lossless, with the per-cell maximum
    cloud = torch.from_numpy(np.concatenate([want["cells"][:, 1:].astype(np.float32), want["features"]], axis=1)).to(DEV)
    alone = anchor.compress(cloud, qstep, colorspace=space, quality=cell_q, block_log2=2, span=24)
    assert alone[:4] == b"PCA1" and split(stream)[5][:4] == b"PCR2"
    assert split(stream)[4:] == split(alone, b"PCA1")[4:]
    assert split(stream)[5] != split(anchor.compress(X, qstep, colorspace=space, scale=scale))[5]
    assert anchor.compress(X, qstep, colorspace=space, quality=np.stack([np.zeros(n), q], axis=1), block_log2=2, scale=scale) == stream
    rec = anchor.decompress(stream, DEV)
    assert tuple(rec.shape) == (len(want["cells"]), 6)
    with pytest.raises(ValueError):
        anchor.compress(X, qstep, quality=q[:-1], scale=scale)


def test_compress_to_bytes_with_a_scale(pcc):
    from pcc_amd import anchor
    x, _, space = ref.anchor_cases()["shell_yuv"]
    X = torch.from_numpy(x).to(DEV)
    for scale, transfer in (((1, 4), "nearest"), ((3, 4), "cell")):
        mid = 6 / 255
        target = len(anchor.compress(X, mid, colorspace=space, scale=scale, transfer=transfer))
        data, qstep, reached = anchor.compress_to_bytes(X, target, colorspace=space, scale=scale, transfer=transfer)
        assert reached and len(data) <= target and data[:4] == b"PCA2" and 0.25 / 255 <= qstep <= mid * 1.01
        assert data == anchor.compress(X, qstep, colorspace=space, scale=scale, transfer=transfer)
        print(f"compress_to_bytes at {scale[0]}/{scale[1]}: target {target}, reached {len(data)} at qstep {qstep * 255:.4f}/255")
        tight, q_tight, ok = anchor.compress_to_bytes(X, target - 20, colorspace=space, scale=scale, transfer=transfer)
        assert (len(tight) <= target - 20 and q_tight > qstep) if ok else q_tight == 64 / 255
    with pytest.raises(ValueError):
        anchor.compress_to_bytes(X, target, scales=(1, 4))
