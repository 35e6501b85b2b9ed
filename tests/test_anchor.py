"""The octree + RAHT anchor codec (pcc_amd.anchor, pcc_amd.raht) end to end on the GPU: lossless geometry in Morton order, symbols
that survive the stream and equal numpy's, the distortion bound of an orthonormal transform with a uniform quantiser, a rate that
falls with the step size, the harness row, and streams that are refused.  The clouds are those of tests/_raht_reference.py
(anchor_cases): the 32^3 sphere shell with smooth colours and 4,000 random voxels at depth 10, rows shuffled."""
import struct

import numpy as np
import pytest
import torch

import _raht_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = sorted(ref.anchor_cases())


def split(stream):
    """PCA1 -> (colorspace byte, PCO1, PCR1)"""
    assert stream[:4] == b"PCA1"
    space, glen = struct.unpack("<B3xI", stream[4:12])
    return space, stream[12:12 + glen], stream[12 + glen:]


@pytest.mark.parametrize("name", CASES)
def test_round_trip(pcc, name):
    from pcc_amd import anchor, raht
    x, qstep, space = ref.anchor_cases()[name]
    want, a, co_ref, tol, sym_ref = ref.anchor_reference(name)
    n = x.shape[0]
    X = torch.from_numpy(x).to(DEV)
    stream = anchor.compress(X, qstep, colorspace=space)
    code, pco1, pcr1 = split(stream)
    assert code == {"rgb": 0, "yuv": 1}[space]
    rec = anchor.decompress(stream, DEV)
    assert rec.dtype == torch.float32 and tuple(rec.shape) == (n, 6)
    rec = rec.cpu().numpy()
    # the decoded voxels are the input's, in ascending Morton order (the order of the restatement's plan)
    xyz = np.round(x[:, :3]).astype(np.int64)
    assert np.array_equal(rec[:, :3].astype(np.int64), xyz[want["perm"]])
    # the plan is made from the PCO1 header's origin and depth: the octree coder's rule
    depth, _, _, _, ox, oy, oz, n_head = struct.unpack("<BBHi3iI", pco1[4:28])
    assert (depth, [ox, oy, oz], n_head) == (want["depth"], xyz.min(axis=0).tolist(), n)
    p = raht.plan(torch.from_numpy(xyz).to(DEV), origin=(ox, oy, oz), depth=depth)
    # the attribute stream is what encode_attributes writes for the coded colours; its symbols come back from the decoder ...
    coded = anchor.to_coded(X[:, 3:6], space)
    assert np.array_equal(coded.cpu().numpy(), a)
    data, sym = raht.encode_attributes(p, coded, qstep, return_symbols=True)
    assert data == pcr1
    back, q = raht.decode_symbols(p, pcr1)
    assert q == qstep and back.dtype == np.int64 and np.array_equal(back, sym)
    # ... and equal numpy's rint(coefficient / qstep) wherever a coefficient within the tolerance cannot round the other way:
    # everywhere (the cases are chosen so; tests/test_raht_reference.py checks that on the CPU)
    co = raht.forward(p, coded).cpu().numpy()
    print(f"{name}: forward max error {np.abs(co - co_ref).max():.3e} (bound {tol:.3e}), bit-equal {np.array_equal(co, co_ref)}")
    assert np.abs(co - co_ref).max() <= tol
    excluded = ref.near_rounding_boundary(co_ref, qstep, tol)
    assert int(excluded.sum()) == 0
    assert np.array_equal(sym[~excluded], sym_ref[~excluded])
    # distortion in the coded colour space before the 8-bit rounding: the transform is orthonormal and every coefficient is
    # off by at most qstep / 2
    dec = raht.decode_attributes(p, pcr1, channels=3).cpu().numpy()
    mse = ((dec - a[want["perm"]]) ** 2).mean()
    print(f"{name}: mse {mse:.6e}, bound {qstep ** 2 / 4:.6e}, {len(stream) * 8 / n:.3f} bpp")
    assert mse <= qstep ** 2 / 4 * (1 + 1e-9)
    # the colours that come out are that reconstruction, rounded to 8 bits like ColorModel's
    rgb = anchor.from_coded(torch.from_numpy(dec).to(DEV), space)
    assert np.array_equal(rec[:, 3:], (torch.clamp(torch.round(rgb * 255), 0.0, 255.0) / 255).to(torch.float32).cpu().numpy())


def test_rate_falls_with_the_step_on_smooth_colours(pcc, tmp_path):
    from pcc_amd import anchor
    x, _, _ = ref.anchor_cases()["shell_yuv"]
    X = torch.from_numpy(x).to(DEV)
    fine, coarse = anchor.compress(X, 1 / 255), anchor.compress(X, 32 / 255, path=str(tmp_path / "coarse.bin"))
    assert len(coarse) < len(fine)
    assert split(fine)[1] == split(coarse)[1]                     # the same geometry bytes
    assert len(split(coarse)[2]) < len(split(fine)[2])
    print(f"shell: {len(fine)} bytes at qstep 1/255, {len(coarse)} at 32/255 ({len(split(fine)[1])} of them geometry)")
    # a stream read from a file decodes like the bytes
    assert torch.equal(anchor.decompress(str(tmp_path / "coarse.bin"), DEV), anchor.decompress(coarse, DEV))


def test_evaluate_anchor_row(pcc, tmp_path):
    from pcc_amd import harness
    syn = pcc.synthetic
    pts = syn.sphere_shell(**syn.CONFIG1)
    data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
    row = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=31)
    model = syn.make_model(0, DEV)
    model.update()
    frame_row = harness.evaluate_frame("anchor_test", model, data, 0.5, 0.5, DEV, str(tmp_path), resolution=31)
    assert set(frame_row) - {"q_g", "q_a"} <= set(row)            # (the anchor has no quality map; its knob is qstep)
    assert row["codec"] == "octree+raht" and row["qstep"] == 8 / 255
    assert row["n_source"] == row["n_decoded"] == pts.shape[0]
    assert row["sym_p2p_psnr"] == float("inf")                    # lossless geometry
    assert 20.0 < row["sym_y_psnr"] < 60.0 and row["bpp"] > 0 and row["t_compress"] > 0 and row["t_decompress"] > 0
    small = harness.evaluate_anchor(data, 8 / 255, DEV, resolution=31, downsample=2, colorspace="rgb")
    assert small["downsample"] == 2.0 and small["n_input"] == pts.shape[0] and small["n_source"] == small["n_decoded"] < pts.shape[0]


def test_bad_streams_are_refused(pcc):
    from pcc_amd import anchor
    x, qstep, space = ref.anchor_cases()["shell_yuv"]
    stream = anchor.compress(torch.from_numpy(x).to(DEV), qstep, colorspace=space)
    _, pco1, pcr1 = split(stream)
    at = 12 + len(pco1)
    flipped = bytearray(stream)
    flipped[at] ^= 0x20                                          # the PCR1 magic
    for bad in (b"QCA1" + stream[4:], bytes(flipped), stream[:-7], stream[:at + 10], stream[:at - 5], stream[:9]):
        with pytest.raises(ValueError):
            anchor.decompress(bad, DEV)
    # a cloud with a voxel twice is refused by the encoder
    twice = torch.from_numpy(np.concatenate([x, x[:1]])).to(DEV)
    with pytest.raises(ValueError):
        anchor.compress(twice, qstep)
    with pytest.raises(ValueError):
        anchor.compress(torch.from_numpy(x).to(DEV), 0.0)
