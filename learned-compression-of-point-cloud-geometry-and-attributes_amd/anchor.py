"""The octree + RAHT anchor codec: a conventional, G-PCC-style point-cloud coder assembled from this package's own parts, for the
rate-distortion sweep to compare the learned codec against (the reference compares against MPEG's G-PCC and V-PCC binaries,
evaluate.py:55-216 and plot.py:373-404, which are not part of its tree).  It is NOT G-PCC compatible.

Geometry: lossless, the "PCO1" octree stream (octree.py), or with ``contexts=True`` its neighbour-context form "PCO2".  Lossy geometry rate points come from coding a down-sampled cloud
(voxelize.downsample).  Attributes: RAHT coefficients quantised with one step size and range coded, "PCR1" (raht.py), by default
in BT.709 YUV.  The RAHT plan uses the origin and depth of the PCO1 header, so the decoder rebuilds it from the geometry alone.

Stream (little-endian):  "PCA1" | u8 colorspace (0 rgb, 1 yuv) | u8[3] 0 | u32 len_geometry | PCO1 | PCR1
"""
import struct

import numpy as np
import torch

from . import octree, raht

MAGIC = b"PCA1"
COLORSPACES = {"rgb": 0, "yuv": 1}
# the BT.709 matrix of metrics.rgb_to_yuv, applied in float64 to the colours as they are (no 8-bit truncation, no chroma offset:
# the transform's DC carries any offset); the inverse is numpy's
RGB_TO_YUV = np.array([[0.2126, 0.7152, 0.0722], [-0.1146, -0.3854, 0.5], [0.5, -0.4542, -0.0458]], dtype=np.float64)
YUV_TO_RGB = np.linalg.inv(RGB_TO_YUV)


def _mix(matrix, c):
    """rows of c [N,3] float64 times matrix^T, every product and sum written out (no BLAS: the bytes do not depend on a library)"""
    m = matrix.tolist()
    return torch.stack([m[r][0] * c[:, 0] + m[r][1] * c[:, 1] + m[r][2] * c[:, 2] for r in range(3)], dim=1)


def to_coded(rgb, colorspace="yuv"):
    """rgb [N,3] in [0, 1] -> float64 [N,3] in the colour space the attributes are coded in"""
    if colorspace not in COLORSPACES:
        raise ValueError(f"colorspace {colorspace!r}: 'yuv' or 'rgb'")
    c = rgb.to(torch.float64)
    return _mix(RGB_TO_YUV, c) if colorspace == "yuv" else c


def from_coded(values, colorspace="yuv"):
    """the inverse of ``to_coded``: float64 [N,3] -> float64 rgb, not clamped"""
    if colorspace not in COLORSPACES:
        raise ValueError(f"colorspace {colorspace!r}: 'yuv' or 'rgb'")
    c = values.to(torch.float64)
    return _mix(YUV_TO_RGB, c) if colorspace == "yuv" else c


def _geometry_header(pco1):
    """PCO1 or PCO2 bytes (the same 28-byte header) -> (depth, (ox, oy, oz), n)"""
    if len(pco1) < 28 or pco1[:4] not in (octree.MAGIC, octree.MAGIC_CONTEXTS):
        raise ValueError("PCA1: the geometry is neither a PCO1 nor a PCO2 stream")
    depth, _, _, _, ox, oy, oz, n = struct.unpack("<BBHi3iI", pco1[4:28])
    return depth, (ox, oy, oz), n


def compress(x, qstep, colorspace="yuv", path=None, contexts=False):
    """x: [N,6] on the GPU (integer voxel coordinates as floats + rgb in [0, 1]; no voxel twice), ``qstep``: the quantisation
    step of the RAHT coefficients (colour units: 1/255 is one 8-bit level) -> PCA1 bytes, also written to ``path`` if given.
    ``contexts``: code the geometry as PCO2 (neighbour contexts) instead of PCO1; ``decompress`` reads either."""
    if colorspace not in COLORSPACES:
        raise ValueError(f"colorspace {colorspace!r}: 'yuv' or 'rgb'")
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("anchor.compress: the cloud must live on the GPU; there is no CPU path")
    if x.dim() != 2 or x.shape[1] < 6 or x.shape[0] < 1:
        raise ValueError(f"anchor.compress: expected a [N, 6] cloud (xyz + rgb) with N >= 1, got {tuple(x.shape)}")
    xyz = torch.round(x[:, :3]).to(torch.int32)
    coords = torch.cat([torch.zeros_like(xyz[:, :1]), xyz], dim=1).contiguous()
    geometry = octree.encode_coordinates(coords, 1, contexts=contexts)
    depth, origin, _ = _geometry_header(geometry)
    p = raht.plan(coords, origin=origin, depth=depth)
    attributes = raht.encode_attributes(p, to_coded(x[:, 3:6], colorspace), qstep)
    data = MAGIC + struct.pack("<B3xI", COLORSPACES[colorspace], len(geometry)) + geometry + attributes
    if path is not None:
        with open(path, "wb") as f:
            f.write(data)
    return data


def decompress(data_or_path, device="cuda:0"):
    """PCA1 bytes (or the path of a file that holds them) -> float32 [N,6] on ``device``: the voxels in ascending Morton order,
    rgb = clamp(round(c * 255), 0, 255) / 255 like ColorModel's reconstruction.  ValueError for a stream that is not one or is
    cut short."""
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        data = bytes(data_or_path)
    else:
        with open(data_or_path, "rb") as f:
            data = f.read()
    if len(data) < 12 or data[:4] != MAGIC:
        raise ValueError("not a PCA1 stream")
    space, glen = struct.unpack("<B3xI", data[4:12])
    names = {v: k for k, v in COLORSPACES.items()}
    if space not in names or len(data) < 12 + glen:
        raise ValueError("PCA1: bad header or truncated geometry")
    geometry, attributes = data[12:12 + glen], data[12 + glen:]
    depth, origin, n = _geometry_header(geometry)
    if n < 1:
        raise ValueError("PCA1: an empty cloud")
    coords = octree.decode_coordinates(geometry, device)
    p = raht.plan(coords, origin=origin, depth=depth)
    coded = raht.decode_attributes(p, attributes, channels=3)
    rgb = torch.clamp(torch.round(from_coded(coded, names[space]) * 255), 0.0, 255.0) / 255
    return torch.cat([coords.index_select(0, p.perm.long())[:, 1:4].to(torch.float32), rgb.to(torch.float32)], dim=1)
