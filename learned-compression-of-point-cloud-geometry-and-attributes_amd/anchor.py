"""The octree + RAHT anchor codec: a conventional, G-PCC-style point-cloud coder assembled from this package's own parts, for the
rate-distortion sweep to compare the learned codec against (the reference compares against MPEG's G-PCC and V-PCC binaries,
evaluate.py:55-216 and plot.py:373-404, which are not part of its tree).  It is NOT G-PCC compatible.

Geometry: lossless, the "PCO1" octree stream (octree.py), or with ``contexts=True`` its neighbour-context form "PCO2".  Lossy geometry rate points come either from coding a down-sampled cloud
(voxelize.downsample: another grid, judged against the down-sampled cloud) or from ``compress(..., scale=...)``, position scaling
with recolouring (rescale.py: the cells are coded, the decoder scales them back, and the result is judged against the original
frame at its own resolution — G-PCC's positionQuantizationScale).  Attributes: RAHT coefficients quantised with one step size and range coded, "PCR1" (raht.py), by default
in BT.709 YUV.  The RAHT plan uses the origin and depth of the PCO1 header, so the decoder rebuilds it from the geometry alone.

With a quality map (``compress(..., quality=...)``) the attributes are quantised region by region, "PCR2" (raht.py): the anchor's
counterpart of G-PCC's region-wise QP offsets, so that the learned codec's spatially steered rows have a conventional baseline;
``compress_to_bytes`` searches the qstep that meets a byte budget.

Stream (little-endian):  "PCA1" | u8 colorspace (0 rgb, 1 yuv) | u8[3] 0 | u32 len_geometry | PCO1 or PCO2 | PCR1 or PCR2
With a scale:            "PCA2" | u8 colorspace | u8 num | u8 den | u8 0 | u32 len_geometry | PCO1 or PCO2 of the CELLS | PCR1 or PCR2
"""
import struct

import numpy as np
import torch

from . import octree, raht, rescale

MAGIC = b"PCA1"
MAGIC_SCALED = b"PCA2"
# the joint operating points at which the reference places G-PCC beside the learned codec, (positionQuantizationScale, QP):
# plot.py:34 and evaluate_view_dep.py:95 of the reference
GPCC_POINTS = ((0.125, 51), (0.25, 46), (0.5, 40), (0.75, 34))
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


def qp_to_qstep(qp):
    """the quantisation step (colour units, 1/255 = one 8-bit level) that stands for a G-PCC attribute QP:
    ``2**((qp - 4) / 6) / 255``, the step rule of the HEVC family (the step doubles every 6 QP and is 1 at QP 4) as recalled.
    tmc3 is not part of this tree or of the reference's, so the rule could not be checked against it: the anchor's rows at
    ``GPCC_POINTS`` are points of THIS codec placed by that rule, not G-PCC's."""
    return 2.0 ** ((float(qp) - 4.0) / 6.0) / 255.0


def _geometry_header(pco1):
    """PCO1 or PCO2 bytes (the same 28-byte header) -> (depth, (ox, oy, oz), n)"""
    if len(pco1) < 28 or pco1[:4] not in (octree.MAGIC, octree.MAGIC_CONTEXTS):
        raise ValueError("PCA1: the geometry is neither a PCO1 nor a PCO2 stream")
    depth, _, _, _, ox, oy, oz, n = struct.unpack("<BBHi3iI", pco1[4:28])
    return depth, (ox, oy, oz), n


def _attribute_quality(quality, n, device):
    """a quality map [N], [N,1] or [N,2] (a Q map's channels [q_g, q_a]: the attribute column counts) -> float64 [N] on
    ``device``"""
    q = quality if isinstance(quality, torch.Tensor) else torch.as_tensor(np.asarray(quality))
    if q.dim() not in (1, 2) or q.shape[0] != n or (q.dim() == 2 and q.shape[1] not in (1, 2)):
        raise ValueError(f"anchor: a quality map of shape {tuple(q.shape)}: need [{n}], [{n}, 1] or [{n}, 2]")
    return q.reshape(n, -1)[:, -1].to(device=device, dtype=torch.float64)


def _prepare(x, colorspace, contexts, quality, block_log2, span, scale=None, transfer="nearest"):
    """what ``compress`` codes and does not depend on qstep: (the head of the stream with the geometry, the RAHT plan, the
    coefficients, the ``raht.Region`` of the quality map or None).  With a ``scale`` the cloud coded is the cell cloud of
    ``rescale.quantize`` with its transferred colours, and a cell's quality is the maximum over its own points."""
    if colorspace not in COLORSPACES:
        raise ValueError(f"colorspace {colorspace!r}: 'yuv' or 'rgb'")
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("anchor.compress: the cloud must live on the GPU; there is no CPU path")
    if x.dim() != 2 or x.shape[1] < 6 or x.shape[0] < 1:
        raise ValueError(f"anchor.compress: expected a [N, 6] cloud (xyz + rgb) with N >= 1, got {tuple(x.shape)}")
    if transfer not in rescale.TRANSFERS:
        raise ValueError(f"transfer {transfer!r}: 'nearest' or 'cell'")
    if scale is None:
        xyz = torch.round(x[:, :3]).to(torch.int32)
        coords = torch.cat([torch.zeros_like(xyz[:, :1]), xyz], dim=1).contiguous()
        colours, magic, fields = x[:, 3:6], MAGIC, (0, 0)
    else:
        s = rescale.quantize(x[:, :6], scale, transfer)
        coords, colours, magic, fields = s.cells, s.features, MAGIC_SCALED, (s.num, s.den)
        if quality is not None:
            q = _attribute_quality(quality, x.shape[0], x.device)
            quality = torch.zeros(coords.shape[0], dtype=torch.float64, device=x.device).scatter_reduce(
                0, s.row.long(), q, reduce="amax", include_self=False)
    geometry = octree.encode_coordinates(coords, 1, contexts=contexts)
    depth, origin, _ = _geometry_header(geometry)
    p = raht.plan(coords, origin=origin, depth=depth)
    region = None
    if quality is not None:
        region = raht.region(p, raht.quality_levels(_attribute_quality(quality, p.n, x.device), span), block_log2)
    head = magic + struct.pack("<BBBxI", COLORSPACES[colorspace], fields[0], fields[1], len(geometry)) + geometry
    return head, p, raht.forward(p, to_coded(colours, colorspace)), region


def _code(p, coeffs, qstep, region):
    """the attribute stream of the coefficients at ``qstep``: PCR1, or PCR2 with a region"""
    return raht.encode_coefficients(p, coeffs, qstep) if region is None else raht.encode_region(p, coeffs, qstep, region)


def compress(x, qstep, colorspace="yuv", path=None, contexts=False, quality=None, block_log2=3, span=24, scale=None, transfer="nearest"):
    """x: [N,6] on the GPU (integer voxel coordinates as floats + rgb in [0, 1]; no voxel twice), ``qstep``: the quantisation
    step of the RAHT coefficients (colour units: 1/255 is one 8-bit level) -> PCA1 bytes, also written to ``path`` if given.
    ``contexts``: code the geometry as PCO2 (neighbour contexts) instead of PCO1; ``decompress`` reads either.

    ``quality``: a quality map in x's row order, [N], [N,1] or [N,2] with values in [0, 1]; of two columns (a Q map's
    [q_g, q_a]) the second, the attribute quality, is used: the geometry is lossless here, so a geometry quality has no
    meaning.  The attributes are then the region-wise stream PCR2: every cube of edge 2^block_log2 is quantised with the
    level ``raht.quality_levels(quality, span)`` of its best point, quality 1 at ``qstep`` itself, quality 0 at
    ``raht.level_steps(qstep)[span]``.  The PCA1 container is the same; ``decompress`` tells the two by the attribute magic.

    ``scale`` (what ``rescale.as_scale`` takes: a (num, den) pair, a Fraction, or a float such as 0.125, 0.25, 0.5, 0.75; None:
    lossless geometry, the PCA1 stream byte for byte): lossy geometry by position scaling -> PCA2 bytes.  The geometry stream
    codes the CELLS of ``rescale.quantize(x, scale, transfer)``, the RAHT plan is made of the cells, and the attributes are the
    colours transferred onto them (``transfer``: "nearest", each cell the mean of the points whose nearest reconstructed
    position it is, or "cell", the mean of its own points).  Duplicate voxels are merged by the quantisation.  With a
    ``quality`` map a cell's quality is the maximum over its own points (PCR2's own "finest level wins")."""
    head, p, coeffs, region = _prepare(x, colorspace, contexts, quality, block_log2, span, scale, transfer)
    data = head + _code(p, coeffs, qstep, region)
    if path is not None:
        with open(path, "wb") as f:
            f.write(data)
    return data


def compress_to_bytes(x, target_bytes, quality=None, qstep_lo=0.25 / 255, qstep_hi=64 / 255, iterations=12, **kw):
    """``compress`` at the finest qstep in [qstep_lo, qstep_hi] whose whole PCA1 stream has at most ``target_bytes`` bytes ->
    (data, qstep, reached).  Bisection in log qstep, ``iterations`` probes after the two ends; geometry, plan, coefficients
    and coefficient levels are made once, only the quantiser and the coder run per probe.  ``reached`` is False, with the
    stream at ``qstep_hi``, when even that is larger than the target.  ``kw``: ``compress``'s colorspace, contexts,
    block_log2, span, scale, transfer (the quantisation and the colour transfer of a scale are made once too)."""
    unknown = set(kw) - {"colorspace", "contexts", "block_log2", "span", "scale", "transfer"}
    if unknown:
        raise ValueError("compress_to_bytes: unknown arguments %s" % sorted(unknown))
    lo, hi = raht._check_qstep(qstep_lo), raht._check_qstep(qstep_hi)
    if lo > hi:
        raise ValueError(f"compress_to_bytes: qstep_lo {lo} above qstep_hi {hi}")
    head, p, coeffs, region = _prepare(x, kw.get("colorspace", "yuv"), kw.get("contexts", False), quality, kw.get("block_log2", 3),
                                       kw.get("span", 24), kw.get("scale"), kw.get("transfer", "nearest"))
    probe = lambda q: head + _code(p, coeffs, q, region)
    best = probe(hi)
    if len(best) > target_bytes:
        return best, hi, False
    data = probe(lo)
    if len(data) <= target_bytes:
        return data, lo, True
    best_q = hi
    for _ in range(int(iterations)):
        mid = float(np.sqrt(lo * hi))
        data = probe(mid)
        if len(data) <= target_bytes:
            best, best_q, hi = data, mid, mid
        else:
            lo = mid
    return best, best_q, True


def decompress(data_or_path, device="cuda:0"):
    """PCA1 or PCA2 bytes (or the path of a file that holds them) -> float32 [N,6] on ``device``: the voxels in ascending Morton
    order, rgb = clamp(round(c * 255), 0, 255) / 255 like ColorModel's reconstruction.  For PCA2 the rows are the M cells in
    ascending Morton order of the CELLS, each at its position ``rescale.positions_of(cell, num, den)`` on the original grid.
    ValueError for a stream that is not one, is cut short, or carries a scale that is none (num = 0, num > den)."""
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        data = bytes(data_or_path)
    else:
        with open(data_or_path, "rb") as f:
            data = f.read()
    if len(data) < 12 or data[:4] not in (MAGIC, MAGIC_SCALED):
        raise ValueError("not a PCA1 or PCA2 stream")
    scaled = data[:4] == MAGIC_SCALED
    space, num, den, zero, glen = struct.unpack("<BBBBI", data[4:12])
    names = {v: k for k, v in COLORSPACES.items()}
    if space not in names or len(data) < 12 + glen:
        raise ValueError("PCA1: bad header or truncated geometry")
    if scaled and (zero != 0 or not 1 <= num <= den):
        raise ValueError(f"PCA2: bad header: scale {num} / {den}")
    geometry, attributes = data[12:12 + glen], data[12 + glen:]
    depth, origin, n = _geometry_header(geometry)
    if n < 1:
        raise ValueError("PCA1: an empty cloud")
    coords = octree.decode_coordinates(geometry, device)
    p = raht.plan(coords, origin=origin, depth=depth)
    coded = raht.decode_attributes(p, attributes, channels=3)
    rgb = torch.clamp(torch.round(from_coded(coded, names[space]) * 255), 0.0, 255.0) / 255
    xyz = coords.index_select(0, p.perm.long())[:, 1:4]
    if scaled:
        xyz = rescale.positions_of(xyz, num, den)
    return torch.cat([xyz.to(torch.float32), rgb.to(torch.float32)], dim=1)
