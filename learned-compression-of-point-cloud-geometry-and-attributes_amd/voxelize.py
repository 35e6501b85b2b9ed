"""Voxelisation: raw points (float xyz, optional attributes, optional batch index) onto a voxel grid, with EXACT per-voxel
attribute means — what turns a float PLY, a scan whose points collide on the grid, or a frame that should be coded at fewer
bits into the duplicate-free integer voxel list ``ColorModel.compress``, ``octree.encode_coordinates`` and the metrics require.

One call of ``pcc_voxelize`` (csrc/voxelize.hip; the arithmetic is specified in include/pcc_hip.h): the distinct voxels in order
of first appearance, per voxel the point count and the int64 sum of its attributes in Q32 fixed point, per point its voxel row.
The mean is taken here from the integer sums, ``float32(float64(sum) / float64(count) / 2**32)``, so the result is bitwise
reproducible and does not depend on the order in which the GPU's threads arrive.

The grid is anchored at ``origin``: cell = floor (or round-half-even) of ``(p - origin) / voxel_size``, and the coordinates
returned are cell indices.  open3d's ``voxel_down_sample``, through which the reference down-samples its "QA" sequences
(data/utils/RawLoader.py:48-57), anchors its grid at the cloud's minimum bound minus half a voxel and also averages the
positions; neither is imitated: position centroids are out of scope, and a grid that moves with the cloud's bounding box would
make two frames of one sequence disagree about their voxels.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .sparse import CoordinateRangeError, _host_count, _read_count, _require_cuda, _set_buffers

Voxelized = namedtuple("Voxelized", ["coords", "features", "counts", "inverse", "first", "sums"])
Voxelized.__doc__ = """coords int32 [M,4] (batch, cell x, y, z) in order of first appearance; features float32 [M,C] or None;
counts int32 [M] points per voxel; inverse int32 [N] voxel row of every point; first int32 [M] lowest input row of every voxel;
sums int64 [M,C] exact Q32 attribute sums (None without attributes)"""

ROUNDINGS = {"floor": 0, "nearest": 1}
MAX_CHANNELS = 16
COORD_LIMIT = _lib.PCC.COORD_LIMIT
Q32 = 4294967296.0


def _device_of(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("libpcc_hip operators need an MI355X device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(a, dtype, device):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype).contiguous()


def _range_error(P, A, B, nbatch, origin, voxel_size, rounding):
    """the ValueError of a call whose count word was PCC_COUNT_ERR_RANGE, naming what was out of range (error path only: the
    checks of the kernel restated with torch operators on the same device data)"""
    causes = []
    g = (P - torch.tensor(origin, dtype=torch.float32, device=P.device)) / torch.tensor(voxel_size, dtype=torch.float32, device=P.device)
    g = torch.round(g) if rounding else torch.floor(g)
    bad = ~torch.isfinite(g)
    if bool(bad.any()):
        causes.append(f"{int(bad.any(dim=1).sum())} points have a coordinate that is not finite")
    far = torch.isfinite(g) & (g.abs() > COORD_LIMIT)
    if bool(far.any()):
        causes.append(f"{int(far.any(dim=1).sum())} points fall in a cell beyond +-{COORD_LIMIT} (translate the cloud with `origin` or "
                      "use a larger voxel)")
    if B is not None:
        out = (B < 0) | (B >= nbatch)
        if bool(out.any()):
            causes.append(f"{int(out.sum())} batch indices lie outside 0..{nbatch - 1}")
    if A is not None and A.numel():
        wrong = ~(A.abs() <= 1)
        if bool(wrong.any()):
            causes.append(f"{int(wrong.any(dim=1).sum())} points have an attribute that is not finite or exceeds 1 in magnitude "
                          "(attributes are fractions such as colour / 255)")
    return CoordinateRangeError("voxelize: " + ("; ".join(causes) if causes else "a value is outside the supported range"))


def voxelize(points, attributes=None, voxel_size=1.0, origin=(0, 0, 0), rounding="floor", batch=None, reduce="mean"):
    """-> ``Voxelized(coords, features, counts, inverse, first, sums)``, all on the device.

    ``points`` [N,3] float xyz and ``attributes`` [N,C] (C <= 16, values in [-1, 1], e.g. colours / 255) may be device tensors,
    CPU tensors or numpy arrays (uploaded; the work itself always runs on the GPU — there is no CPU path).  The grid is anchored
    at ``origin``: the cell of a point is ``floor((p - origin) / voxel_size)`` (``rounding="floor"``) or that quotient rounded
    to nearest, ties to even (``"nearest"``), every operation in float32; ``coords`` holds (batch, cell indices), voxels in
    order of first appearance, never merged across ``batch`` items (int [N], optional).
    ``reduce="mean"``: ``features`` is the exact mean of each voxel's attributes (rounded once to float32);
    ``reduce="first"``: ``attributes[first]``, the first-occurrence-wins rule.  ``sums`` / ``counts`` are returned either way.
    Raises ValueError naming the cause when a point is not finite or falls beyond cell +-PCC_COORD_LIMIT (include/pcc_hip.h), a batch index is out of range
    or an attribute is not finite or exceeds 1 in magnitude.  One synchronisation: reading the voxel count."""
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding {rounding!r}: 'floor' or 'nearest'")
    if reduce not in ("mean", "first"):
        raise ValueError(f"reduce {reduce!r}: 'mean' or 'first'")
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and np.isfinite(np.float32(voxel_size))):
        raise ValueError(f"voxel_size {voxel_size}: a positive finite number")
    origin = [float(np.float32(v)) for v in np.asarray(origin, dtype=np.float64).reshape(3)]
    dev = _device_of(points, attributes, batch)
    P = _to_device(points, torch.float32, dev)
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError(f"points of shape {tuple(P.shape)}: need [N, 3]")
    _require_cuda(P)
    n = P.shape[0]
    A = None
    if attributes is not None:
        A = _to_device(attributes, torch.float32, dev)
        if A.dim() != 2 or A.shape[0] != n or A.shape[1] > MAX_CHANNELS:
            raise ValueError(f"attributes of shape {tuple(A.shape)}: need [{n}, C] with C <= {MAX_CHANNELS}")
        if A.shape[1] == 0:
            A = None
    c = 0 if A is None else A.shape[1]
    B, nbatch = None, 1
    if batch is not None:
        B = _to_device(batch, torch.int32, dev).reshape(-1)
        if B.shape[0] != n:
            raise ValueError(f"batch of {B.shape[0]} entries for {n} points")
        nbatch = _lib.PCC.BATCH_LIMIT + 1         # every index the voxel key can hold: no read of the largest one
    keys, vals, cap, scratch = _set_buffers(n, dev)
    m1 = max(n, 1)
    coords = torch.empty((m1, 4), dtype=torch.int32, device=dev)
    first = torch.empty(m1, dtype=torch.int32, device=dev)
    npts = torch.empty(m1, dtype=torch.int32, device=dev)
    sums = torch.empty((m1, max(c, 1)), dtype=torch.int64, device=dev)
    row = torch.empty(m1, dtype=torch.int32, device=dev)
    count, word = _host_count()
    check(_lib.lib().pcc_voxelize(ptr(P), ptr(B), n, nbatch, ptr(A) if c else None, c, origin[0], origin[1], origin[2], voxel_size,
                                  ROUNDINGS[rounding], ptr(keys), ptr(vals), cap, ptr(scratch), ptr(coords), ptr(first), ptr(npts),
                                  ptr(sums), ptr(row), ptr(count), _lib.stream()))
    try:
        m = _read_count(word, dev)
    except CoordinateRangeError:
        raise _range_error(P, A, B, nbatch, origin, voxel_size, ROUNDINGS[rounding]) from None
    coords, first, npts, row = coords[:m], first[:m], npts[:m], row[:n]
    if A is None:
        return Voxelized(coords, None, npts, row, first, None)
    sums = sums[:m]
    if reduce == "first":
        feats = A[first.long()]
    else:
        feats = (sums.to(torch.float64) / npts.to(torch.float64).unsqueeze(1) / Q32).to(torch.float32)
    return Voxelized(coords, feats, npts, row, first, sums)


def downsample(x, factor, rounding="floor"):
    """A codec cloud ``x`` [N,6] (xyz voxel coordinates + rgb in [0, 1]) on a grid ``factor`` times coarser, anchored at the
    origin: float32 [M,6] with xyz = the cell index (``floor(xyz / factor)``, or rounded to nearest with ``rounding="nearest"``)
    and rgb = the exact mean colour of the cell's points, voxels in order of first appearance — ready for ``compress``.  An
    8iVFB frame (10 bits) at ``factor`` 2 or 4 is the frame at 9 or 8 bits; ``factor`` 1 merges duplicate voxels and changes
    nothing else.  Unlike open3d's ``voxel_down_sample`` (the reference's RawLoader) the grid does not move with the cloud's
    bounding box and positions are cell indices, not centroids (see the module's docstring)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dim() != 2 or x.shape[1] < 6:
        raise ValueError(f"downsample: expected a [N, 6] cloud (xyz + rgb), got {tuple(x.shape)}")
    v = voxelize(x[:, :3], x[:, 3:6], voxel_size=factor, rounding=rounding)
    return torch.cat([v.coords[:, 1:].to(torch.float32), v.features], dim=1)
