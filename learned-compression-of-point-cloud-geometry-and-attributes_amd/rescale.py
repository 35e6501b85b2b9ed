"""Position scaling: lossy geometry the way a conventional coder makes it (G-PCC's positionQuantizationScale), with the colours
moved onto the quantised geometry ("recolouring").

A scale is a fraction s = num / den with 1 <= num <= den <= 255.  Per axis, in integers with floor division (the contract of
include/pcc_hip.h):

    cell(p) = floor((2 p num + den) / (2 den))        p s rounded to nearest, halves up
    pos(c)  = floor((2 c den + num) / (2 num))        c / s rounded to nearest, halves up

``quantize`` maps a cloud onto its distinct cells (``pcc_scaled_cells``: first-appearance order, exact Q32 attribute sums of each
cell's own points) and, with ``transfer="nearest"``, gives every cell the mean colour of the source points whose nearest
RECONSTRUCTED position ``pos(cell)`` it is (``pcc_scaled_transfer``, csrc/rescale.hip: a shell walk in the cell domain that stops
on an exact bound).  That is the association the D1 / colour metric makes from the source to the reconstruction, so this colouring
minimises the source -> reconstruction colour error among all colourings of the given geometry.  A cell that no point chose
(with s = 1/2 every odd coordinate lies exactly between two positions, and the tie rule sends it down) takes the colour of the
source point nearest to its position: the association the metric makes in the other direction.

G-PCC's own recolouring blends both directions with distance weights and search ranges that are encoder parameters; this one is
the exact minimiser of one direction with the other as the fallback, and is not meant to reproduce tmc3's colours.
"""
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .sparse import CoordMap, CoordinateRangeError, _host_count, _read_count, _require_cuda, _set_buffers

Scaled = namedtuple("Scaled", ["cells", "positions", "row", "first", "counts", "sums", "features", "nearest", "d2", "num", "den"])
Scaled.__doc__ = """cells int32 [M,4] (batch, cell x, y, z) in order of first appearance; positions int32 [M,3] = pos(cell) on the
original grid; row int32 [N] the own cell of every point; first int32 [M] lowest input row of every cell; counts int32 [M] and
sums int64 [M,C] (Q32) of the points that colour the cell; features float32 [M,C] (None without attributes); nearest int32 [N]
and d2 int64 [N] (transfer "nearest" only, else None): the cell row whose position is nearest to the point and the squared
distance in original voxels; num, den: the scale"""

SCALE_MAX = 255
MAX_CHANNELS = 16
COORD_LIMIT = _lib.PCC.COORD_LIMIT
Q32 = 4294967296.0
TRANSFERS = ("nearest", "cell")


def as_scale(scale):
    """-> (num, den) in lowest terms with 1 <= num <= den <= 255, from a ``(num, den)`` pair of integers, a
    ``fractions.Fraction`` or a float that IS such a fraction (0.125, 0.25, 0.5, 0.75 are; 0.3 is not).  ValueError otherwise."""
    if isinstance(scale, bool):
        raise ValueError(f"scale {scale!r}: a (num, den) pair, a Fraction or a float that is one exactly")
    try:
        if isinstance(scale, Fraction):
            f = scale
        elif isinstance(scale, (tuple, list)):
            if len(scale) != 2 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in scale):
                raise ValueError
            num, den = int(scale[0]), int(scale[1])
            if not 1 <= num <= den <= SCALE_MAX:
                raise ValueError
            f = Fraction(num, den)
        elif isinstance(scale, (float, int, np.floating, np.integer)):
            f = Fraction(float(scale))             # exact: every finite float is a dyadic fraction
        else:
            raise ValueError
    except (ValueError, OverflowError, ZeroDivisionError):
        raise ValueError(f"scale {scale!r}: a (num, den) pair with 1 <= num <= den <= {SCALE_MAX}, a Fraction or a float that is "
                         "such a fraction exactly") from None
    if not (0 < f <= 1 and f.denominator <= SCALE_MAX):
        raise ValueError(f"scale {scale!r}: not a fraction num / den with 1 <= num <= den <= {SCALE_MAX}")
    return f.numerator, f.denominator


def _floor_div(a, b):
    return torch.div(a, b, rounding_mode="floor") if torch.is_tensor(a) else a // b


def _as_int64(v):
    if torch.is_tensor(v):
        if v.dtype.is_floating_point or v.dtype == torch.bool:
            raise ValueError("the scale formulas are defined on integers")
        return v.to(torch.int64), v.dtype
    a = np.asarray(v)
    if a.dtype.kind not in "iu":
        raise ValueError("the scale formulas are defined on integers")
    return a.astype(np.int64), a.dtype


def cells_of(p, num, den):
    """cell(p) = floor((2 p num + den) / (2 den)) on an integer tensor or array, in its dtype"""
    v, dtype = _as_int64(p)
    out = _floor_div(2 * v * int(num) + int(den), 2 * int(den))
    return out.to(dtype) if torch.is_tensor(out) else out.astype(dtype)


def positions_of(c, num, den):
    """pos(c) = floor((2 c den + num) / (2 num)) on an integer tensor or array, in its dtype"""
    v, dtype = _as_int64(c)
    out = _floor_div(2 * v * int(den) + int(num), 2 * int(num))
    return out.to(dtype) if torch.is_tensor(out) else out.astype(dtype)


def to_q32(attributes):
    """float32 attributes -> int64 Q32 fixed point, ties to even: the kernels' llrint((double)a * 2**32)"""
    return torch.round(attributes.to(torch.float32).to(torch.float64) * Q32).to(torch.int64)


def _check_extent(coords, num, den):
    """the host-side range check, before a kernel runs: every source coordinate and every position it maps to within
    +-PCC_COORD_LIMIT (pos and cell are monotone, so the extremes decide).  One read of four numbers."""
    if coords.shape[0] == 0:
        return
    xyz = coords[:, 1:4]
    lo, hi, b_lo, b_hi = torch.stack([xyz.min(), xyz.max(), coords[:, 0].min(), coords[:, 0].max()]).tolist()
    if lo < -COORD_LIMIT or hi > COORD_LIMIT:
        raise CoordinateRangeError(f"rescale: source coordinates span {lo} .. {hi}, beyond +-{COORD_LIMIT} (PCC_COORD_LIMIT): "
                                   "translate the cloud towards the origin")
    ends = positions_of(cells_of(np.array([lo, hi], dtype=np.int64), num, den), num, den)
    if ends[0] < -COORD_LIMIT or ends[1] > COORD_LIMIT:
        raise CoordinateRangeError(f"rescale: at scale {num}/{den} the positions span {int(ends[0])} .. {int(ends[1])}, beyond "
                                   f"+-{COORD_LIMIT} (PCC_COORD_LIMIT): translate the cloud towards the origin")
    if b_lo < 0 or b_hi > _lib.PCC.BATCH_LIMIT:
        raise CoordinateRangeError(f"rescale: batch indices span {b_lo} .. {b_hi}, outside 0 .. {_lib.PCC.BATCH_LIMIT}")


def scaled_cells(coords, attributes, num, den):
    """``pcc_scaled_cells``: coords int32 [N,4] and attributes float32 [N,C] or None on the device ->
    (cells [M,4], first [M], npts [M], sums [M,C] or None, row [N], table (keys, vals, cap)).  One synchronisation: the count."""
    dev = coords.device
    n = coords.shape[0]
    c = 0 if attributes is None else attributes.shape[1]
    keys, vals, cap, scratch = _set_buffers(n, dev)
    m1 = max(n, 1)
    cells = torch.empty((m1, 4), dtype=torch.int32, device=dev)
    first = torch.empty(m1, dtype=torch.int32, device=dev)
    npts = torch.empty(m1, dtype=torch.int32, device=dev)
    sums = torch.empty((m1, max(c, 1)), dtype=torch.int64, device=dev)
    row = torch.empty(m1, dtype=torch.int32, device=dev)
    count, word = _host_count()
    check(_lib.lib().pcc_scaled_cells(ptr(coords), n, ptr(attributes) if c else None, c, num, den, ptr(keys), ptr(vals), cap, ptr(scratch),
                                      ptr(cells), ptr(first), ptr(npts), ptr(sums), ptr(row), ptr(count), _lib.stream()))
    try:
        m = _read_count(word, dev)
    except CoordinateRangeError:
        raise CoordinateRangeError("rescale: a coordinate or batch index is out of range, or an attribute is not finite or exceeds 1 "
                                   "in magnitude (attributes are fractions such as colour / 255)") from None
    return cells[:m], first[:m], npts[:m], (sums[:m] if c else None), row[:n], (keys, vals, cap)


def scaled_transfer(coords, attributes, num, den, table, m):
    """``pcc_scaled_transfer`` over the table of the points' own cell set (m rows) -> (nearest int32 [N], d2 int64 [N],
    npts int32 [M], sums int64 [M,C] or None).  No synchronisation."""
    dev = coords.device
    n = coords.shape[0]
    c = 0 if attributes is None else attributes.shape[1]
    keys, vals, cap = table
    nearest = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    d2 = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    npts = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    sums = torch.empty((max(m, 1), max(c, 1)), dtype=torch.int64, device=dev)
    check(_lib.lib().pcc_scaled_transfer(ptr(coords), n, ptr(attributes) if c else None, c, num, den, ptr(keys), ptr(vals), cap, m,
                                         ptr(nearest), ptr(d2), ptr(npts), ptr(sums), _lib.stream()))
    return nearest[:n], d2[:n], npts[:m], (sums[:m] if c else None)


def quantize_coords(coords, attributes, scale, transfer="nearest"):
    """``quantize`` on integer rows: coords int32 [N,4] (batch, x, y, z) and attributes float32 [N,C] (C <= 16, values in
    [-1, 1]) or None, both on the device -> ``Scaled``.  Cells of two batch items never merge, and a point is only ever
    associated with a cell of its own item."""
    from .metrics import nearest_neighbours
    if transfer not in TRANSFERS:
        raise ValueError(f"transfer {transfer!r}: 'nearest' or 'cell'")
    num, den = as_scale(scale)
    _require_cuda(coords)
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 4:
        raise ValueError(f"rescale: coordinates are int32 [N, 4] rows (batch, x, y, z), got {coords.dtype} {tuple(coords.shape)}")
    coords = coords.contiguous()
    n = coords.shape[0]
    A = None
    if attributes is not None and not (attributes.dim() == 2 and attributes.shape[1] == 0):
        if attributes.dim() != 2 or attributes.shape[0] != n or attributes.shape[1] > MAX_CHANNELS:
            raise ValueError(f"rescale: attributes of shape {tuple(attributes.shape)}: need [{n}, C] with C <= {MAX_CHANNELS}")
        A = attributes.detach().to(device=coords.device, dtype=torch.float32).contiguous()
    _check_extent(coords, num, den)
    cells, first, npts, sums, row, table = scaled_cells(coords, A, num, den)
    m = cells.shape[0]
    positions = positions_of(cells[:, 1:4], num, den).contiguous()
    nearest = d2 = None
    if transfer == "nearest" and n:
        nearest, d2, npts, sums = scaled_transfer(coords, A, num, den, table, m)
        empty = torch.nonzero(npts == 0).flatten()
        if A is not None and empty.numel():
            # a cell no point chose takes the colour of the source point nearest to its position (the metric's B -> A association)
            query = torch.cat([cells[empty, :1], positions[empty]], dim=1).contiguous()
            idx, _, _, _ = nearest_neighbours(query, CoordMap(coords, 1))
            sums[empty] = to_q32(A[idx.long()])
    elif transfer == "nearest":
        nearest, d2 = torch.empty(0, dtype=torch.int32, device=coords.device), torch.empty(0, dtype=torch.int64, device=coords.device)
    feats = None
    if A is not None:
        feats = (sums.to(torch.float64) / torch.clamp(npts, min=1).to(torch.float64).unsqueeze(1) / Q32).to(torch.float32)
    return Scaled(cells, positions, row, first, npts, sums, feats, nearest, d2, num, den)


def quantize(x, scale, transfer="nearest"):
    """A cloud ``x`` [N, 3+C] on the GPU (integer voxel coordinates as floats, attributes in [0, 1], C <= 16) quantised by
    ``scale`` (what ``as_scale`` takes) -> ``Scaled``: the distinct cells in order of first appearance, their positions on the
    original grid and their colours.

    ``transfer="cell"``: ``features`` are the exact means of each cell's own points.  ``transfer="nearest"`` (the default): a
    cell's colour is the exact mean over the points whose nearest reconstructed position it is (ties to the smallest (x, y, z));
    a cell that no point chose takes the colour of the source point nearest to its position (``counts`` stays 0 there, and
    ``features`` divides by max(count, 1)).  Means are ``float32(float64(sum) / float64(count) / 2**32)`` of exact integer sums:
    bitwise reproducible.  ValueError (before a kernel runs) when a source coordinate, or a position it maps to, lies beyond
    +-PCC_COORD_LIMIT; ValueError when an attribute is not finite or exceeds 1 in magnitude."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("rescale.quantize: the cloud must live on the GPU; there is no CPU path")
    if x.dim() != 2 or x.shape[1] < 3 or x.shape[1] > 3 + MAX_CHANNELS:
        raise ValueError(f"rescale.quantize: expected a [N, 3 + C] cloud with C <= {MAX_CHANNELS}, got {tuple(x.shape)}")
    xyz = x[:, :3]
    if not x.dtype.is_floating_point:
        xyz = xyz.to(torch.float64)
    if not bool(torch.isfinite(xyz).all()):
        raise CoordinateRangeError("rescale.quantize: a coordinate is not finite")
    xyz = torch.round(xyz).clamp(-2.0 ** 30, 2.0 ** 30).to(torch.int32)
    coords = torch.cat([torch.zeros_like(xyz[:, :1]), xyz], dim=1).contiguous()
    return quantize_coords(coords, x[:, 3:] if x.shape[1] > 3 else None, scale, transfer)
