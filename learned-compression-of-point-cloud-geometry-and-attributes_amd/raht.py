"""RAHT (region-adaptive hierarchical transform, de Queiroz & Chou 2016) of per-voxel attributes and its coefficient stream
"PCR1": the attribute half of the octree + RAHT anchor codec (anchor.py), the transform G-PCC's attribute coder uses.

Device (csrc/raht.hip; the arithmetic is specified in include/pcc_hip.h): Morton keys, radix sort, the closed-form plan (per row
the one step at which it receives its coefficient, its partner row and the two weights), the rows bucketed by step, and the
transform itself, one launch per step in float64 without atomics.  Host: quantisation to integer symbols, the choice of one of
the 64 Gaussian tables per (step, channel) context, and the range coder shared with the latents.

RAHT here is open-loop transform coding: the decoder needs the integer symbols and the geometry, nothing else, so encoder and
decoder never have to agree on a float.

Stream (little-endian):
    "PCR1" | u8 depth | u8 C | u16 0 | f64 qstep | u32 n | i64 dc[C] | u8 table[3 * depth * C] | u32 payload_len | payload
Symbols are rint(coefficient / qstep), ties to even.  The DC row's go into the header; the n - 1 high-pass rows are coded
channel-major, rows ascending, the context of a symbol being (step of its row, channel) and ``table[step * C + channel]`` the
one of the 64 tables of ``GaussianConditional(get_scale_table())`` that codes the context's symbols shortest (symbols outside
a table go through the coder's escape).
"""
import functools
import struct

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .entropy import GaussianConditional, _rans_decode, _rans_encode, get_scale_table

MAGIC = b"PCR1"
MAX_CHANNELS = 16
MAX_DEPTH = 17                    # 2^17 > PCC_COORD_LIMIT
SYMBOL_LIMIT = 1 << 28            # |symbol| below this: the coder's escape carries 32 bits
_HEAD = struct.Struct("<4sBBHdI")
_COST_SCALE = 1 << 20             # code lengths are compared in units of 2^-20 bit, as integers: no sum depends on its order


class Plan:
    """What ``plan`` returns: ``n`` rows, ``depth``, ``origin`` (three ints), and on the device the int32 arrays ``perm`` (input
    row of every Morton row), ``step``, ``left``, ``w0``, ``w1`` (per row) and ``step_rows``; ``step_offsets`` is a host int32
    array of 3 * depth + 1 entries."""

    def __init__(self, n, depth, origin, perm, step, left, w0, w1, step_rows, step_offsets):
        self.n, self.depth, self.origin = n, depth, origin
        self.perm, self.step, self.left, self.w0, self.w1, self.step_rows = perm, step, left, w0, w1, step_rows
        self.step_offsets = step_offsets
        self._step_host = None

    @property
    def device(self):
        return self.perm.device

    def step_host(self):
        """``step`` as a host int64 array (read once)"""
        if self._step_host is None:
            self._step_host = self.step.cpu().numpy().astype(np.int64)
        return self._step_host


def plan(coords, origin=None, depth=None):
    """coords: int [N,4] (batch, x, y, z; one cloud, batch ignored) or [N,3], on the GPU, N >= 1, no voxel twice -> ``Plan``.
    ``origin`` / ``depth`` default to the rule of ``octree.encode_coordinates``: the per-axis minimum, and the bit length of the
    largest extent.  Raises ValueError when a voxel lies outside [origin, origin + 2^depth)^3 or occurs twice."""
    L = _lib.lib()
    if not isinstance(coords, torch.Tensor) or coords.device.type != "cuda":
        raise RuntimeError("raht.plan: coordinates must live on the GPU; there is no CPU path")
    if coords.dim() != 2 or coords.shape[1] not in (3, 4) or coords.shape[0] < 1:
        raise ValueError(f"raht.plan: coordinates of shape {tuple(coords.shape)}: need [N, 4] or [N, 3] with N >= 1")
    coords = coords.to(torch.int32)
    if coords.shape[1] == 3:
        coords = torch.cat([torch.zeros_like(coords[:, :1]), coords], dim=1)
    coords = coords.contiguous()
    n, dev = int(coords.shape[0]), coords.device
    if origin is None or depth is None:
        lohi = torch.cat([coords[:, 1:4].amin(dim=0), coords[:, 1:4].amax(dim=0)]).cpu().numpy().astype(np.int64)
        if origin is None:
            origin = lohi[:3]
        if depth is None:
            depth = int((lohi[3:] - np.asarray(origin, dtype=np.int64)).max()).bit_length() if n else 0
    depth = int(depth)
    if not 0 <= depth <= MAX_DEPTH:
        raise ValueError(f"raht.plan: depth {depth} outside 0..{MAX_DEPTH}")
    origin_h = np.ascontiguousarray(np.asarray(origin, dtype=np.int64).reshape(3), dtype=np.int32)
    rows = torch.empty((6, n), dtype=torch.int32, device=dev)          # perm, step, left, w0, w1, step_rows
    words = torch.empty(3 * depth + 1 + 2, dtype=torch.int32, device=dev)      # step_offsets, then status
    nbytes = L.pcc_raht_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.pcc_raht_plan(ptr(coords), n, ptr(origin_h), depth, ptr(rows[0]), ptr(rows[1]), ptr(rows[2]), ptr(rows[3]), ptr(rows[4]),
                          ptr(rows[5]), ptr(words), ptr(words[3 * depth + 1:]), ptr(scratch), nbytes, _lib.stream()))
    host = words.cpu().numpy()
    outside, twice = int(host[-2]), int(host[-1])
    if outside:
        raise ValueError(f"raht.plan: {outside} voxels lie outside the grid of {depth} bits per axis at origin {origin_h.tolist()}")
    if twice:
        raise ValueError(f"raht.plan: duplicate voxels ({n - twice} distinct of {n}); merge them first (pcc_amd.voxelize)")
    return Plan(n, depth, tuple(int(v) for v in origin_h), rows[0], rows[1], rows[2], rows[3], rows[4], rows[5],
                np.ascontiguousarray(host[:3 * depth + 1], dtype=np.int32))


def _transform(p, values, inverse):
    c = int(values.shape[1])
    check(_lib.lib().pcc_raht_transform(ptr(values), p.n, c, ptr(p.left), ptr(p.w0), ptr(p.w1), ptr(p.step_rows), ptr(p.step_offsets),
                                        p.depth, int(inverse), _lib.stream()))
    return values


def _rows_of(p, t, what):
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.dim() != 2 or t.shape[0] != p.n or not 1 <= t.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"raht: {what} of shape {tuple(t.shape)}: need [{p.n}, C] with 1 <= C <= {MAX_CHANNELS}")
    return t.to(device=p.device, dtype=torch.float64)


def forward(p, attrs):
    """attrs [N,C] in the order of the coordinates the plan was made of -> float64 [N,C] coefficients in Morton row order: row 0
    the DC, every other row one high-pass coefficient"""
    a = _rows_of(p, attrs, "attributes")
    return _transform(p, a.index_select(0, p.perm.long()).contiguous(), 0)        # (index_select copies: the input stays)


def inverse(p, coeffs):
    """coefficients [N,C] in Morton row order -> float64 [N,C] attributes in Morton row order (row i belongs to input row
    ``perm[i]``)"""
    return _transform(p, _rows_of(p, coeffs, "coefficients").clone().contiguous(), 1)


@functools.lru_cache(maxsize=1)
def gaussian_tables():
    """-> (cdf [64, L], cdf_length [64], offset [64]) int32 host arrays: the tables ``GaussianConditional`` builds from
    ``get_scale_table()``, which every codec of this package shares"""
    gc = GaussianConditional(get_scale_table())
    gc.update()
    return gc.tables()


@functools.lru_cache(maxsize=1)
def _table_costs():
    """-> (bits [64, L - 1] int64, maxv [64], offset [64]): the code length of every table's bins in units of 2^-20 bit; bin
    ``maxv[t]`` is the table's tail (escape) bin"""
    cdf, cdf_len, off = gaussian_tables()
    freq = np.diff(cdf.astype(np.int64), axis=1)
    bits = np.zeros(freq.shape, dtype=np.int64)
    ok = freq > 0
    bits[ok] = np.rint((16.0 - np.log2(freq[ok].astype(np.float64))) * _COST_SCALE).astype(np.int64)
    return bits, cdf_len.astype(np.int64) - 2, off.astype(np.int64)


def symbol_costs(values):
    """int64 symbol values [U] -> int64 [64, U]: what each of the 64 tables spends on each value, in units of 2^-20 bit.  A value
    outside a table costs the tail bin plus the coder's bypass: 4 bits per nibble of the folded remainder, and 4 bits per
    started group of 15 nibbles for their count (csrc/rans_host.cpp)."""
    bits, maxv, off = _table_costs()
    v = np.asarray(values, dtype=np.int64)[None, :] - off[:, None]
    inside = (v >= 0) & (v < maxv[:, None])
    cost = np.take_along_axis(bits, np.where(inside, v, maxv[:, None]), axis=1)
    raw = np.where(v < 0, -2 * v - 1, 2 * (v - maxv[:, None]))
    raw = np.where(inside, 0, raw)
    nibbles = np.zeros(raw.shape, dtype=np.int64)
    for k in range(16):
        nibbles += (raw >> (4 * k)) != 0
    return cost + np.where(inside, 0, 4 * nibbles + 4 * (nibbles // 15 + 1)) * _COST_SCALE


def choose_tables(symbols, contexts, n_contexts):
    """symbols, contexts: int arrays of one length -> uint8 [n_contexts]: per context the table (of the 64) with the smallest
    ideal code length of the context's symbols, the lowest index on ties, 0 for a context without symbols"""
    symbols = np.asarray(symbols, dtype=np.int64).reshape(-1)
    contexts = np.asarray(contexts, dtype=np.int64).reshape(-1)
    table = np.zeros(n_contexts, dtype=np.uint8)
    if symbols.size == 0:
        return table
    values, which = np.unique(symbols, return_inverse=True)
    costs = symbol_costs(values)                                     # [64, U]
    order = np.argsort(contexts, kind="stable")
    bounds = np.searchsorted(contexts[order], np.arange(n_contexts + 1))
    for ctx in range(n_contexts):
        rows = order[bounds[ctx]:bounds[ctx + 1]]
        if rows.size:
            hist = np.bincount(which[rows], minlength=values.size)
            used = np.flatnonzero(hist)
            table[ctx] = int(np.argmin(costs[:, used] @ hist[used]))
    return table


def quantize(coeffs, qstep):
    """float64 coefficients -> int64 symbols rint(coeff / qstep), ties to even (a tensor divisor: torch turns x / python_float
    into a multiplication by the reciprocal)"""
    return torch.round(coeffs / torch.tensor(float(qstep), dtype=torch.float64, device=coeffs.device)).to(torch.int64)


def _check_qstep(qstep):
    qstep = float(qstep)
    if not (qstep > 0.0 and np.isfinite(qstep)):
        raise ValueError(f"raht: qstep {qstep}: a positive finite number")
    return qstep


def _stream_indexes(p, table, c):
    """the table index of every coded symbol, in stream order (channel-major over rows 1 .. n-1)"""
    step = p.step_host()[1:]
    return table.astype(np.int32).reshape(3 * p.depth, c)[step].T.reshape(-1) if p.n > 1 else np.zeros(0, dtype=np.int32)


def encode_symbols(p, symbols):
    """int64 host symbols [N,C] in Morton row order -> the PCR1 stream behind its qstep-bearing head: dc, tables, payload"""
    n, c = symbols.shape
    if np.abs(symbols[1:]).max(initial=0) >= SYMBOL_LIMIT:
        raise ValueError(f"raht: a symbol of magnitude {int(np.abs(symbols[1:]).max())}: qstep is too small for these attributes")
    high = np.ascontiguousarray(symbols[1:].T)                       # [C, N-1]: channel-major, rows ascending
    step = p.step_host()[1:]
    contexts = (step[None, :] * c + np.arange(c, dtype=np.int64)[:, None]).reshape(-1)
    table = choose_tables(high.reshape(-1), contexts, 3 * p.depth * c)
    payload = b""
    if high.size:
        cdf, cdf_len, off = gaussian_tables()
        payload = _rans_encode(high.reshape(-1).astype(np.int32), _stream_indexes(p, table, c), cdf, cdf_len, off)
    return struct.pack("<%dq" % c, *[int(v) for v in symbols[0]]) + table.tobytes() + struct.pack("<I", len(payload)) + payload


def encode_attributes(p, attrs, qstep, return_symbols=False):
    """attrs [N,C] (rows as the plan's coordinates) -> PCR1 bytes; with ``return_symbols`` also the int64 host symbols [N,C] in
    Morton row order"""
    qstep = _check_qstep(qstep)
    sym = quantize(forward(p, attrs), qstep).cpu().numpy()
    data = _HEAD.pack(MAGIC, p.depth, sym.shape[1], 0, qstep, p.n) + encode_symbols(p, sym)
    return (data, sym) if return_symbols else data


def decode_symbols(p, data):
    """PCR1 bytes -> (int64 host symbols [N,C] in Morton row order, qstep); ValueError for a stream that is not one, is cut short
    or was not made for this plan"""
    data = bytes(data)
    if len(data) < _HEAD.size or data[:4] != MAGIC:
        raise ValueError("not a PCR1 attribute stream")
    _, depth, c, _, qstep, n = _HEAD.unpack(data[:_HEAD.size])
    if (depth, n) != (p.depth, p.n):
        raise ValueError(f"PCR1: the stream holds {n} rows at depth {depth}, the plan {p.n} at depth {p.depth}")
    if not 1 <= c <= MAX_CHANNELS or not (qstep > 0.0 and np.isfinite(qstep)):
        raise ValueError("PCR1: bad header")
    pos, ntab = _HEAD.size, 3 * depth * c
    if len(data) < pos + 8 * c + ntab + 4:
        raise ValueError("PCR1: truncated header")
    sym = np.empty((n, c), dtype=np.int64)
    sym[0] = struct.unpack("<%dq" % c, data[pos:pos + 8 * c])
    pos += 8 * c
    table = np.frombuffer(data, dtype=np.uint8, count=ntab, offset=pos)
    pos += ntab
    if ntab and int(table.max()) >= 64:
        raise ValueError("PCR1: table index out of range")
    (plen,) = struct.unpack("<I", data[pos:pos + 4])
    pos += 4
    payload = data[pos:pos + plen]
    if len(payload) != plen:
        raise ValueError("PCR1: truncated payload")
    if n > 1:
        cdf, cdf_len, off = gaussian_tables()
        try:
            high = _rans_decode(payload, _stream_indexes(p, table, c), cdf, cdf_len, off)
        except _lib.PccError as e:
            raise ValueError(f"PCR1: corrupt payload ({e})") from None
        sym[1:] = high.reshape(c, n - 1).T
    return sym, float(qstep)


def decode_attributes(p, data, channels=None):
    """PCR1 bytes -> float64 [N,C] attributes in Morton row order: symbols times qstep through the inverse transform.
    ``channels``: the C the caller expects (ValueError when the stream holds another)"""
    sym, qstep = decode_symbols(p, data)
    if channels is not None and sym.shape[1] != int(channels):
        raise ValueError(f"PCR1: the stream holds {sym.shape[1]} channels, expected {int(channels)}")
    coeffs = torch.from_numpy(sym).to(p.device).to(torch.float64) * qstep
    return _transform(p, coeffs.contiguous(), 1)
