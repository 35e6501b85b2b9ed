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

Region-wise quantisation, "PCR2" (``encode_attributes(..., levels=...)``): every point carries a quantisation LEVEL 0 .. 63, level
l quantising with ``level_steps(qstep)[l]``, one Gaussian-table spacing per level.  The rows inside one cube of edge
2^block_log2 form a block (in Morton row order: a row opens a block iff it is row 0 or its step is >= 3 * block_log2, so the plan
alone gives the boundaries), a block takes the MINIMUM of its points' levels, and the coefficient of row i, which summarises the
rows [left[i], i + w1[i]), the minimum level among them (include/pcc_hip.h states the walk that computes it).  Blocks, block
levels, coefficient levels, quantisation and dequantisation run on the device; the stream carries the block levels only.
    "PCR2" | u8 depth | u8 C | u8 block_log2 | u8 0 | f64 qstep | u32 n | u32 n_blocks | u8 level_table | u32 levels_len
           | levels payload | i64 dc[C] | u8 table[3 * depth * C] | u32 payload_len | payload
The levels payload is level[0], level[1] - level[0], ... in block order, range coded with the one table ``level_table`` that
codes it shortest.  The DC symbols are rint(dc / step[coeff_level[0]]); coeff_level[0] is the smallest level of the cloud,
``level_min``.  The high-pass symbols are coded as in PCR1, but the table of a symbol is
clip(table[context] - (coeff_level[row] - level_min), 0, 63): a level coarser divides the symbols by one table spacing, so the
neighbouring table fits them, and no table bytes are spent on levels.  ``table[context]`` is chosen under that rule.
"""
import functools
import struct

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .entropy import SCALES_MAX, SCALES_MIN, GaussianConditional, _rans_decode, _rans_encode, get_scale_table

MAGIC = b"PCR1"
MAGIC_REGION = b"PCR2"
LEVELS = 64                       # quantisation levels of PCR2, one per Gaussian table
MAX_BLOCK_LOG2 = 17
MAX_CHANNELS = 16
MAX_DEPTH = 17                    # 2^17 > PCC_COORD_LIMIT
SYMBOL_LIMIT = 1 << 28            # |symbol| below this: the coder's escape carries 32 bits
_HEAD = struct.Struct("<4sBBHdI")
_HEAD_REGION = struct.Struct("<4sBBBBdIIBI")
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


def choose_tables(symbols, contexts, n_contexts, shift=None):
    """symbols, contexts: int arrays of one length -> uint8 [n_contexts]: per context the table (of the 64) with the smallest
    ideal code length of the context's symbols, the lowest index on ties, 0 for a context without symbols.

    ``shift`` (int array of the same length, every entry >= 0): a symbol with shift h is coded with table clip(t - h, 0, 63)
    when its context chooses t, and t is chosen under that rule (PCR2)."""
    symbols = np.asarray(symbols, dtype=np.int64).reshape(-1)
    contexts = np.asarray(contexts, dtype=np.int64).reshape(-1)
    table = np.zeros(n_contexts, dtype=np.uint8)
    if symbols.size == 0:
        return table
    values, which = np.unique(symbols, return_inverse=True)
    costs = symbol_costs(values)                                     # [64, U]
    if shift is not None:
        return _choose_tables_shifted(which, contexts, n_contexts, np.asarray(shift, dtype=np.int64).reshape(-1), costs)
    order = np.argsort(contexts, kind="stable")
    bounds = np.searchsorted(contexts[order], np.arange(n_contexts + 1))
    for ctx in range(n_contexts):
        rows = order[bounds[ctx]:bounds[ctx + 1]]
        if rows.size:
            hist = np.bincount(which[rows], minlength=values.size)
            used = np.flatnonzero(hist)
            table[ctx] = int(np.argmin(costs[:, used] @ hist[used]))
    return table


def _choose_tables_shifted(which, contexts, n_contexts, shift, costs):
    """``choose_tables`` with a per-symbol shift: the symbols of one (context, shift) group cost g[t'] under table t', and the
    group adds g[clip(t - shift, 0, 63)] to what table t costs its context"""
    if shift.shape != which.shape or int(shift.min()) < 0:
        raise ValueError("raht.choose_tables: shift needs one non-negative entry per symbol")
    n_tables = costs.shape[0]
    shift = np.minimum(shift, n_tables - 1)                          # (a larger shift clips to table 0 all the same)
    group = contexts * n_tables + shift
    order = np.argsort(group, kind="stable")
    ids, starts = np.unique(group[order], return_index=True)
    ends = np.append(starts[1:], order.size)
    total = np.zeros((n_contexts, n_tables), dtype=np.int64)
    t = np.arange(n_tables)
    for gid, lo, hi in zip(ids.tolist(), starts.tolist(), ends.tolist()):
        used, count = np.unique(which[order[lo:hi]], return_counts=True)
        g = costs[:, used] @ count
        total[gid // n_tables] += g[np.clip(t - gid % n_tables, 0, n_tables - 1)]
    return np.argmin(total, axis=1).astype(np.uint8)                 # (the lowest index on ties; 0 for a context of zeros)


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


def encode_attributes(p, attrs, qstep, return_symbols=False, levels=None, block_log2=3):
    """attrs [N,C] (rows as the plan's coordinates) -> PCR1 bytes; with ``return_symbols`` also the int64 host symbols [N,C] in
    Morton row order.

    ``levels`` (uint8 [N], 0 .. 63, rows as the plan's coordinates; ``quality_levels`` makes them from a quality map): PCR2
    bytes, every cube of edge 2^block_log2 quantised with ``level_steps(qstep)`` at the smallest level among its points"""
    qstep = _check_qstep(qstep)
    if levels is not None:
        return encode_region(p, forward(p, attrs), qstep, region(p, levels, block_log2), return_symbols=return_symbols)
    return encode_coefficients(p, forward(p, attrs), qstep, return_symbols=return_symbols)


def encode_coefficients(p, coeffs, qstep, return_symbols=False):
    """float64 [N,C] coefficients (device, Morton row order) -> PCR1 bytes at ``qstep``: what ``encode_attributes`` does behind
    the transform, for callers that code one set of coefficients at several steps"""
    qstep = _check_qstep(qstep)
    sym = quantize(coeffs, qstep).cpu().numpy()
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
    """PCR1 or PCR2 bytes -> float64 [N,C] attributes in Morton row order: symbols times their step through the inverse
    transform.  ``channels``: the C the caller expects (ValueError when the stream holds another)"""
    if bytes(data[:4]) == MAGIC_REGION:
        sym, qstep, reg = decode_region(p, data)
        name = "PCR2"
    else:
        sym, qstep = decode_symbols(p, data)
        name = "PCR1"
    if channels is not None and sym.shape[1] != int(channels):
        raise ValueError(f"{name}: the stream holds {sym.shape[1]} channels, expected {int(channels)}")
    if name == "PCR2":
        coeffs = dequantize_levels(torch.from_numpy(sym.astype(np.int32)).to(p.device), reg.coeff_level, level_steps(qstep))
    else:
        coeffs = torch.from_numpy(sym).to(p.device).to(torch.float64) * qstep
    return _transform(p, coeffs.contiguous(), 1)


# ---- region-wise quantisation: PCR2 -------------------------------------------------------------------------------------------
def level_steps(qstep):
    """-> float64 [64]: the quantisation step of every level, ``qstep * (SCALES_MAX / SCALES_MIN) ** (l / 63)``.  Level 0 is
    ``qstep`` exactly; one level is one spacing of the 64 log-spaced Gaussian tables, so a level coarser moves a context's
    symbols to the neighbouring table"""
    return np.float64(_check_qstep(qstep)) * np.float64(SCALES_MAX / SCALES_MIN) ** (np.arange(LEVELS, dtype=np.float64) / (LEVELS - 1))


def quality_levels(q, span=24):
    """quality in [0, 1] (array or tensor, any shape) -> uint8 levels of the same shape: ``rint((1 - clip(q, 0, 1)) * span)``,
    ties to even, with 0 <= span <= 63.  Quality 1 codes at ``qstep``, quality 0 at ``level_steps(qstep)[span]``: about 19
    times ``qstep`` for the default span, which is a starting value and has not been tuned."""
    span = int(span)
    if not 0 <= span <= LEVELS - 1:
        raise ValueError(f"raht.quality_levels: span {span} outside 0..{LEVELS - 1}")
    if isinstance(q, torch.Tensor):
        return torch.round((1.0 - torch.clamp(q.to(torch.float64), 0.0, 1.0)) * span).to(torch.uint8)
    return np.rint((1.0 - np.clip(np.asarray(q, dtype=np.float64), 0.0, 1.0)) * span).astype(np.uint8)


class Region:
    """What ``region`` returns: ``block_log2``, ``n_blocks``, and on the device ``block_of_row`` (int32 [N]), ``block_level``
    (int32 [n_blocks]) and ``coeff_level`` (uint8 [N], Morton row order)"""

    def __init__(self, block_log2, n_blocks, block_of_row, block_level, coeff_level):
        self.block_log2, self.n_blocks = block_log2, n_blocks
        self.block_of_row, self.block_level, self.coeff_level = block_of_row, block_level, coeff_level
        self._host = None

    def host(self):
        """-> (block_level int64 [n_blocks], coeff_level int64 [N]) on the host (read once)"""
        if self._host is None:
            self._host = (self.block_level.cpu().numpy().astype(np.int64), self.coeff_level.cpu().numpy().astype(np.int64))
        return self._host


def blocks(p, block_log2=3):
    """-> (block_of_row int32 [N] on the device, n_blocks): the cubes of edge 2^block_log2 as runs of Morton rows"""
    block_log2 = int(block_log2)
    if not 0 <= block_log2 <= MAX_BLOCK_LOG2:
        raise ValueError(f"raht.blocks: block_log2 {block_log2} outside 0..{MAX_BLOCK_LOG2}")
    L = _lib.lib()
    block_of_row = torch.empty(p.n, dtype=torch.int32, device=p.device)
    count = torch.empty(1, dtype=torch.int32, device=p.device)
    nbytes = L.pcc_raht_scratch_bytes(p.n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    check(L.pcc_raht_blocks(ptr(p.step), p.n, block_log2, ptr(block_of_row), ptr(count), ptr(scratch), nbytes, _lib.stream()))
    return block_of_row, int(count.item())


def block_levels(p, levels, block_of_row, n_blocks):
    """levels [N] (0 .. 63, rows as the plan's coordinates) -> int32 [n_blocks] on the device: the smallest level of every
    block.  ValueError for a level outside 0 .. 63."""
    t = levels if isinstance(levels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(levels))
    if t.numel() != p.n or t.dim() > 2 or t.is_floating_point():
        raise ValueError(f"raht: levels of shape {tuple(t.shape)} and type {t.dtype}: need {p.n} integers")
    t = t.reshape(-1).to(p.device)
    if t.dtype != torch.uint8:
        t = torch.where((t < 0) | (t >= LEVELS), 255, t).to(torch.uint8)         # (the kernel counts them)
    t = t.contiguous()
    out = torch.empty(n_blocks, dtype=torch.int32, device=p.device)
    status = torch.empty(1, dtype=torch.int32, device=p.device)
    check(_lib.lib().pcc_raht_block_levels(ptr(t), ptr(p.perm), ptr(block_of_row), p.n, n_blocks, ptr(out), ptr(status), _lib.stream()))
    bad = int(status.item())
    if bad:
        raise ValueError(f"raht: {bad} levels outside 0..{LEVELS - 1}")
    return out


def coeff_levels(p, block_level, block_of_row):
    """block levels int32 [n_blocks] (device) -> uint8 [N] on the device: the level of every row's coefficient, the smallest
    block level among the rows the coefficient summarises; row 0 (the DC) gets the smallest of the cloud"""
    out = torch.empty(p.n, dtype=torch.uint8, device=p.device)
    lev = torch.empty(p.n, dtype=torch.int32, device=p.device)
    check(_lib.lib().pcc_raht_coeff_levels(ptr(block_level), ptr(block_of_row), p.n, int(block_level.numel()), ptr(p.left), ptr(p.step_rows),
                                           ptr(p.step_offsets), p.depth, ptr(out), ptr(lev), _lib.stream()))
    return out


def region(p, levels, block_log2=3):
    """per-point levels (rows as the plan's coordinates) -> ``Region``: blocks, block levels and coefficient levels, all made on
    the device.  It depends on the plan and the levels only, so one ``Region`` serves every qstep."""
    block_of_row, n_blocks = blocks(p, block_log2)
    block_level = block_levels(p, levels, block_of_row, n_blocks)
    return Region(int(block_log2), n_blocks, block_of_row, block_level, coeff_levels(p, block_level, block_of_row))


def quantize_levels(coeffs, coeff_level, steps):
    """float64 [N,C] coefficients, uint8 [N] levels (device), float64 [64] steps (host) -> int32 [N,C] symbols
    rint(coeff / steps[level]) on the device; ValueError when one reaches 2^28"""
    coeffs = coeffs.contiguous()
    n, c = coeffs.shape
    steps = np.ascontiguousarray(steps, dtype=np.float64).reshape(LEVELS)
    out = torch.empty((n, c), dtype=torch.int32, device=coeffs.device)
    status = torch.empty(1, dtype=torch.int32, device=coeffs.device)
    check(_lib.lib().pcc_raht_quantize(ptr(coeffs), n, c, ptr(coeff_level), ptr(steps), ptr(out), ptr(status), _lib.stream()))
    bad = int(status.item())
    if bad:
        raise ValueError(f"raht: {bad} symbols of magnitude 2^28 or more: qstep is too small for these attributes")
    return out


def dequantize_levels(symbols, coeff_level, steps):
    """int32 [N,C] symbols, uint8 [N] levels (device), float64 [64] steps (host) -> float64 [N,C] symbol * steps[level]"""
    symbols = symbols.contiguous()
    n, c = symbols.shape
    steps = np.ascontiguousarray(steps, dtype=np.float64).reshape(LEVELS)
    out = torch.empty((n, c), dtype=torch.float64, device=symbols.device)
    check(_lib.lib().pcc_raht_dequantize(ptr(symbols), n, c, ptr(coeff_level), ptr(steps), ptr(out), _lib.stream()))
    return out


def _region_indexes(p, table, c, coeff_level):
    """the table index of every coded symbol of a PCR2 stream, in stream order: the context's table lowered by the row's level
    above the smallest (host ``coeff_level`` int64 [N])"""
    if p.n <= 1:
        return np.zeros(0, dtype=np.int32)
    base = table.astype(np.int64).reshape(3 * p.depth, c)[p.step_host()[1:]]
    return np.clip(base - (coeff_level[1:] - coeff_level[0])[:, None], 0, LEVELS - 1).T.reshape(-1).astype(np.int32)


def encode_level_deltas(block_level):
    """host block levels [n_blocks] -> (table, payload): level[0], level[1] - level[0], ... range coded with the one Gaussian
    table that codes them shortest"""
    deltas = np.diff(np.asarray(block_level, dtype=np.int64), prepend=0)
    table = int(choose_tables(deltas, np.zeros(deltas.size, dtype=np.int64), 1)[0])
    cdf, cdf_len, off = gaussian_tables()
    return table, _rans_encode(deltas.astype(np.int32), np.full(deltas.size, table, dtype=np.int32), cdf, cdf_len, off)


def encode_region_symbols(p, symbols, reg):
    """int64 host symbols [N,C] in Morton row order, their ``Region`` -> the PCR2 stream behind its fixed head: block levels,
    dc, tables, payload"""
    n, c = symbols.shape
    block_level, coeff_level = reg.host()
    level_table, level_bytes = encode_level_deltas(block_level)
    high = np.ascontiguousarray(symbols[1:].T)                       # [C, N-1]: channel-major, rows ascending
    step = p.step_host()[1:]
    contexts = (step[None, :] * c + np.arange(c, dtype=np.int64)[:, None]).reshape(-1)
    shift = np.broadcast_to(coeff_level[1:] - coeff_level[0], high.shape).reshape(-1)
    table = choose_tables(high.reshape(-1), contexts, 3 * p.depth * c, shift=shift)
    payload = b""
    if high.size:
        cdf, cdf_len, off = gaussian_tables()
        payload = _rans_encode(high.reshape(-1).astype(np.int32), _region_indexes(p, table, c, coeff_level), cdf, cdf_len, off)
    return (struct.pack("<IBI", reg.n_blocks, level_table, len(level_bytes)) + level_bytes + struct.pack("<%dq" % c, *[int(v) for v in symbols[0]])
            + table.tobytes() + struct.pack("<I", len(payload)) + payload)


def encode_region(p, coeffs, qstep, reg, return_symbols=False):
    """float64 [N,C] coefficients (device, Morton row order) -> PCR2 bytes at ``qstep`` with the levels of ``reg``; only the
    quantiser and the coder depend on ``qstep``, so a rate search calls this once per probe"""
    qstep = _check_qstep(qstep)
    sym = quantize_levels(coeffs, reg.coeff_level, level_steps(qstep)).cpu().numpy().astype(np.int64)
    data = struct.pack("<4sBBBBdI", MAGIC_REGION, p.depth, sym.shape[1], reg.block_log2, 0, qstep, p.n) + encode_region_symbols(p, sym, reg)
    return (data, sym) if return_symbols else data


def parse_region(p, data, count_blocks):
    """PCR2 bytes -> (C, block_log2, qstep, block levels int64 [n_blocks], dc int64 [C], table uint8 [3 * depth * C], payload),
    all on the host and all checked: ValueError for a stream that is not one, is cut short, was not made for the plan ``p``
    (its ``n`` and ``depth``), whose block count is not ``count_blocks(block_log2)``, or whose levels leave 0 .. 63.  Nothing
    the stream says reaches a kernel before these checks."""
    data = bytes(data)
    if len(data) < _HEAD_REGION.size or data[:4] != MAGIC_REGION:
        raise ValueError("not a PCR2 attribute stream")
    _, depth, c, block_log2, zero, qstep, n, n_blocks, level_table, levels_len = _HEAD_REGION.unpack(data[:_HEAD_REGION.size])
    if (depth, n) != (p.depth, p.n):
        raise ValueError(f"PCR2: the stream holds {n} rows at depth {depth}, the plan {p.n} at depth {p.depth}")
    if not 1 <= c <= MAX_CHANNELS or not (qstep > 0.0 and np.isfinite(qstep)) or block_log2 > MAX_BLOCK_LOG2 or zero or level_table >= LEVELS:
        raise ValueError("PCR2: bad header")
    if not 1 <= n_blocks <= n or n_blocks != int(count_blocks(block_log2)):
        raise ValueError(f"PCR2: {n_blocks} blocks of edge 2^{block_log2}, which the geometry does not have")
    pos, ntab = _HEAD_REGION.size, 3 * depth * c
    if len(data) < pos + levels_len + 8 * c + ntab + 4:
        raise ValueError("PCR2: truncated header")
    cdf, cdf_len, off = gaussian_tables()
    try:
        deltas = _rans_decode(data[pos:pos + levels_len], np.full(n_blocks, level_table, dtype=np.int32), cdf, cdf_len, off)
    except _lib.PccError as e:
        raise ValueError(f"PCR2: corrupt levels ({e})") from None
    pos += levels_len
    block_level = np.cumsum(deltas.astype(np.int64))
    if int(block_level.min()) < 0 or int(block_level.max()) >= LEVELS:
        raise ValueError("PCR2: a block level outside 0..63")
    dc = np.array(struct.unpack("<%dq" % c, data[pos:pos + 8 * c]), dtype=np.int64)
    pos += 8 * c
    table = np.frombuffer(data, dtype=np.uint8, count=ntab, offset=pos)
    pos += ntab
    if ntab and int(table.max()) >= LEVELS:
        raise ValueError("PCR2: table index out of range")
    (plen,) = struct.unpack("<I", data[pos:pos + 4])
    pos += 4
    payload = data[pos:pos + plen]
    if len(payload) != plen:
        raise ValueError("PCR2: truncated payload")
    return c, block_log2, float(qstep), block_level, dc, table, payload


def decode_region(p, data):
    """PCR2 bytes -> (int64 host symbols [N,C] in Morton row order, qstep, ``Region``): blocks and coefficient levels are
    rebuilt from the plan and the stream's block levels; ValueError as ``parse_region``"""
    made = {}

    def count_blocks(block_log2):
        made["block_of_row"], made["n_blocks"] = blocks(p, block_log2)
        return made["n_blocks"]

    c, block_log2, qstep, block_level, dc, table, payload = parse_region(p, data, count_blocks)
    if np.abs(dc).max() >= SYMBOL_LIMIT:
        raise ValueError("PCR2: a DC symbol of magnitude 2^28 or more")
    level_dev = torch.from_numpy(block_level.astype(np.int32)).to(p.device)
    reg = Region(block_log2, made["n_blocks"], made["block_of_row"], level_dev, coeff_levels(p, level_dev, made["block_of_row"]))
    sym = np.empty((p.n, c), dtype=np.int64)
    sym[0] = dc
    if p.n > 1:
        cdf, cdf_len, off = gaussian_tables()
        try:
            high = _rans_decode(payload, _region_indexes(p, table, c, reg.host()[1]), cdf, cdf_len, off)
        except _lib.PccError as e:
            raise ValueError(f"PCR2: corrupt payload ({e})") from None
        sym[1:] = high.reshape(c, p.n - 1).T
    return sym, qstep, reg
