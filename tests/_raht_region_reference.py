"""Region-wise quantisation of the RAHT coefficients (the "PCR2" stream of pcc_amd.raht) restated in numpy, built another way than
the kernels: blocks from the Morton keys (key >> 3b) instead of the plan's steps, block levels with np.minimum.at, coefficient
levels as the closed-form range minimum over the rows [left[i], i + w1[i]) a coefficient summarises instead of the step walk,
np.rint as the quantiser, a symbol-by-symbol table choice under the level shift, and the assembly and parsing of the stream.  The
step-based forms the kernels use are restated too (blocks_from_steps, coeff_levels_walk), so that the CPU tests can hold the two
against each other.  Plans are the dicts of tests/_raht_reference.py."""
import functools
import struct

import numpy as np

import _raht_reference as ref

LEVELS = 64
SCALES_MIN, SCALES_MAX = 0.11, 256.0
HEAD = struct.Struct("<4sBBBBdIIBI")


def block_sizes(depth, with_17=True):
    """the block sizes of the tests for a cloud of ``depth``: 0, 1, 3, the depth itself, and 17"""
    return sorted({0, 1, 3, depth} | ({17} if with_17 else set()))


def blocks_from_keys(p, b):
    """-> (block_of_row int32 [n], n_blocks): rows whose keys agree above bit 3b share a cube of edge 2^b"""
    cube = p["keys"] >> np.uint64(min(3 * b, 63))
    _, block_of_row = np.unique(cube, return_inverse=True)          # (the keys ascend, so the cubes are numbered in row order)
    return block_of_row.astype(np.int32), int(block_of_row.max()) + 1


def blocks_from_steps(p, b):
    """the rule of pcc_raht_blocks: a row opens a block iff it is row 0 or its step is >= 3b"""
    start = p["step"].astype(np.int64) >= 3 * b
    start[0] = False
    block_of_row = np.cumsum(start)
    return block_of_row.astype(np.int32), int(block_of_row[-1]) + 1


def block_levels(p, levels, block_of_row, n_blocks):
    """levels [n] in INPUT row order -> int32 [n_blocks]: the minimum over every block"""
    out = np.full(n_blocks, LEVELS - 1, dtype=np.int64)
    np.minimum.at(out, block_of_row, np.asarray(levels, dtype=np.int64)[p["perm"]])
    return out.astype(np.int32)


def coeff_levels_range_min(p, block_level, block_of_row):
    """uint8 [n]: row i > 0 takes the smallest block level among the rows [left[i], i + w1[i]), row 0 the smallest of all"""
    lev = np.asarray(block_level, dtype=np.int64)[block_of_row]
    out = np.empty(lev.size, dtype=np.uint8)
    out[0] = lev.min()
    for i in range(1, lev.size):
        out[i] = lev[p["left"][i]:i + p["w1"][i]].min()
    return out


def coeff_levels_walk(p, block_level, block_of_row):
    """the same by the walk of pcc_raht_coeff_levels over the transform's steps, finest first"""
    lev = np.asarray(block_level, dtype=np.int64)[block_of_row]
    out = lev.copy()
    for s in range(3 * p["depth"]):
        rows = p["step_rows"][p["step_offsets"][s]:p["step_offsets"][s + 1]].astype(np.int64)
        left = p["left"][rows].astype(np.int64)
        m = np.minimum(lev[left], lev[rows])
        out[rows] = m
        lev[left] = m
    out[0] = lev[0]
    return out.astype(np.uint8)


def level_steps(qstep):
    return np.float64(qstep) * np.float64(SCALES_MAX / SCALES_MIN) ** (np.arange(LEVELS, dtype=np.float64) / (LEVELS - 1))


def quantize(coeffs, coeff_level, steps):
    return np.rint(np.asarray(coeffs, dtype=np.float64) / steps[coeff_level][:, None]).astype(np.int64)


def dequantize(symbols, coeff_level, steps):
    return np.asarray(symbols, dtype=np.float64) * steps[coeff_level][:, None]


def level_maps(coords, seed=31):
    """name -> uint8 [n] per-point levels in input order: flat 0, flat 63, seeded random 0 .. 63, and two halves along x (the
    lower half at level 0, the upper at 12)"""
    coords = np.asarray(coords)
    n = coords.shape[0]
    x = coords[:, 0]
    return {"flat0": np.zeros(n, dtype=np.uint8), "flat63": np.full(n, 63, dtype=np.uint8),
            "random": np.random.default_rng(seed).integers(0, 64, n).astype(np.uint8),
            "halves": np.where(x > (int(x.min()) + int(x.max())) // 2, 12, 0).astype(np.uint8)}


def choose_tables_shifted(symbols, contexts, n_contexts, shift, cdf, cdf_len, offset):
    """per context the table t with the smallest ideal code length when a symbol with shift h is coded with table
    clip(t - h, 0, 63); ties to the lowest index, 0 for an empty context.  Symbol by symbol, integer costs of 2^-20 bit."""
    scale = 1 << 20
    n_tables = cdf.shape[0]

    @functools.lru_cache(maxsize=None)
    def cost(t, v):
        maxv = int(cdf_len[t]) - 2
        x = v - int(offset[t])
        extra = 0
        if x < 0:
            extra, x = ref.bypass_bits(-2 * x - 1), maxv
        elif x >= maxv:
            extra, x = ref.bypass_bits(2 * (x - maxv)), maxv
        freq = int(cdf[t, x + 1]) - int(cdf[t, x])
        return int(np.rint((16.0 - np.log2(np.float64(freq))) * scale)) + extra * scale

    symbols, contexts, shift = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (symbols, contexts, shift))
    out = np.zeros(n_contexts, dtype=np.uint8)
    for ctx in range(n_contexts):
        mine = contexts == ctx
        pairs, counts = np.unique(np.stack([symbols[mine], shift[mine]], axis=1), axis=0, return_counts=True)
        if pairs.shape[0] == 0:
            continue
        best, best_cost = 0, None
        for t in range(n_tables):
            total = sum(k * cost(min(max(t - h, 0), n_tables - 1), v) for (v, h), k in zip(pairs.tolist(), counts.tolist()))
            if best_cost is None or total < best_cost:
                best, best_cost = t, total
        out[ctx] = best
    return out


def stream_indexes(p, table, c, coeff_level):
    """the table of every coded symbol, channel-major over the rows 1 .. n-1"""
    n = p["step"].size
    out = []
    for ch in range(c):
        for i in range(1, n):
            out.append(min(max(int(table[int(p["step"][i]) * c + ch]) - (int(coeff_level[i]) - int(coeff_level[0])), 0), LEVELS - 1))
    return np.asarray(out, dtype=np.int32)


def assemble(p, symbols, qstep, block_log2, block_level, coeff_level, tables, rans_encode):
    """PCR2 bytes of int64 symbols [n,c] (Morton row order).  ``tables`` = (cdf, cdf_length, offset) of the 64 Gaussian tables,
    ``rans_encode(symbols, indexes, cdf, cdf_length, offset)`` the range coder."""
    n, c = symbols.shape
    deltas = np.diff(np.asarray(block_level, dtype=np.int64), prepend=0)
    level_table = int(choose_tables_shifted(deltas, np.zeros(deltas.size), 1, np.zeros(deltas.size), *tables)[0])
    level_bytes = rans_encode(deltas.astype(np.int32), np.full(deltas.size, level_table, dtype=np.int32), *tables)
    high = symbols[1:].T.reshape(-1)
    contexts = (p["step"][1:].astype(np.int64)[None, :] * c + np.arange(c)[:, None]).reshape(-1)
    shift = np.tile(coeff_level[1:].astype(np.int64) - int(coeff_level[0]), c)
    table = choose_tables_shifted(high, contexts, 3 * p["depth"] * c, shift, *tables)
    payload = rans_encode(high.astype(np.int32), stream_indexes(p, table, c, coeff_level), *tables) if high.size else b""
    return (HEAD.pack(b"PCR2", p["depth"], c, block_log2, 0, qstep, n, len(block_level), level_table, len(level_bytes)) + level_bytes
            + struct.pack("<%dq" % c, *[int(v) for v in symbols[0]]) + table.tobytes() + struct.pack("<I", len(payload)) + payload)


def field_boundaries(data):
    """the offsets at which the fields of a PCR2 stream begin (and its length): a stream cut at any of them but the last is
    short"""
    _, depth, c, _, _, _, _, _, _, levels_len = HEAD.unpack(data[:HEAD.size])
    fixed = [0, 4, 5, 6, 7, 8, 16, 20, 24, 25, 29]
    pos = 29 + levels_len
    dc = pos + 8 * c
    tab = dc + 3 * depth * c
    return fixed + [pos, dc, tab, tab + 4, len(data)]


def parse(data):
    """PCR2 bytes -> dict of its fields, unchecked beyond their lengths"""
    magic, depth, c, block_log2, zero, qstep, n, n_blocks, level_table, levels_len = HEAD.unpack(data[:HEAD.size])
    assert magic == b"PCR2" and zero == 0
    pos = HEAD.size
    levels = data[pos:pos + levels_len]
    pos += levels_len
    dc = np.array(struct.unpack("<%dq" % c, data[pos:pos + 8 * c]), dtype=np.int64)
    pos += 8 * c
    table = np.frombuffer(data, dtype=np.uint8, count=3 * depth * c, offset=pos)
    pos += 3 * depth * c
    (plen,) = struct.unpack("<I", data[pos:pos + 4])
    pos += 4
    assert len(data) == pos + plen
    return {"depth": depth, "c": c, "block_log2": block_log2, "qstep": qstep, "n": n, "n_blocks": n_blocks, "level_table": level_table,
            "levels": levels, "dc": dc, "table": table, "payload": data[pos:]}
