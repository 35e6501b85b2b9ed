"""TEST INFRASTRUCTURE ONLY: numpy restatement of the neighbour-context octree stream "PCO2" (the product's side is
learned-compression-..._amd/octree.py + csrc/octree.hip; the format is described in that module's docstring and in DESIGN.md
"Octree contexts (PCO2)").  Patterns, histograms, tables, the mode choice and the whole encoder and decoder, on the CPU.  The
occupancy bytes come from the PCO1 twin (oracle/octree.py); the range coder is the library's host entry points, which need no
GPU.  The product imports neither this file nor the oracle.

The encoder's mode choice compares float64 costs; the expressions below are evaluated in the order the format's encoder defines
(per level: counts times 16 - log2(frequency), summed by numpy over the 512 x 2 table), so both sides get the same floats.
"""
import struct

import numpy as np

from oracle import octree as oo

MAGIC = b"PCO2"
MIN_CODED_NODES = 64
STREAM_BITS = 96.0          # u32 length + the coder's 8-byte final state
DIRECTIONS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))      # bit 0 .. bit 5


# ---------------------------------------------------------------------------------------------- the range coder (host entry points)
def _lib():
    from pcc_amd import _lib as binding
    return binding.lib()


def rans_encode(symbols, indexes, cdf, sizes, offsets):
    symbols = np.ascontiguousarray(symbols, dtype=np.int32)
    indexes = np.ascontiguousarray(indexes, dtype=np.int32)
    cdf = np.ascontiguousarray(cdf, dtype=np.int32)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    cap = 4 * (3 * symbols.size + 4)
    out = np.empty(cap, dtype=np.uint8)
    got = _lib().pcc_rans_encode_with_indexes(symbols.ctypes.data, indexes.ctypes.data, symbols.size, cdf.ctypes.data, cdf.shape[1],
                                              sizes.ctypes.data, offsets.ctypes.data, out.ctypes.data, cap)
    assert got >= 8, got
    return out[:got].tobytes()


def rans_decode(payload, indexes, cdf, sizes, offsets):
    indexes = np.ascontiguousarray(indexes, dtype=np.int32)
    cdf = np.ascontiguousarray(cdf, dtype=np.int32)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    buf = np.frombuffer(payload, dtype=np.uint8)
    out = np.empty(indexes.size, dtype=np.int32)
    rc = _lib().pcc_rans_decode_with_indexes(buf.ctypes.data, len(payload), indexes.ctypes.data, indexes.size, cdf.ctypes.data,
                                             cdf.shape[1], sizes.ctypes.data, offsets.ctypes.data, out.ctypes.data)
    if rc < 0:
        raise ValueError("PCO2: the range coder refused the payload (%d)" % rc)
    return out


# ---------------------------------------------------------------------------------------------- model
def level_nodes(keys_sorted, depth):
    """sorted leaf keys -> per level 0..depth-1 the ascending node keys (3 * level bits)"""
    return [np.unique(keys_sorted >> np.uint64(3 * (depth - level))) for level in range(depth)]


def patterns_of(nodes, level):
    """ascending node keys of one level -> uint8 patterns: bit d set when the neighbour in DIRECTIONS[d] is a node"""
    grid = oo.keys_to_grid(nodes, level)
    out = np.zeros(nodes.shape[0], dtype=np.uint8)
    for bit, d in enumerate(DIRECTIONS):
        nb = grid + np.asarray(d, dtype=np.int64)
        inside = ((nb >= 0) & (nb < (1 << level))).all(axis=1)
        keys = oo.morton_keys(np.where(inside[:, None], nb, 0), level)
        at = np.minimum(np.searchsorted(nodes, keys), nodes.shape[0] - 1)
        out |= ((inside & (nodes[at] == keys)).astype(np.uint8) << bit).astype(np.uint8)
    return out


def histogram(level_bytes, patterns):
    """int64 [512,2]: how often bit j of a byte is 0 / 1 in context pattern * 8 + j"""
    hist = np.zeros((512, 2), dtype=np.int64)
    for j in range(8):
        bit = (level_bytes.astype(np.int64) >> j) & 1
        for b in (0, 1):
            hist[j::8, b] += np.bincount(patterns[bit == b], minlength=64)
    return hist


def f1_of(counts):
    out = np.zeros(512, dtype=np.int64)
    for c in range(512):
        n0, n1 = int(counts[c, 0]), int(counts[c, 1])
        out[c] = min(max(((2 * n1 + 1) * 65535) // (2 * (n0 + n1) + 2), 1), 65534)
    return out


def tables_of(f1):
    return np.stack([np.zeros(512, np.int64), 65535 - f1, np.full(512, 65535), np.full(512, 65536)], axis=1).astype(np.int32)


def bits_of(freq):
    return 16.0 - np.log2(np.asarray(freq, dtype=np.float64))


def binary_cost(hist, f1):
    return float((hist[:, 0] * bits_of(65535 - f1) + hist[:, 1] * bits_of(f1)).sum())


def binary_symbols(level_bytes, patterns):
    symbols = np.unpackbits(level_bytes[:, None], axis=1, bitorder="little").reshape(-1)
    indexes = (patterns.astype(np.int64)[:, None] * 8 + np.arange(8)).reshape(-1)
    return symbols, indexes


def level_costs(level_bytes, hist, state):
    """bits of mode 0, 1, 2, 3 for one level"""
    byte_freq = np.diff(oo.level_cdf(level_bytes).astype(np.int64))
    counts = np.bincount(level_bytes.astype(np.int64) - 1, minlength=255)
    used = int((hist.sum(axis=1) > 0).sum())
    return [8.0 * level_bytes.shape[0],
            binary_cost(hist, f1_of(state)) + STREAM_BITS,
            binary_cost(hist, f1_of(hist)) + 8.0 * (64 + 2 * used) + STREAM_BITS,
            float((counts * bits_of(byte_freq[:255])).sum()) + 8.0 * len(oo._leb128(byte_freq)) + STREAM_BITS]


def choose_mode(level_bytes, hist, state):
    if level_bytes.shape[0] < MIN_CODED_NODES:
        return 0
    return int(np.argmin(level_costs(level_bytes, hist, state)))


SIZES4, ZEROS = np.full(512, 4, dtype=np.int32), np.zeros(512, dtype=np.int32)


def encode_level(level_bytes, patterns, hist, state, mode):
    if mode == 0:
        return b"\x00" + level_bytes.tobytes()
    if mode == 3:
        cdf = oo.level_cdf(level_bytes)
        side = oo._leb128(np.diff(cdf.astype(np.int64)))
        payload = rans_encode(level_bytes.astype(np.int32) - 1, np.zeros(level_bytes.shape[0]), cdf[None], [257], [0])
    else:
        f1 = f1_of(state if mode == 1 else hist)
        side = b""
        if mode == 2:
            used = hist.sum(axis=1) > 0
            bitmap = bytearray(64)
            for c in np.nonzero(used)[0]:
                bitmap[c >> 3] |= 1 << (c & 7)
            side = bytes(bitmap) + b"".join(struct.pack("<H", int(f1[c])) for c in np.nonzero(used)[0])
        payload = rans_encode(*binary_symbols(level_bytes, patterns), tables_of(f1), SIZES4, ZEROS)
    return bytes([mode]) + side + struct.pack("<I", len(payload)) + payload


def analyse(points, stride):
    """-> (origin, depth, levels, patterns, hists) of a cloud: everything the encoder codes"""
    origin, g, depth = oo.grid_of(points, stride)
    keys = np.sort(oo.morton_keys(g, depth)) if g.shape[0] else np.zeros(0, dtype=np.uint64)
    if keys.shape[0] > 1 and (np.diff(keys.astype(np.int64)) == 0).any():
        raise ValueError("duplicate coordinates")
    levels = oo.occupancy_levels(keys, depth)
    pats = [patterns_of(nodes, level) for level, nodes in enumerate(level_nodes(keys, depth))]
    hists = [histogram(lv, p) for lv, p in zip(levels, pats)]
    return origin, depth, levels, pats, hists


def encode_points(points, stride, modes=None):
    """int [N,3] -> PCO2 bytes; ``modes`` (test hook) forces the mode of the levels it lists: {level: mode}"""
    points = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    origin, depth, levels, pats, hists = analyse(points, stride)
    out = MAGIC + struct.pack("<BBHi3iI", depth, 0, 0, int(stride), *[int(v) for v in origin], points.shape[0])
    out += struct.pack("<%dI" % depth, *[lv.shape[0] for lv in levels])
    state = np.zeros((512, 2), dtype=np.int64)
    chosen = []
    for level in range(depth):
        mode = choose_mode(levels[level], hists[level], state)
        if modes and level in modes:
            mode = modes[level]
        chosen.append(mode)
        out += encode_level(levels[level], pats[level], hists[level], state, mode)
        state = (state >> 1) + hists[level]
    encode_points.last_modes = chosen
    return out


def _take(data, pos, count, what):
    if pos + count > len(data):
        raise ValueError("PCO2: truncated " + what)
    return data[pos:pos + count], pos + count


def _varints(data, pos, count):
    vals = []
    for _ in range(count):
        v = shift = 0
        while True:
            if pos >= len(data):
                raise ValueError("PCO2: truncated frequency table")
            byte = data[pos]
            pos += 1
            v |= (byte & 0x7F) << shift
            shift += 7
            if not byte & 0x80:
                break
        vals.append(v)
    return np.array(vals, dtype=np.int64), pos


def decode_keys(data):
    """PCO2 bytes -> (origin, stride, depth, leaf keys ascending, mode per level, offset of every level's mode byte);
    ValueError for anything malformed"""
    data = bytes(data)
    if len(data) < 28 or data[:4] != MAGIC:
        raise ValueError("not a PCO2 stream")
    depth, _, _, stride, ox, oy, oz, n = struct.unpack("<BBHi3iI", data[4:28])
    if depth > 21 or stride < 1:
        raise ValueError("PCO2: bad header")
    sizes, pos = _take(data, 28, 4 * depth, "header")
    counts = list(struct.unpack("<%dI" % depth, sizes))
    origin = np.array([ox, oy, oz], dtype=np.int64)
    if n == 0 or depth == 0:
        if depth or n > 1 or pos != len(data):
            raise ValueError("PCO2: bad header")
        return origin, stride, depth, np.zeros(n, dtype=np.uint64), [], []
    if counts[0] != 1:
        raise ValueError("PCO2: the root level must hold one node")
    nodes = np.zeros(1, dtype=np.uint64)
    state = np.zeros((512, 2), dtype=np.int64)
    modes, offsets = [], []
    for level in range(depth):
        nl = counts[level]
        assert nl == nodes.shape[0]
        want = counts[level + 1] if level + 1 < depth else n
        pats = patterns_of(nodes, level)
        offsets.append(pos)
        head, pos = _take(data, pos, 1, "level")
        mode = head[0]
        modes.append(mode)
        if mode > 3 or (nl < MIN_CODED_NODES and mode != 0):
            raise ValueError("PCO2: mode %d at level %d (%d nodes)" % (mode, level, nl))
        if mode == 0:
            raw, pos = _take(data, pos, nl, "raw level")
            lv = np.frombuffer(raw, dtype=np.uint8)
        else:
            if mode == 3:
                freqs, pos = _varints(data, pos, 256)
                if freqs.min() < 1 or freqs.sum() != 65536:
                    raise ValueError("PCO2: invalid frequency table")
                cdf = np.concatenate([[0], np.cumsum(freqs)])[None]
            elif mode == 2:
                bitmap, pos = _take(data, pos, 64, "bitmap")
                used = np.array([(bitmap[c >> 3] >> (c & 7)) & 1 for c in range(512)], dtype=bool)
                present = np.zeros(512, dtype=bool)
                for p in set(pats.tolist()):
                    present[p * 8:p * 8 + 8] = True
                if (used != present).any():
                    raise ValueError("PCO2: the context bitmap does not match the patterns")
                table, pos = _take(data, pos, 2 * int(used.sum()), "tables")
                f1 = np.full(512, 32767, dtype=np.int64)
                f1[used] = struct.unpack("<%dH" % int(used.sum()), table)
                if f1.min() < 1 or f1.max() > 65534:
                    raise ValueError("PCO2: frequency out of range")
            else:
                f1 = f1_of(state)
            length, pos = _take(data, pos, 4, "payload length")
            payload, pos = _take(data, pos, struct.unpack("<I", length)[0], "payload")
            if mode == 3:
                sym = rans_decode(payload, np.zeros(nl), cdf, [257], [0])
                if sym.min() < 0 or sym.max() > 254:
                    raise ValueError("PCO2: corrupt payload")
                lv = (sym + 1).astype(np.uint8)
            else:
                indexes = (pats.astype(np.int64)[:, None] * 8 + np.arange(8)).reshape(-1)
                sym = rans_decode(payload, indexes, tables_of(f1), SIZES4, ZEROS)
                if sym.min() < 0 or sym.max() > 1:
                    raise ValueError("PCO2: corrupt payload")
                lv = (sym.reshape(nl, 8) << np.arange(8)).sum(axis=1).astype(np.uint8)
        if (lv == 0).any():
            raise ValueError("PCO2: an empty node at level %d" % level)
        bits = np.unpackbits(lv[:, None], axis=1, bitorder="little")
        if int(bits.sum()) != want:
            raise ValueError("PCO2: the occupancy of level %d does not match the size of the next" % level)
        state = (state >> 1) + histogram(lv, pats)
        rows, children = np.nonzero(bits)
        nodes = (nodes[rows] << np.uint64(3)) | children.astype(np.uint64)
    if pos != len(data):
        raise ValueError("PCO2: bytes behind the last level")
    return origin, stride, depth, nodes, modes, offsets


def decode_points(data):
    """PCO2 bytes -> int64 [N,3] in ascending Morton order"""
    origin, stride, depth, keys, _, _ = decode_keys(data)
    if keys.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.int64)
    return oo.keys_to_grid(keys, depth) * stride + origin
