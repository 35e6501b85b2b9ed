"""Lossless coder for the stride-8 latent coordinate list of file mode ("PCO1").

Takes the place of ``ColorModel.gpcc_encode`` / ``gpcc_decode`` (/root/reference/model/model.py:318-395),
which write a PLY and shell out to the external MPEG G-PCC binary ``tmc3``.  ``tmc3`` is not part
of the reference tree and not available here, and its bitstream is not reproduced: PCO1 is this
build's own format, lossless like the G-PCC octree mode the reference configures
(``--mode=0 --positionQuantizationScale=1 ...``), but NOT G-PCC compatible.

Device (csrc/octree.hip): Morton keys, radix sort, one occupancy byte per occupied octree node and
level; and the inverse expansion.  Host: the per-level frequency tables and the range coder shared
with the latents (``pcc_rans_*_with_indexes``), table index = octree level.

Stream (little-endian):
    "PCO1" | u8 depth | u8 0 | u16 0 | i32 stride | i32 origin[3] | u32 n_points |
    u32 nodes_per_level[depth] | u8 has_table[depth] | 256 LEB128 frequencies per level with a table |
    u32 payload_len | payload
A level with fewer than 64 nodes is coded with the flat table (257 / 65536 per byte value).

"PCO2" (opt-in, ``encode_coordinates(..., contexts=True)``; DESIGN.md "Octree contexts (PCO2)") codes the same occupancy bytes
with neighbour contexts.  The pattern of a node at level L is 6 bits (+x, -x, +y, -y, +z, -z from bit 0), set when the face
neighbour is an occupied node of level L; bit j of the node's byte is a binary symbol with context ``pattern * 8 + j``.  No
context depends on bits of the same byte, so the table indexes of a level are known before the level is decoded and the range
coder is the one above.  The table of a context with counts (n0, n1): f1 = clamp((2 n1 + 1) * 65535 // (2 (n0 + n1) + 2), 1,
65534), CDF [0, 65535 - f1, 65535, 65536].  Backward state ``cnt[512][2]``: zero at the root, after every level
``cnt = (cnt >> 1) + hist_L`` with hist_L the level's (context, bit) histogram.  Stream:
    "PCO2" | the rest of PCO1's 28-byte header | u32 nodes_per_level[depth] | per level: u8 mode | side information | payload
    mode 0  raw: the level's bytes (the only mode below 64 nodes)
    mode 1  backward: tables from cnt, no side information | u32 len | rANS stream of the level's 8 n binary symbols
    mode 2  explicit: tables from hist_L: 64-byte bitmap of the contexts in use (bit c, little-endian), u16 f1 per context in
            use, ascending | u32 len | rANS stream
    mode 3  byte table: 256 LEB128 frequencies as in PCO1 | u32 len | rANS stream of the symbols byte - 1
The encoder takes the mode with the smallest estimated cost (float64, on the host); the choice is part of the stream.  Device:
patterns and histograms of all levels in one call (encode), a level-stepped expansion (decode); the decoder checks everything it
reads on the host before a kernel consumes it.
"""
import struct

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .entropy import _rans_decode, _rans_encode, _to_device, _to_host

MAGIC = b"PCO1"
MAGIC_CONTEXTS = b"PCO2"
_MIN_TABLE_NODES = 64
_PRECISION = 16
_CONTEXTS = 512
MODE_RAW, MODE_BACKWARD, MODE_EXPLICIT, MODE_BYTES = 0, 1, 2, 3
# what a coded level pays besides its symbols, in bits: the u32 length and the range coder's final state (8 bytes)
_STREAM_BITS = 96.0


def _flat_cdf():
    f = np.full(256, 257, dtype=np.int64)
    f[255] = 1                          # tail bin (the coder's escape symbol; never emitted)
    out = np.zeros(257, dtype=np.int32)
    out[1:] = np.cumsum(f)
    return out


def _quantized_cdf(level_bytes):
    """occupancy bytes of one level -> 257-entry CDF (255 byte values + tail), 16-bit precision"""
    L = _lib.lib()
    counts = np.bincount(level_bytes.astype(np.int64) - 1, minlength=255).astype(np.float32)
    pmf = np.zeros(256, dtype=np.float32)
    pmf[:255] = counts / np.float32(counts.sum())
    cdf = np.zeros(257, dtype=np.int32)
    check(L.pcc_pmf_to_quantized_cdf(ptr(pmf), 256, _PRECISION, ptr(cdf)))
    return cdf


def _write_varints(values):
    out = bytearray()
    for v in values:
        v = int(v)
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80)
            v >>= 7
        out.append(v)
    return bytes(out)


def _read_varints(buf, pos, count):
    out = np.empty(count, dtype=np.int64)
    for i in range(count):
        v = shift = 0
        while True:
            if pos >= len(buf):
                raise ValueError("PCO1: truncated frequency table")
            b = buf[pos]
            pos += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if b < 0x80:
                break
        out[i] = v
    return out, pos


def _split_levels(host, cnt, depth):
    levels, o = [], 0
    for l in range(depth):
        levels.append(host[o:o + int(cnt[l])])
        o += int(cnt[l])
    return levels


def _device_levels(coords, stride, contexts):
    """the device half of the encoder: coords int32 [n,4] (n >= 1) -> (origin, depth, nodes per level, occupancy bytes per level)
    and, with ``contexts``, also (pattern bytes per level, int64 histograms [depth,512,2]), else (None, None)"""
    L = _lib.lib()
    n = int(coords.shape[0])
    lo = coords[:, 1:4].amin(dim=0)
    hi = coords[:, 1:4].amax(dim=0)
    lohi = torch.cat([lo, hi]).cpu().numpy().astype(np.int64)
    origin = np.ascontiguousarray(lohi[:3], dtype=np.int32)
    depth = int(((lohi[3:] - lohi[:3]).max() // stride)).bit_length()
    dev = coords.device
    occ = torch.empty(max(depth, 1) * n, dtype=torch.uint8, device=dev)
    counts = torch.empty(depth + 2, dtype=torch.int32, device=dev)
    nbytes = L.pcc_octree_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if contexts:
        pat = torch.empty(max(depth, 1) * n, dtype=torch.uint8, device=dev)
        hists = torch.empty((max(depth, 1), _CONTEXTS, 2), dtype=torch.int32, device=dev)       # uint32 counters, each <= n < 2^31
        check(L.pcc_octree_context_levels(ptr(coords), n, stride, ptr(origin), depth, ptr(occ), ptr(pat), ptr(hists), ptr(counts),
                                          ptr(scratch), nbytes, _lib.stream()))
    else:
        check(L.pcc_octree_occupancy(ptr(coords), n, stride, ptr(origin), depth, ptr(occ), ptr(counts), ptr(scratch), nbytes,
                                     _lib.stream()))
    cnt = counts.cpu().numpy().astype(np.int64)
    if cnt[depth + 1] != 0:
        raise ValueError("encode_coordinates: %d coordinates are not on the stride-%d lattice" % (cnt[depth + 1], stride))
    if depth and cnt[depth] != n:
        raise ValueError("encode_coordinates: duplicate coordinates (%d distinct of %d)" % (cnt[depth], n))
    if depth == 0 and n != 1:
        raise ValueError("encode_coordinates: duplicate coordinates")
    host = host_pat = np.zeros(0, dtype=np.uint8)
    host_hists = None
    if depth:
        picked = torch.cat([occ[l * n:l * n + int(cnt[l])] for l in range(depth)])
        host = _to_host(picked, "octree_occ").copy()
        if contexts:
            picked = torch.cat([pat[l * n:l * n + int(cnt[l])] for l in range(depth)])
            host_pat = _to_host(picked, "octree_pat").copy()
            host_hists = _to_host(hists[:depth], "octree_hist").astype(np.int64)
    return origin, depth, cnt, host, host_pat, host_hists


def encode_coordinates(coords, stride, contexts=False):
    """coords: int32 [N,4] on the GPU (batch column ignored; one cloud) -> bytes: PCO1, or with ``contexts`` PCO2."""
    if coords.device.type != "cuda":
        raise RuntimeError("encode_coordinates: coordinates must live on the GPU")
    coords = coords.to(torch.int32).contiguous()
    n = int(coords.shape[0])
    stride = int(stride)
    if contexts:
        return _encode_contexts(coords, n, stride)
    if n == 0:
        return MAGIC + struct.pack("<BBHi3iI", 0, 0, 0, stride, 0, 0, 0, 0) + struct.pack("<I", 0)
    origin, depth, cnt, host, _, _ = _device_levels(coords, stride, False)
    levels = _split_levels(host, cnt, depth)
    head = MAGIC + struct.pack("<BBHi3iI", depth, 0, 0, stride, int(origin[0]), int(origin[1]), int(origin[2]), n)
    head += struct.pack("<%dI" % depth, *[int(c) for c in cnt[:depth]])
    flags, tables = bytearray(), b""
    cdf = np.zeros((max(depth, 1), 257), dtype=np.int32)
    for l, lv in enumerate(levels):
        if lv.shape[0] >= _MIN_TABLE_NODES:
            cdf[l] = _quantized_cdf(lv)
            flags.append(1)
            tables += _write_varints(np.diff(cdf[l].astype(np.int64)))
        else:
            cdf[l] = _flat_cdf()
            flags.append(0)
    head += bytes(flags) + tables
    if depth == 0:
        return head + struct.pack("<I", 0)
    symbols = host.astype(np.int32) - 1
    indexes = np.repeat(np.arange(depth, dtype=np.int32), cnt[:depth])
    payload = _rans_encode(symbols, indexes, cdf, np.full(depth, 257, dtype=np.int32), np.zeros(depth, dtype=np.int32))
    return head + struct.pack("<I", len(payload)) + payload


# ---- PCO2: neighbour contexts ----------------------------------------------------------------------------------------
def _context_f1(counts):
    """(n0, n1) per context, int64 [512,2] -> the 16-bit frequency of a set bit, int64 [512]"""
    n0, n1 = counts[:, 0], counts[:, 1]
    return np.clip(((2 * n1 + 1) * 65535) // (2 * (n0 + n1) + 2), 1, 65534)


def _context_cdf(f1):
    """f1 int64 [512] -> the coder's tables, int32 [512,4]: bit 0, bit 1 and the tail bin of frequency 1 (never emitted)"""
    cdf = np.empty((_CONTEXTS, 4), dtype=np.int32)
    cdf[:, 0] = 0
    cdf[:, 1] = 65535 - f1
    cdf[:, 2] = 65535
    cdf[:, 3] = 65536
    return cdf


def _bits(freq):
    return 16.0 - np.log2(np.asarray(freq, dtype=np.float64))


def _binary_cost(hist, f1):
    """bits the level's binary symbols take with the tables of f1 (float64)"""
    return float((hist[:, 0] * _bits(65535 - f1) + hist[:, 1] * _bits(f1)).sum())


def _level_hist(level_bytes, patterns):
    """the (context, bit) histogram of one level on the host, int64 [512,2] (what the device counts in the encoder)"""
    bits = np.unpackbits(level_bytes[:, None], axis=1, bitorder="little").astype(np.int64)
    index = (patterns.astype(np.int64)[:, None] * 8 + np.arange(8)) * 2 + bits
    return np.bincount(index.reshape(-1), minlength=2 * _CONTEXTS).reshape(_CONTEXTS, 2)


def _binary_symbols(level_bytes, patterns):
    symbols = np.unpackbits(level_bytes[:, None], axis=1, bitorder="little").astype(np.int32).reshape(-1)
    indexes = (patterns.astype(np.int32)[:, None] * 8 + np.arange(8, dtype=np.int32)).reshape(-1)
    return symbols, indexes


_BINARY_SIZES = np.full(_CONTEXTS, 4, dtype=np.int32)
_BINARY_OFFSETS = np.zeros(_CONTEXTS, dtype=np.int32)
_ONE_BYTE_TABLE = (np.full(1, 257, dtype=np.int32), np.zeros(1, dtype=np.int32))


def _encode_level(level_bytes, patterns, hist, cnt):
    """one level of PCO2 after its node count: the mode byte, the mode's side information and the payload"""
    nl = level_bytes.shape[0]
    if nl < _MIN_TABLE_NODES:
        return bytes([MODE_RAW]) + level_bytes.tobytes()
    f1_back, f1_own = _context_f1(cnt), _context_f1(hist)
    used = hist.sum(axis=1) > 0
    byte_cdf = _quantized_cdf(level_bytes)
    byte_table = _write_varints(np.diff(byte_cdf.astype(np.int64)))
    byte_counts = np.bincount(level_bytes.astype(np.int64) - 1, minlength=255)
    costs = [8.0 * nl,
             _binary_cost(hist, f1_back) + _STREAM_BITS,
             _binary_cost(hist, f1_own) + 8.0 * (64 + 2 * int(used.sum())) + _STREAM_BITS,
             float((byte_counts * _bits(np.diff(byte_cdf.astype(np.int64))[:255])).sum()) + 8.0 * len(byte_table) + _STREAM_BITS]
    mode = int(np.argmin(costs))                    # the first of equal costs
    if mode == MODE_RAW:
        return bytes([MODE_RAW]) + level_bytes.tobytes()
    if mode == MODE_BYTES:
        side = byte_table
        payload = _rans_encode(level_bytes.astype(np.int32) - 1, np.zeros(nl, dtype=np.int32), byte_cdf.reshape(1, 257), *_ONE_BYTE_TABLE)
    else:
        if mode == MODE_BACKWARD:
            side, f1 = b"", f1_back
        else:
            side = np.packbits(used, bitorder="little").tobytes() + f1_own[used].astype("<u2").tobytes()
            f1 = f1_own
        symbols, indexes = _binary_symbols(level_bytes, patterns)
        payload = _rans_encode(symbols, indexes, _context_cdf(f1), _BINARY_SIZES, _BINARY_OFFSETS)
    return bytes([mode]) + side + struct.pack("<I", len(payload)) + payload


def context_levels(coords, stride):
    """coords int32 [N,4] on the GPU, N >= 1 -> (depth, occupancy bytes per level, pattern bytes per level, int64 histograms
    [depth,512,2]): what the device hands the PCO2 encoder"""
    coords = coords.to(torch.int32).contiguous()
    _, depth, cnt, host, host_pat, hists = _device_levels(coords, int(stride), True)
    if hists is None:
        hists = np.zeros((0, _CONTEXTS, 2), dtype=np.int64)
    return depth, _split_levels(host, cnt, depth), _split_levels(host_pat, cnt, depth), hists


def _encode_contexts(coords, n, stride):
    if n == 0:
        return MAGIC_CONTEXTS + struct.pack("<BBHi3iI", 0, 0, 0, stride, 0, 0, 0, 0)
    origin, depth, cnt, host, host_pat, hists = _device_levels(coords, stride, True)
    out = [MAGIC_CONTEXTS + struct.pack("<BBHi3iI", depth, 0, 0, stride, int(origin[0]), int(origin[1]), int(origin[2]), n),
           struct.pack("<%dI" % depth, *[int(c) for c in cnt[:depth]])]
    state = np.zeros((_CONTEXTS, 2), dtype=np.int64)
    levels, patterns = _split_levels(host, cnt, depth), _split_levels(host_pat, cnt, depth)
    for l in range(depth):
        out.append(_encode_level(levels[l], patterns[l], hists[l], state))
        state = (state >> 1) + hists[l]
    return b"".join(out)


def _take(data, pos, count, what):
    if count < 0 or pos + count > len(data):
        raise ValueError("PCO2: truncated %s" % what)
    return data[pos:pos + count], pos + count


def _decode_level(data, pos, nl, patterns, cnt, level):
    """reads one level at ``pos`` -> (occupancy bytes uint8 [nl], new pos); everything it reads is checked here"""
    mode_byte, pos = _take(data, pos, 1, "level %d" % level)
    mode = mode_byte[0]
    if mode > MODE_BYTES:
        raise ValueError("PCO2: mode %d at level %d" % (mode, level))
    if nl < _MIN_TABLE_NODES and mode != MODE_RAW:
        raise ValueError("PCO2: level %d holds %d nodes and is not raw" % (level, nl))
    if mode == MODE_RAW:
        raw, pos = _take(data, pos, nl, "level %d" % level)
        return np.frombuffer(raw, dtype=np.uint8).copy(), pos
    if mode == MODE_BYTES:
        freqs, pos = _read_varints(data, pos, 256)
        if freqs.min() < 1 or freqs.sum() != 1 << _PRECISION:
            raise ValueError("PCO2: invalid frequency table at level %d" % level)
        byte_cdf = np.zeros((1, 257), dtype=np.int32)
        byte_cdf[0, 1:] = np.cumsum(freqs)
    elif mode == MODE_EXPLICIT:
        bitmap, pos = _take(data, pos, _CONTEXTS // 8, "context bitmap at level %d" % level)
        used = np.unpackbits(np.frombuffer(bitmap, dtype=np.uint8), bitorder="little").astype(bool)
        present = np.zeros(_CONTEXTS, dtype=bool)
        present.reshape(64, 8)[np.unique(patterns)] = True
        if (used != present).any():
            raise ValueError("PCO2: the context bitmap of level %d does not match the level's patterns" % level)
        table, pos = _take(data, pos, 2 * int(used.sum()), "tables at level %d" % level)
        f1 = np.full(_CONTEXTS, 32767, dtype=np.int64)
        f1[used] = np.frombuffer(table, dtype="<u2")
        if f1.min() < 1 or f1.max() > 65534:
            raise ValueError("PCO2: frequency out of range at level %d" % level)
    else:
        f1 = _context_f1(cnt)
    length, pos = _take(data, pos, 4, "payload length at level %d" % level)
    payload, pos = _take(data, pos, struct.unpack("<I", length)[0], "payload at level %d" % level)
    try:
        if mode == MODE_BYTES:
            sym = _rans_decode(payload, np.zeros(nl, dtype=np.int32), byte_cdf, *_ONE_BYTE_TABLE)
        else:
            indexes = (patterns.astype(np.int32)[:, None] * 8 + np.arange(8, dtype=np.int32)).reshape(-1)
            sym = _rans_decode(payload, indexes, _context_cdf(f1), _BINARY_SIZES, _BINARY_OFFSETS)
    except _lib.PccError as e:
        raise ValueError("PCO2: corrupt payload at level %d (%s)" % (level, e)) from None
    if mode == MODE_BYTES:
        if sym.min() < 0 or sym.max() > 254:
            raise ValueError("PCO2: corrupt payload at level %d" % level)
        return (sym + 1).astype(np.uint8), pos
    if sym.min() < 0 or sym.max() > 1:
        raise ValueError("PCO2: corrupt payload at level %d" % level)
    return np.packbits(sym.astype(np.uint8).reshape(nl, 8), axis=1, bitorder="little").reshape(nl), pos


def level_modes(data):
    """PCO2 bytes -> the mode of every level (a walk over the framing; nothing is decoded)"""
    data = bytes(data)
    if len(data) < 28 or data[:4] != MAGIC_CONTEXTS or data[4] > 21:
        raise ValueError("not a PCO2 coordinate stream")
    depth = data[4]
    sizes, pos = _take(data, 28, 4 * depth, "header")
    modes = []
    for l, nl in enumerate(struct.unpack("<%dI" % depth, sizes)):
        mode, pos = _take(data, pos, 1, "level %d" % l)
        modes.append(mode[0])
        if mode[0] > MODE_BYTES:
            raise ValueError("PCO2: mode %d at level %d" % (mode[0], l))
        if mode[0] == MODE_RAW:
            pos += nl
            continue
        if mode[0] == MODE_EXPLICIT:
            bitmap, pos = _take(data, pos, _CONTEXTS // 8, "context bitmap at level %d" % l)
            pos += 2 * int(np.unpackbits(np.frombuffer(bitmap, dtype=np.uint8)).sum())
        elif mode[0] == MODE_BYTES:
            _, pos = _read_varints(data, pos, 256)
        length, pos = _take(data, pos, 4, "payload length at level %d" % l)
        pos += struct.unpack("<I", length)[0]
    if pos != len(data):
        raise ValueError("PCO2: the levels end at byte %d of %d" % (pos, len(data)))
    return modes


def _decode_contexts(data, device, batch):
    L = _lib.lib()
    depth, _, _, stride, ox, oy, oz, n = struct.unpack("<BBHi3iI", data[4:28])
    if depth > 21 or stride < 1 or n >= 1 << 31:
        raise ValueError("PCO2: bad header")
    sizes, pos = _take(data, 28, 4 * depth, "header")
    cnt = np.array(struct.unpack("<%dI" % depth, sizes), dtype=np.int64)
    if n == 0 or depth == 0:
        if depth or n > 1 or pos != len(data):
            raise ValueError("PCO2: bad header")
        if n == 0:
            return torch.zeros((0, 4), dtype=torch.int32, device=device)
    elif cnt[0] != 1:
        raise ValueError("PCO2: the root level must hold one node")
    origin = np.array([ox, oy, oz], dtype=np.int32)
    stream = _lib.stream()
    keys = torch.zeros(1, dtype=torch.int64, device=device)             # the root: prefix 0
    state = np.zeros((_CONTEXTS, 2), dtype=np.int64)
    for l in range(depth):
        nl = int(cnt[l])                                                # == the size of `keys`: checked one level up
        nxt = int(cnt[l + 1]) if l + 1 < depth else n
        pat_dev = torch.empty(nl, dtype=torch.uint8, device=device)
        check(L.pcc_octree_patterns(ptr(keys), nl, l, ptr(pat_dev), stream))
        patterns = _to_host(pat_dev, "octree_pat")
        occ, pos = _decode_level(data, pos, nl, patterns, state, l)
        if occ.min() == 0:
            raise ValueError("PCO2: an empty node at level %d" % l)
        if int(np.unpackbits(occ).sum()) != nxt:
            raise ValueError("PCO2: the occupancy of level %d does not match the size of the next" % l)
        state = (state >> 1) + _level_hist(occ, patterns)
        occ_dev = _to_device(occ, device, "octree_occ_up")
        nbytes = L.pcc_octree_scratch_bytes(nl)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        children = torch.empty(nxt, dtype=torch.int64, device=device)
        check(L.pcc_octree_expand_level(ptr(keys), ptr(occ_dev), nl, nxt, ptr(children), ptr(scratch), nbytes, stream))
        keys = children
    if pos != len(data):
        raise ValueError("PCO2: %d bytes behind the last level" % (len(data) - pos))
    out = torch.empty((n, 4), dtype=torch.int32, device=device)
    check(L.pcc_octree_keys_to_coords(ptr(keys), n, stride, ptr(origin), int(batch), ptr(out), stream))
    return out


def decode_coordinates(data, device, batch=0):
    """bytes (PCO1 or PCO2) -> int32 [N,4] = (batch, x, y, z) on ``device``, ascending Morton order."""
    L = _lib.lib()
    data = bytes(data)
    if len(data) >= 28 and data[:4] == MAGIC_CONTEXTS:
        return _decode_contexts(data, device, batch)
    if len(data) < 28 or data[:4] != MAGIC:
        raise ValueError("not a PCO1 coordinate stream")
    depth, _, _, stride, ox, oy, oz, n = struct.unpack("<BBHi3iI", data[4:28])
    if depth > 21 or stride < 1:
        raise ValueError("PCO1: bad header")
    pos = 28
    if len(data) < pos + 5 * depth + 4:
        raise ValueError("PCO1: truncated header")
    cnt = np.array(struct.unpack("<%dI" % depth, data[pos:pos + 4 * depth]), dtype=np.int64)
    pos += 4 * depth
    flags = data[pos:pos + depth]
    pos += depth
    cdf = np.zeros((max(depth, 1), 257), dtype=np.int32)
    for l in range(depth):
        if flags[l]:
            freqs, pos = _read_varints(data, pos, 256)
            if freqs.min() < 1 or freqs.sum() != 1 << _PRECISION:
                raise ValueError("PCO1: invalid frequency table at level %d" % l)
            cdf[l, 1:] = np.cumsum(freqs)
        else:
            cdf[l] = _flat_cdf()
    (plen,) = struct.unpack("<I", data[pos:pos + 4])
    pos += 4
    payload = data[pos:pos + plen]
    if len(payload) != plen:
        raise ValueError("PCO1: truncated payload")
    if n == 0:
        return torch.zeros((0, 4), dtype=torch.int32, device=device)
    out = torch.empty((n, 4), dtype=torch.int32, device=device)
    origin = np.array([ox, oy, oz], dtype=np.int32)
    occ_dev = torch.zeros(1, dtype=torch.uint8, device=device)
    if depth:
        indexes = np.repeat(np.arange(depth, dtype=np.int32), cnt)
        sym = _rans_decode(payload, indexes, cdf, np.full(depth, 257, dtype=np.int32), np.zeros(depth, dtype=np.int32))
        if sym.min() < 0 or sym.max() > 254:
            raise ValueError("PCO1: corrupt payload")
        occ = (sym + 1).astype(np.uint8)
        # every level's popcounts must add up to the size of the next (the last to n_points)
        pop = np.unpackbits(occ[:, None], axis=1).sum(axis=1)
        ends = np.cumsum(cnt)
        want = np.append(cnt[1:], n)
        got = np.add.reduceat(pop, np.concatenate([[0], ends[:-1]]))
        if cnt[0] != 1 or (got != want).any():
            raise ValueError("PCO1: occupancy does not match the level sizes")
        occ_dev = torch.from_numpy(occ).to(device)
    nbytes = L.pcc_octree_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
    counts64 = np.ascontiguousarray(cnt if depth else np.zeros(1), dtype=np.int64)
    check(L.pcc_octree_expand(ptr(occ_dev), ptr(counts64), depth, stride, ptr(origin), int(batch), n, ptr(out), ptr(scratch),
                              nbytes, _lib.stream()))
    return out
