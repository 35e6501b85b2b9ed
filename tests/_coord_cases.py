"""Case tables, input builders and numpy references for tests/test_coord_paths.py: the hashed-voxel table (csrc/common.h
table_claim / table_find, csrc/coords.hip pcc_hash_build / pcc_hash_lookup / pcc_stride_map) and the kernel maps built from it
(csrc/coords.hip pcc_kernel_map, csrc/select.hip pcc_small_kernel_map).  Host only: numpy and the oracle's coordinate algebra;
nothing here imports the GPU library.

The references are oracle.coords (pack, lookup, kernel_map, kernel_offsets: sorted keys and a binary search, no hash) and, for
the execution order, the stable sort of order_key below — the one restatement of the key of csrc/select.hip, which
tests/test_hip_parity.py imports from here.
"""
import collections

import numpy as np

from oracle import coords as oc

# ---- the constants of the library the cases are built around (test_constants_are_the_librarys holds them to the header) ------
COORD_LIMIT = 130000                   # include/pcc_hip.h  PCC_COORD_LIMIT
BATCH_LIMIT = 1022                     # include/pcc_hip.h  PCC_BATCH_LIMIT
BATCH_EDGES = (0, 511, 512, 1022)      # bit 63 of the voxel key is set from item 512 on; 1022 is the last item
MAP_BLOCK_ROWS = 64                    # csrc/coords.hip    one 256-thread workgroup per 64 output rows (both map kernels)
SMALL_MAP_MAX = 256                    # csrc/select.hip    SMALL_MAP_MAX: the one-launch map (pcc_small_map_max())
PROBE_STEP = 8                         # csrc/common.h      TABLE_PROBE_STEP: a key's lane is every 8th slot from its first one
UNIQUE_SMALL_BIT = 4                   # include/pcc_hip.h  bit of pcc_small_paths: coordinate sets in one workgroup


# ---- references -------------------------------------------------------------------------------------------------------------
def order_key(masks):
    """the execution-order key of csrc/select.hip: the 27-bit neighbour mask read with the rarest offset as the most
    significant bit (ties: lower offset first), descending"""
    masks = np.asarray(masks, dtype=np.int64) & 0x7FFFFFF
    cnt = np.array([int(((masks >> b) & 1).sum()) for b in range(27)])
    pos = [26 - sum(1 for o in range(27) if cnt[o] < cnt[b] or (cnt[o] == cnt[b] and o < b)) for b in range(27)]
    key = np.zeros(masks.shape[0], dtype=np.int64)
    for b in range(27):
        key |= ((masks >> b) & 1) << pos[b]
    return 0x7FFFFFF - key


def reference_map(in_coords, out_coords, ksize, step, sign):
    """(nbr int32 [n_out, K], row_mask uint32 [n_out], pairs) of include/pcc_hip.h's kernel map: nbr[j, k] = the input row at
    c_out + sign * off_k * step or -1, bit k of row_mask[j] set iff nbr[j, k] >= 0, pairs = the number of hits"""
    nbr = oc.kernel_map(in_coords, out_coords, ksize, step, transposed=sign < 0)
    mask = ((nbr >= 0).astype(np.int64) << np.arange(nbr.shape[1])).sum(axis=1)
    return nbr.astype(np.int32), mask.astype(np.uint32), int((nbr >= 0).sum())


def reference_order(row_mask):
    """(order int32 [n], group_mask32 uint32 [ceil(n / 32)]): THE stable ascending sort of the order key, and the OR of the
    masks over every 32 positions of it"""
    m = np.asarray(row_mask).astype(np.int64)
    n = m.shape[0]
    order = np.argsort(order_key(m), kind="stable")
    tiles = np.concatenate([m[order], np.zeros((-n) % 32, np.int64)]).reshape(-1, 32)
    return order.astype(np.int32), np.bitwise_or.reduce(tiles, axis=1).astype(np.uint32) if n else np.zeros(0, np.uint32)


def first_lookup(table_coords, query):
    """oracle.coords.lookup: with duplicate table rows the stable sort and the left binary search give the smallest row"""
    return oc.lookup(table_coords, query).astype(np.int32)


def popcount(words):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1).astype(np.int64)


def capacity_for(n):
    """the smallest capacity the entry points accept: a power of two >= 2 n (pcc_hash_capacity never goes below 1,024)"""
    cap = PROBE_STEP
    while cap < 2 * n:
        cap *= 2
    return cap


def map_kernel(ksize, step, sign):
    """pcc_kernel_map's choice (csrc/coords.hip): kernel size 3 takes kernel_map27_kernel, <true> unless the parent pitch
    2 * step of a transposed map is no power of two; sizes 1 and 2 take the generic kernel"""
    if ksize != 3:
        return "kernel_map_kernel"
    pitch = 0 if sign > 0 else 2 * step
    return "kernel_map27_kernel<true>" if pitch & (pitch - 1) == 0 else "kernel_map27_kernel<false>"


def table_shift(tensor_stride):
    """csrc/common.h grid_shift_of: log2 for powers of two, else 0"""
    return int(tensor_stride).bit_length() - 1 if tensor_stride & (tensor_stride - 1) == 0 else 0


# ---- coordinate sets --------------------------------------------------------------------------------------------------------
BLOCK27 = (-7, 5, -3)                  # centre of a full 3 x 3 x 3 block (grid units), in the first two items
LONELY = (40, -40, 37)                 # a voxel with no neighbour in its own item; the next item holds its +x neighbour
SHARED8 = (10, 10, -10)                # corner of a 2 x 2 x 2 block that EVERY item holds at the same xyz
FAR = (90, -90, 90)                    # (grid units) nothing of any set lies within 30 steps of it


def _planted(items, grid, limits):
    a, b = items[0], items[1 % len(items)]
    rows = []
    for item in dict.fromkeys((a, b)):
        rows += [(item, BLOCK27[0] + i, BLOCK27[1] + j, BLOCK27[2] + k) for i in (0, -1, 1) for j in (0, -1, 1) for k in (0, -1, 1)]
    rows.append((a, *LONELY))
    if b != a:
        rows.append((b, LONELY[0] + 1, LONELY[1], LONELY[2]))
    for item in items:
        rows += [(item, SHARED8[0] + i, SHARED8[1] + j, SHARED8[2] + k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    if limits:
        top = COORD_LIMIT // grid
        for axis in range(3):
            for s in (1, -1):
                for g in (top, top - 1):                     # the row at the limit and its neighbour on the inside
                    cell = [3 * axis + 1, -2 * axis - 5, 7 - axis]
                    cell[axis] = s * g
                    rows.append((a, *cell))
        rows += [(a, top, -top, top), (a, top - 1, -top + 1, top - 1)]      # a corner: every field of the key at its end
    return rows


def build_set(n, grid=1, seed=0, items=(0, 1, 2), limits=False):
    """[n, 4] int32 rows, all distinct, every coordinate a multiple of ``grid``, both signs, in random order.  Planted first
    (so a set of at least planted_rows() rows holds all of it): a full 3 x 3 x 3 block in the first two items at the same xyz,
    a lonely voxel whose +x neighbour exists in the next item only, a 2 x 2 x 2 block that every item holds at the same xyz
    and, with ``limits``, rows at +-COORD_LIMIT on each axis with their neighbours on the inside.  The rest: blobs of 1 to 27
    voxels (isolated voxels, lines, partly filled blocks) at random places of a 60^3 cube in random items."""
    rng = np.random.default_rng([n, grid, seed, len(items), 7])
    seen = dict.fromkeys(_planted(items, grid, limits)[:n])
    while len(seen) < n:
        item = items[int(rng.integers(0, len(items)))]
        cx, cy, cz = (int(v) for v in rng.integers(-30, 31, 3))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            cells = [(0, 0, 0)]
        elif kind == 1:
            axis = int(rng.integers(0, 3))
            cells = [tuple(t if a == axis else 0 for a in range(3)) for t in range(int(rng.integers(2, 6)))]
        else:
            r = (0, 1) if kind == 2 else (-1, 0, 1)
            keep = rng.random(len(r) ** 3) < (0.9 if kind == 2 else 0.6)
            cells = [c for c, k in zip([(i, j, k) for i in r for j in r for k in r], keep) if k]
        for dx, dy, dz in cells:
            if len(seen) < n:
                seen.setdefault((item, cx + dx, cy + dy, cz + dz))
    c = np.array(list(seen), dtype=np.int64).reshape(-1, 4)
    c[:, 1:] *= grid
    return c[rng.permutation(n)].astype(np.int32)


def planted_rows(items, limits):
    return len(dict.fromkeys(_planted(items, 1, limits)))


def shuffled(c, seed):
    return np.ascontiguousarray(c[np.random.default_rng([c.shape[0], seed, 9]).permutation(c.shape[0])]).astype(np.int32)


def in_range(c):
    return (np.abs(c[:, 1:].astype(np.int64)) <= COORD_LIMIT).all(axis=1)


def out_down(c, ts, seed=0):
    """the output set of a stride-2 convolution, rows in random order"""
    return shuffled(oc.stride_map(c, ts), seed)


def out_children(c, ts, ksize, seed=0):
    """the output set of a generative transposed convolution (parents of stride ts), rows in random order; a parent at the
    limit keeps the children that stay inside the key range"""
    ch = oc.children(c, ts, ksize)
    return shuffled(ch[in_range(ch)], seed)


def out_cross(c, step, seed=0):
    """another set of the same stride: every row of ``c`` as it is, shifted by (+step, 0, 0) and shifted by (0, -step, +step)
    (what stays in range, once each), and one row far from everything: no neighbour at all"""
    c = c.astype(np.int64)
    far = np.array([[c[0, 0], FAR[0] * step, FAR[1] * step, FAR[2] * step]], dtype=np.int64)
    rows = np.concatenate([c, c + [0, step, 0, 0], c + [0, 0, -step, step], far])
    rows = rows[in_range(rows)]
    return shuffled(oc.unpack(np.unique(oc.pack(rows))), seed)


# ---- the kernel-map table ---------------------------------------------------------------------------------------------------
# kind: same (out = in), down (out = stride map of in), cross (another set of the same stride), up (out = children of in:
# a transposed map, sign -1, step = ts / 2).  ts: the stride NAMED to the table and the map; grid: the pitch the coordinates
# really have (ts unless the case is about a foreign stride).  n: input rows.  n_out: None = the whole derived set, else its
# first n_out rows (the derived sets are larger than every boundary that is asked for: map_inputs asserts it).
MapCase = collections.namedtuple("MapCase", "id path kind ts grid n items limits ksize n_out")
BOUNDARY_ROWS = (1, 63, 64, 65, 127, 255, 256, 257, 1003)      # 1003: 16 workgroups, the last one with 43 rows
SMALL_ROWS = (1, 63, 64, 65, 127, 255, 256)
PATHS = ("kernel_map27_kernel<true>", "kernel_map27_kernel<false>", "kernel_map_kernel", "small_map_kernel<3>", "small_map_kernel<2>")


def case_step_sign(case):
    return (case.ts // 2, -1) if case.kind == "up" else (case.ts, 1)


def _map_cases():
    out = []

    def add(path, kind, ts, n, ksize=3, items=(0, 1, 2), limits=False, n_out=None, grid=None, tag=""):
        small = path.startswith("small")
        name = {True: "small%d" % ksize, False: {"kernel_map27_kernel<true>": "k27pow2", "kernel_map27_kernel<false>": "k27mod",
                                                 "kernel_map_kernel": "generic%d" % ksize}.get(path)}[small]
        cid = f"{name}-{kind}{tag}-ts{ts}-n{n}" + ("" if n_out is None else f"-out{n_out}") + ("-limits" if limits else "")
        out.append(MapCase(cid, path, kind, ts, grid or ts, n, tuple(items), limits, ksize, n_out))

    P27, N27, GEN, S3, S2 = PATHS
    # kernel_map27_kernel<true>: same / down / cross at strides 1, 2, 8; up3 at steps 1, 2, 8
    add(P27, "same", 1, 700, limits=True)
    add(P27, "same", 2, 1100, items=(0, 1), limits=True)
    add(P27, "same", 8, 1500, items=BATCH_EDGES, limits=True)
    add(P27, "down", 1, 900, limits=True)
    add(P27, "down", 2, 900, items=BATCH_EDGES)
    add(P27, "down", 8, 900, items=(0, 1), limits=True)
    add(P27, "cross", 1, 600, items=BATCH_EDGES, limits=True)
    add(P27, "cross", 2, 600)
    add(P27, "cross", 8, 600, items=(0, 1), limits=True)
    add(P27, "up", 2, 160, limits=True)
    add(P27, "up", 4, 160, items=BATCH_EDGES)
    add(P27, "up", 16, 160, items=(0, 1), limits=True)
    add(P27, "same", 3, 500, tag="-shift0")                          # not a power of two: the table's shift is 0
    add(P27, "cross", 1, 400, grid=8, tag="-grid8")                  # multiples of 8 under a table and a map that name stride 1
    add(P27, "cross", 8, 800, grid=1, tag="-grid1")                  # arbitrary integers under a table and a map that name stride 8
    for n_out in (0,) + BOUNDARY_ROWS:
        add(P27, "cross", 2, 600, n_out=n_out)
    for n_out in (1, 64, 65, 257):
        add(P27, "up", 4, 160, n_out=n_out)
    # kernel_map27_kernel<false>: a transposed map whose parent pitch is no power of two
    add(N27, "up", 6, 160, limits=True)
    add(N27, "up", 6, 160, items=BATCH_EDGES, n_out=1003)
    for n_out in (1, 65, 257):
        add(N27, "up", 6, 160, n_out=n_out)
    # the generic kernel: kernel sizes 2 (both signs) and 1
    add(GEN, "up", 2, 300, ksize=2, limits=True)
    add(GEN, "up", 8, 300, ksize=2, items=BATCH_EDGES)
    add(GEN, "up", 6, 300, ksize=2, items=(0, 1))                    # the runtime-pitch modulo with a pitch that is no power of two
    add(GEN, "down", 1, 900, ksize=2, limits=True)
    add(GEN, "down", 8, 900, ksize=2, items=BATCH_EDGES)
    add(GEN, "same", 2, 800, ksize=2)
    add(GEN, "cross", 1, 600, ksize=1, limits=True)
    add(GEN, "cross", 8, 600, ksize=1, items=BATCH_EDGES)
    for n_out in (0,) + BOUNDARY_ROWS:
        add(GEN, "up", 4, 300, ksize=2, n_out=n_out)
    # the one-launch map, kernel sizes 3 and 2
    add(S3, "same", 2, 200, limits=True)
    add(S3, "same", 1, 256, items=BATCH_EDGES)
    add(S3, "down", 1, 900, n_out=200, limits=True)
    add(S3, "up", 4, 160, n_out=250, items=BATCH_EDGES)
    add(S3, "up", 6, 160, n_out=250, limits=True)
    for n_out in (0,) + SMALL_ROWS:
        add(S3, "cross", 8, 600, n_out=n_out, items=(0, 1))
    add(S2, "down", 8, 900, ksize=2, n_out=200, limits=True)
    add(S2, "up", 6, 300, ksize=2, n_out=130, items=BATCH_EDGES)
    add(S2, "same", 1, 256, ksize=2)
    for n_out in (0,) + SMALL_ROWS:
        add(S2, "up", 2, 300, ksize=2, n_out=n_out)
    return out


MAP_CASES = _map_cases()
_INPUTS = {}


def map_inputs(case):
    """(input rows, output rows, kernel size, step, sign) of a case; computed once and shared (read only)"""
    if case.id not in _INPUTS:
        step, sign = case_step_sign(case)
        c = build_set(case.n, case.grid, seed=3, items=case.items, limits=case.limits)
        if case.kind == "same":
            out = c
        elif case.kind == "down":
            out = out_down(c, case.ts)
        elif case.kind == "up":
            out = out_children(c, case.ts, case.ksize)
        else:
            out = out_cross(c, step)
        if case.n_out is not None:
            assert out.shape[0] >= case.n_out, (case.id, out.shape[0])
            out = np.ascontiguousarray(out[:case.n_out])
        for a in (c, out):
            a.setflags(write=False)
        _INPUTS[case.id] = (c, out, case.ksize, step, sign)
    return _INPUTS[case.id]


_REFERENCES = {}


def map_reference(case):
    """reference_map of a case (and reference_order of its masks), computed once and shared (read only)"""
    if case.id not in _REFERENCES:
        c, out, ksize, step, sign = map_inputs(case)
        nbr, mask, pairs = reference_map(c, out, ksize, step, sign)
        order, gmask = reference_order(mask)
        for a in (nbr, mask, order, gmask):
            a.setflags(write=False)
        _REFERENCES[case.id] = (nbr, mask, pairs, order, gmask)
    return _REFERENCES[case.id]


# ---- the table cases --------------------------------------------------------------------------------------------------------
LOOKUP_SIZES = (0, 1, 255, 256, 257)             # one 256-thread workgroup of lookup_kernel, and one row more
SMALL_CAPS = (8, 16, 32, 64)                     # n = cap / 2 rows: a lane has 1, 2, 4 and 8 slots
POOL_ROWS, POOL_STRIDE = 4096, 2                 # the pool the full lanes are drawn from: even coordinates, stride 2 named
LANE_TABLE_CAP = 1024                            # the planted tables: 128 slots per lane
LANE_ROWS, LANE_ROWS_MIN = 300, 200              # rows of one lane put into such a table
STRIDE_PARENTS = 200                             # parents of one lane; two source rows each: 400 candidates


def pool_voxels():
    """POOL_ROWS distinct voxels of two items in a cube around the origin, every coordinate a multiple of POOL_STRIDE"""
    rng = np.random.default_rng(41)
    side = 24
    cell = rng.permutation(2 * side ** 3)[:POOL_ROWS]
    b, cell = cell // side ** 3, cell % side ** 3
    xyz = np.stack([cell % side, (cell // side) % side, cell // side ** 2], axis=1) - side // 2
    return np.concatenate([b[:, None], xyz * POOL_STRIDE], axis=1).astype(np.int32)


def cube_voxels(n, seed, items=(0, 511, 512), side=4):
    """n distinct random voxels of a side^3 cube around the origin, spread over ``items``: dense enough for neighbours, random
    enough for two keys to meet in one slot of a table of 2 n slots"""
    rng = np.random.default_rng([n, seed, side, 19])
    cell = rng.permutation(len(items) * side ** 3)[:n]
    b, cell = np.asarray(items)[cell // side ** 3], cell % side ** 3
    xyz = np.stack([cell % side, (cell // side) % side, cell // side ** 2], axis=1) - side // 2
    return np.concatenate([b[:, None], xyz], axis=1).astype(np.int32)


def with_duplicates(c, copies, seed=0):
    """``c`` (distinct rows) with ``copies`` more rows that repeat earlier ones — a fifth of them repeat a row that is repeated
    already — in random order: pcc_hash_build counts exactly ``copies`` duplicates"""
    rng = np.random.default_rng([c.shape[0], copies, seed, 11])
    src = rng.integers(0, c.shape[0], copies)
    src[copies - copies // 5:] = src[:copies // 5]
    return shuffled(np.concatenate([c, c[src]]), seed)


def slots_of(table_keys, coords):
    """the slot of every row of ``coords`` in a table read back from the device (uint64 keys, ~0 = empty), -1 = not in it"""
    keys = np.asarray(table_keys).view(np.uint64)
    order = np.argsort(keys, kind="stable")
    want = oc.pack(coords)
    pos = np.minimum(np.searchsorted(keys[order], want), keys.shape[0] - 1)
    return np.where(keys[order][pos] == want, order[pos], -1)


def fullest_lane(slots, rows):
    """(lane, the first ``rows`` row indices of it) for the most populated lane (slot & 7) of a table"""
    lanes = np.asarray(slots) & (PROBE_STEP - 1)
    lane = int(np.bincount(lanes, minlength=PROBE_STEP).argmax())
    return lane, np.nonzero(lanes == lane)[0][:rows]


def lane_is_full(table_keys, lane):
    """every slot of the lane holds a key"""
    keys = np.asarray(table_keys).view(np.uint64)
    return bool((keys[lane::PROBE_STEP] != np.uint64(0xFFFFFFFFFFFFFFFF)).all())


def stride_sources(parents, seed=0):
    """two distinct source rows (stride 1) for every parent of a stride-2 set, all rows in random order: [2 n, 4]"""
    rng = np.random.default_rng([parents.shape[0], seed, 13])
    first = rng.integers(0, 8, parents.shape[0])
    second = (first + rng.integers(1, 8, parents.shape[0])) % 8
    rows = []
    for corner in (first, second):
        off = np.stack([np.zeros_like(corner), corner & 1, (corner >> 1) & 1, corner >> 2], axis=1)
        rows.append(parents.astype(np.int64) + off)
    return shuffled(np.concatenate(rows), seed)


# queries outside the key range against a table of (0, 5, 4, 5) and (0, 5, 5, 4): their masked keys are those two voxels'
RANGE_TABLE = ((0, 5, 4, 5), (0, 5, 5, 4))
RANGE_QUERIES = ((0, 5 + (1 << 18), 4, 5), (0, 5, 5 - (1 << 18), 4), (1024, 5, 4, 5), (-1, 5, 4, 5))
