"""Case tables, input builders and numpy references for tests/test_select_paths.py: the top-k selection (csrc/select.hip,
pcc_topk_mask), the row compaction and its three-kernel scan (csrc/coords.hip, pcc_compact_rows) and the small row kernels
beside them.  Host only: numpy and the oracle's coordinate key; nothing here imports the GPU library.

The references are the documented contract (include/pcc_hip.h) written out: rows ordered by the order-preserving key of the
fp32 logit (oracle.coords.float_key: NaN on top, -0 == +0), descending, exact ties by ascending voxel key; item b keeps
max(0, min(k[b], count_b)) rows; rows whose item index is outside [0, nbatch) are never selected and never counted.
"""
import collections

import numpy as np

from oracle import coords as oc
from oracle.coords import float_key          # ONE key for the oracle (oracle/codec.py:topk_mask) and these references

__all__ = ["float_key", "reference_topk", "reference_compact"]

# ---- the constants of the launch code the tables are built around (the table test checks the tables against THESE) ----------
TK_SMALL_N = 32768                     # csrc/select.hip:286  TK_SMALL_N: one workgroup up to here (one item)
TK_LDS_BATCHES = 16                    # csrc/select.hip:30   TK_LDS_BATCHES: LDS histogram up to here, global atomics above
TK_GRID_ROWS = 512 * 256               # csrc/select.hip:610  blocks_for(n, 256, 512): topk_hist strides above this row count
TK1_ROWS_PER_ITER = 256 * 1024 * 4     # csrc/select.hip:162-163,174  TK1_GROUPS x TK1_THREADS x 4 rows: topk_hist1_kernel loops above
TOPK_SMALL_BIT = 2                     # include/pcc_hip.h:192  bit of pcc_small_paths that allows the one-item kernels
BATCH_MAX = 1023                       # csrc/common.h:53     BATCH_LIMIT + 1 items (csrc/select.hip:598)
SCAN_TILE = 1024                       # csrc/coords.hip:29-31  SCAN_BLOCK x SCAN_ITEMS flags per workgroup
SCAN_SECOND_ROWS = 256 * SCAN_TILE     # csrc/coords.hip:82   scan_of_block_sums takes SCAN_BLOCK block sums per iteration
ROW_GRID_ELEMS = 65536 * 256           # csrc/coords.hip:865,873,881  blocks_for(n * c, 256, 65536): the row movers stride above
PAIR_GRID_ROWS = 512 * 256             # csrc/coords.hip:856  blocks_for(n, 256 * 16, 512) groups of 256 threads
COUNT_WAVE = 64                        # csrc/coords.hip:718-732  count_batch_kernel ballots within a wave of 64 rows


# ---- references -------------------------------------------------------------------------------------------------------------
def topk_order(logits, coords, nbatch):
    """the documented order of all rows at once: (rows, item, rank within the item, rows per item)"""
    coords = np.asarray(coords)
    b = coords[:, 0].astype(np.int64)
    idx = np.nonzero((b >= 0) & (b < nbatch))[0]
    fk = float_key(np.asarray(logits)[idx]).astype(np.int64)
    ck = oc.pack(coords[idx])
    order = np.lexsort((ck, -fk, b[idx]))
    rows = idx[order]
    item = b[rows]
    counts = np.bincount(item, minlength=nbatch).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = np.arange(rows.size, dtype=np.int64) - start[item]
    return rows, item, rank, counts


def reference_topk(logits, coords, ks, nbatch, order=None):
    """uint8 mask [n] of the documented selection; ``order``: a topk_order() of the same rows (shared among the k values)"""
    rows, item, rank, counts = order if order is not None else topk_order(logits, coords, nbatch)
    ks = np.asarray(ks, dtype=np.int64)
    assert ks.shape == (nbatch,)
    keep = np.clip(np.minimum(ks, counts), 0, None)
    mask = np.zeros(np.asarray(coords).shape[0], dtype=np.uint8)
    mask[rows[rank < keep[item]]] = 1
    return mask


def kept_per_item(mask, coords, nbatch):
    b = np.asarray(coords)[:, 0]
    ok = (b >= 0) & (b < nbatch) & (mask != 0)
    return np.bincount(b[ok], minlength=nbatch).astype(np.int64)


def reference_compact(mask, coords=None, feats=None):
    """boolean indexing: (kept coords, kept feats, new_index, count)"""
    keep = np.asarray(mask) != 0
    new_index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return (coords[keep] if coords is not None else None, feats[keep] if feats is not None else None, new_index, int(keep.sum()))


# ---- coordinates ------------------------------------------------------------------------------------------------------------
def build_coords(n, nbatch=1, seed=0, empty=None, strays=False):
    """[n, 4] int32 rows, all distinct, negative coordinates included.  The voxels are an affine bijection of a 256^3 cube
    (odd multiplier modulo 2^24), stretched so that the fields of the voxel key differ in high and low bytes.  Several
    items: the rows of the items are interleaved at random with uneven shares, item ``empty`` gets none, and with ``strays``
    about one row in fifty carries item index -1 or nbatch."""
    rng = np.random.default_rng([n, nbatch, seed, 1])
    i = np.arange(n, dtype=np.int64)
    a = 2 * int(rng.integers(1 << 20, 1 << 23)) + 1
    flat = (a * i + int(rng.integers(0, 1 << 24))) & ((1 << 24) - 1)
    c = np.empty((n, 4), dtype=np.int32)
    c[:, 1] = ((flat >> 16) - 128) * 389
    c[:, 2] = ((flat >> 8) & 255) - 128
    c[:, 3] = ((flat & 255) - 100) * 3
    if nbatch == 1:
        c[:, 0] = 0
        return c
    live = np.array([b for b in range(nbatch) if b != empty])
    w = rng.random(live.size) + 0.2
    c[:, 0] = rng.choice(live, size=n, p=w / w.sum())
    if strays:
        m = max(1, n // 100)
        pos = rng.permutation(n)[:2 * m]
        c[pos[:m], 0] = -1
        c[pos[m:], 0] = nbatch
    return c


# ---- logits -----------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "ties", "all_equal", "two_values", "specials", "same_exponent")
FLT_MAX_BITS, FLT_MIN_BITS = 0x7F7FFFFF, 0x00800000
DENORMAL = np.float32(1e-40)
# NaN of both signs and two payloads (one of them signalling), +-inf, +-1e-40 (denormal), +-FLT_MAX, FLT_MIN — as bit patterns
SPECIAL_BITS = (0x7FC00000, 0xFFC00000, 0x7FC00123, 0xFF800001, 0x7F800000, 0xFF800000,
                int(DENORMAL.view(np.uint32)), int(DENORMAL.view(np.uint32)) | 0x80000000,
                FLT_MAX_BITS, FLT_MAX_BITS | 0x80000000, FLT_MIN_BITS)


def build_logits(family, n, seed=0):
    """float32 [n] of one family (module docstring of the test)"""
    rng = np.random.default_rng([n, seed, FAMILIES.index(family) if family in FAMILIES else 99, 2])
    v = rng.normal(size=n).astype(np.float32)
    if family == "normal":
        return v
    if family in ("ties", "mixed"):
        v[rng.integers(0, n, n // 3)] = 0.25                     # a third of the rows: exact ties, broken by the voxel key
        v[rng.integers(0, n, n // 20 + 1)] = -0.0
        v[rng.integers(0, n, n // 20 + 1)] = 0.0
        if family == "mixed":                                    # (several items) a few NaN and infinities on top
            u = v.view(np.uint32)
            for j, bits in enumerate(SPECIAL_BITS[:6]):
                u[rng.integers(0, n, n // 60 + 1)] = bits
        return v
    if family == "all_equal":
        return np.full(n, -1.5, dtype=np.float32)
    if family == "two_values":
        return rng.choice(np.array([0.25, -1.5], dtype=np.float32), size=n)
    if family == "specials":
        # every special value on m rows of its own: with 4 m NaN rows, m rows of +inf and m denormals, the k values of the
        # case (ks_for) fall strictly inside each of these groups from m >= 2 on
        m = max(3, n // 40) if n >= 63 else 1
        u = v.view(np.uint32)
        pos = rng.permutation(n)
        for j, bits in enumerate(SPECIAL_BITS):
            u[pos[j * m:(j + 1) * m]] = bits
        return v
    if family == "same_exponent":
        # 1.0 + j 2^-23, j < 256: the first three bytes of the key are the same for every row (one bin per radix pass)
        return (np.uint32(0x3F800000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    raise ValueError(family)


def tie_values(family):
    """the logit values of a family that many rows share: the k values of a case straddle each of these groups"""
    return {"ties": (0.25, 0.0), "mixed": (0.25,), "all_equal": (-1.5,), "two_values": (0.25, -1.5),
            "specials": (float("nan"), float("inf"), float(DENORMAL)),
            "same_exponent": (float(np.float32(1.0) + np.float32(128 * 2.0 ** -23)),)}.get(family, ())


def tie_group(logits, value):
    """(rows above the group, rows in it) in the documented order"""
    fk, key = float_key(logits), float_key(np.array([value], dtype=np.float32))[0]
    return int((fk > key).sum()), int((fk == key).sum())


def ks_for(logits, family):
    """the k values every top-k case uses, for the rows of ONE item"""
    count = int(np.asarray(logits).shape[0])
    ks = [0, -3, 1, count // 3, count - 1, count, count + 5]
    for value in tie_values(family):
        n_above, n_tie = tie_group(logits, value)
        if n_tie:
            ks += [n_above, n_above + 1, n_above + n_tie // 2]
    return list(dict.fromkeys(ks))


def k_vectors(logits, coords, nbatch, empty):
    """the k vectors of a case with several items.  Every value of ks_for reaches some item; vector 3 mixes items that
    resolve in pass 0 (k >= count), items whose boundary lies inside the 0.25 ties (resolved by the voxel key, up to pass 11)
    and plain ones; the empty item always has k > 0."""
    b = coords[:, 0]
    per = [logits[b == i] for i in range(nbatch)]
    count = np.array([p.shape[0] for p in per], dtype=np.int64)
    groups = [tie_group(p, 0.25) if p.shape[0] else (0, 0) for p in per]
    above = np.array([g[0] for g in groups], dtype=np.int64)
    tie = np.array([g[1] for g in groups], dtype=np.int64)
    i = np.arange(nbatch)
    vecs = [count // 3,
            np.choose(i % 3, [np.zeros_like(count), np.full_like(count, -3), np.ones_like(count)]),
            np.choose(i % 3, [count - 1, count, count + 5]),
            np.choose(i % 3, [count + 5, above + tie // 2, count // 3]),
            np.choose(i % 2, [above, above + 1])]
    if empty is not None:
        for v in vecs:
            v[empty] = 7
    return [v.astype(np.int32) for v in vecs]


# ---- the top-k table --------------------------------------------------------------------------------------------------------
TopkCase = collections.namedtuple("TopkCase", "id path n nbatch family ld small empty")
PATHS = ("small", "large1", "generic1", "lds", "global")
SMALL_ROWS = (1, 63, 64, 65, 1023, 1025, 32768)
LARGE1_ROWS = (32769, 150001, 1048577, 1100003)
GENERIC1_ROWS = (65, 32768, 131073)
LDS_ITEMS, LDS_ROWS = (2, 3, 16), (300, 40000, 131073 + 7)
GLOBAL_ITEMS, GLOBAL_ROWS = (17, 64, 1023), (5000, 140001)


def topk_path(nbatch, n, small_paths):
    """pcc_topk_mask's choice (csrc/select.hip:596-633), from the constants above"""
    one_item_kernels = bool(small_paths & TOPK_SMALL_BIT) and nbatch == 1
    if one_item_kernels and 0 < n <= TK_SMALL_N:
        return "small"
    if one_item_kernels:
        return "large1"
    if nbatch == 1:
        return "generic1"
    return "lds" if nbatch <= TK_LDS_BATCHES else "global"


def _topk_cases():
    out = []

    def add(path, n, nbatch, family, ld, small=True, empty=None):
        out.append(TopkCase(f"{path}-n{n}-b{nbatch}-{family}-ld{ld}", path, n, nbatch, family, ld, small, empty))

    for i, n in enumerate(SMALL_ROWS):
        for j, family in enumerate(FAMILIES):
            add("small", n, 1, family, (1, 5)[(i + j) % 2])
    large = {32769: (("ties", 1), ("specials", 2), ("same_exponent", 1), ("all_equal", 2)),      # all_equal here only: its tail
             150001: (("ties", 2), ("specials", 1), ("same_exponent", 2)),                       # walks all rows eight times in one CU
             1048577: (("ties", 1), ("specials", 2), ("same_exponent", 2)),
             1100003: (("same_exponent", 1), ("specials", 1), ("ties", 2))}
    for n in LARGE1_ROWS:
        for family, ld in large[n]:
            add("large1", n, 1, family, ld)
    for i, n in enumerate(GENERIC1_ROWS):
        for j, family in enumerate(("ties", "specials")):
            add("generic1", n, 1, family, (1, 2)[(i + j) % 2], small=False)
    for path, items, rows in (("lds", LDS_ITEMS, LDS_ROWS), ("global", GLOBAL_ITEMS, GLOBAL_ROWS)):
        for i, nbatch in enumerate(items):
            for j, n in enumerate(rows):
                # two items cannot hold an empty one beside a resolved and a tied one: the smallest case has it, the others not
                empty = (1 if j == 0 else None) if nbatch == 2 else nbatch // 2
                add(path, n, nbatch, "mixed", (1, 3)[(i + j) % 2], empty=empty)
    return out


TOPK_CASES = _topk_cases()


def topk_inputs(case):
    """(logit column [n], coords [n, 4], list of k vectors [nbatch] int32)"""
    coords = build_coords(case.n, case.nbatch, seed=3, empty=case.empty, strays=case.nbatch > 1)
    logits = build_logits(case.family, case.n, seed=5)
    if case.nbatch == 1:
        ks = [np.array([k], dtype=np.int32) for k in ks_for(logits, case.family)]
    else:
        ks = k_vectors(logits, coords, case.nbatch, case.empty)
    return logits, coords, ks


# ---- the compaction table ---------------------------------------------------------------------------------------------------
CompactCase = collections.namedtuple("CompactCase", "id n mask c coords feats index offset")
COMPACT_ROWS = (0, 1, 1023, 1024, 1025, 262144, 262145, 524289)
MASK_KINDS = ("none", "all", "last", "first", "random", "bytes")
COMPACT_C = (0, 1, 3, 4, 6, 64)
NULL_COMBOS = tuple((c, f, x) for c in (True, False) for f in (True, False) for x in (True, False))


def build_mask(kind, n, seed=0):
    rng = np.random.default_rng([n, seed, MASK_KINDS.index(kind), 3])
    m = np.zeros(n, dtype=np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "last":
        m[n - 1:] = 1
    elif kind == "first":
        m[:1] = 1
    elif kind == "random":
        m[:] = rng.random(n) < 0.3
    elif kind == "bytes":                      # any non-zero byte counts as set
        m[:] = rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=n)
    return m


def _compact_cases():
    out = []
    for i, n in enumerate(COMPACT_ROWS):
        for j, kind in enumerate(MASK_KINDS):
            c = COMPACT_C[(i + j) % len(COMPACT_C)]
            has_c, has_f, has_x = NULL_COMBOS[(i * len(MASK_KINDS) + j) % len(NULL_COMBOS)]
            has_f = has_f and c > 0
            out.append(CompactCase(f"n{n}-{kind}-c{c}-{'C' if has_c else '_'}{'F' if has_f else '_'}{'X' if has_x else '_'}",
                                   n, kind, c, has_c, has_f, has_x, 0))
    return out


COMPACT_CASES = _compact_cases()
# c = 4 with the features one float off a 16-byte boundary: the scalar copy where c % 4 == 0 (csrc/coords.hip:905)
MISALIGNED_ROWS = (1025, 262145)

# ---- the row kernels --------------------------------------------------------------------------------------------------------
COUNT_ITEMS = (1, 3, 64, 65, 1023)
COUNT_ROWS = (1, 63, 65, 257, 100003)
PAIR_ROWS = (1, 4095, 4097, 2097153)
MOVER_SHAPES = ((1, 1), (257, 3), (5000, 24), (131073, 128))


def popcount_sum(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)).sum(dtype=np.int64))
