"""The hashed-voxel table and the kernel maps built from it, on every launch path and table state, held to EQUALITY with the numpy
references of tests/_coord_cases.py (oracle.coords: sorted keys and a binary search; the stable sort of order_key).  Integer
work throughout: no tolerances.  Everything goes through the C ABI (pcc.lib()), every device output lies between 64 sentinel
words, and the guards — and whatever a call must not write — keep the sentinel.

Kernel maps (MAP_CASES, one test each; the id names the path).  Input sets of 160 to 1,500 rows from a seeded builder: two to four
batch items that share xyz (a hit never crosses items), both signs, rows in random order, dense blocks and isolated voxels (a
row with all 27 neighbours, rows with one or none), items 0 / 511 / 512 / 1022 in one set, rows at +-PCC_COORD_LIMIT on each
axis at steps 1 and 8 (and 2, 3), children on all eight parity classes of the parent grid, tables and maps that name a stride
that is not the set's own.
  k27pow2   kernel_map27_kernel<true>: same / down / cross at strides 1, 2, 8, up3 at steps 1, 2, 8, a same-set map at
            stride 3 (shift 0)
  k27mod    kernel_map27_kernel<false>: up3 from parents of stride 6 (also through CoordMap(c, 6).up(3))
  generic   kernel_map_kernel: kernel size 2 with sign -1 (pitches 2, 8 and 6) and sign +1, kernel size 1 ([n, 1])
  small3/2  small_map_kernel<3> / <2> through pcc_small_kernel_map: nbr, row_mask, order and group_mask32 against the references
Output rows 0, 1, 63, 64, 65, 127, 255, 256, 257 and 1,003 (pcc_small_kernel_map: up to 256; 257 is refused and writes nothing).
pcc_kernel_map runs three times per case: row_mask and pair_count (pair_count_kernel), pair_count alone (the count inside the
map kernel), neither.

The table.  pcc_hash_build with planted duplicates (dup_count, the smallest row of each group) and pcc_hash_lookup of 0, 1,
255, 256, 257 queries; capacities 8, 16, 32, 64 at half load (a lane of 1 to 8 slots: phase B's lane_slots guard) through build,
lookup and the three map kernels; a FULL LANE — about 300 keys whose lane has 128 slots, found from a table read back, never
from a copy of the hash — through lookup (present rows, absent keys of the full lane and of others, with duplicates) and the
three map kernels, where the overflowed rows are reachable only by table_find's slot-by-slot walk; the same planting for
pcc_stride_map in both forms (unique_small_kernel, and first_rows_clear / insert / flag / finalize_kernel with the three scan
kernels), rows in order of first appearance and a table that indexes them.

Decided and pinned: a query of pcc_hash_lookup outside the key range is in no set (-1) — before this module lookup_kernel packed
it unchecked and answered through the aliased key.  Out-of-range ROWS handed to pcc_hash_build and out-of-range queries of
pcc_nn_search stay as they are (the coordinate-set builders report such rows; tests/test_hip_parity.py).

Kernel names launched: 18 — kernel_map27_kernel<true>, kernel_map27_kernel<false>, kernel_map_kernel, pair_count_kernel,
small_map_kernel<3>, small_map_kernel<2>, first_rows_clear_kernel, build_insert, build_count_dups, lookup_kernel,
unique_small_kernel<GenStride>, unique_small_kernel<GenChildren>, and the seven-launch builder: first_rows_insert_kernel,
first_rows_flag_kernel, scan_block_sums / scan_of_block_sums / scan_apply, first_rows_finalize_kernel.

No device case failed when this module first ran with the range test in lookup_kernel; without it the three aliasing queries
fail (item -1 masks to item 1023 and never aliased).  A find that starts its slot-by-slot walk one slot late — insert and find
no longer mirror each other — fails the full-lane tests and the small capacities and nothing else of this module: those tests
are what reaches the second loop.

Measured on an MI355X box (16 host cores): the module 1.9 s of wall time after collection (100 tests: 5 host-only, 76 map
cases — 29 k27pow2, 5 k27mod, 18 generic, 13 small3, 11 small2 —, the refusal at 257 rows, the Python route, 5 + 4 + 2 + 2
table tests, 4 range queries); the slowest case, k27pow2-same-ts1-n700-limits, 0.18 s — the first one to touch the device —,
every other one 0.01 s or less; the largest output set has 2,588 rows.
"""
import time

import numpy as np
import pytest

import _coord_cases as cc
from _coord_cases import MAP_CASES
from oracle import coords as oc

DEV = "cuda:0"
G = 64                                   # guard elements on both sides of every output
WORD_FILL, KEY_FILL, BYTE_FILL = -777777, -0x5A5A5A5A5A5A5A5B, 0xA5
KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

_FAULT = []


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_device_error():
    """a HIP error (not a mismatch) in one test of this module: the later ones do not touch the device again"""
    if _FAULT:
        pytest.fail("an earlier test of this module ended in a device error: " + _FAULT[0])
    yield


def device_call(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except AssertionError:
        raise
    except Exception as e:                # torch / PccError: the device or the library refused
        _FAULT.append(repr(e)[:300])
        raise


# ---- host: the references on hand-written examples ---------------------------------------------------------------------------
def test_references_on_hand_written_examples():
    c = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 0, -1, 1], [0, 2, 2, 2]], dtype=np.int32)
    assert oc.kernel_offsets(3)[[0, 12, 13, 14, 26]].tolist() == [[-1, -1, -1], [-1, 0, 0], [0, 0, 0], [1, 0, 0], [1, 1, 1]]
    assert oc.kernel_offsets(2)[[0, 1, 2, 4, 7]].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]]
    nbr, mask, pairs = cc.reference_map(c, c, 3, 1, 1)
    want = np.full((5, 27), -1)
    want[np.arange(5), 13] = np.arange(5)
    want[0, 14], want[1, 12] = 1, 0                                   # (0,0,0,0) <-> (0,1,0,0); (1,1,0,0) is another item's
    want[0, 13 - 3 + 9], want[3, 13 + 3 - 9] = 3, 0                   # (0,0,-1,1) = (0,0,0,0) + (0,-1,+1): offset index 13 - 3 + 9
    want[3, 2 + 6], want[1, 18] = 1, 3                                # (0,1,0,0) = (0,0,-1,1) + (+1,+1,-1): offset index 2 + 3 * 2 + 9 * 0
    assert np.array_equal(nbr, want) and pairs == 11
    assert mask.tolist() == [(1 << 13) | (1 << 14) | (1 << 19), (1 << 13) | (1 << 12) | (1 << 18), 1 << 13, (1 << 13) | (1 << 7) | (1 << 8), 1 << 13]
    # a transposed map: the child at parent + off * step finds the parent at offset off (c_in = c_out - off * step)
    parents = np.array([[0, 0, 0, 0], [0, 4, 0, 0]], dtype=np.int32)
    kids = np.array([[0, 2, 0, 0], [0, 0, -2, 2], [0, 1, 0, 0]], dtype=np.int32)
    nbr, mask, pairs = cc.reference_map(parents, kids, 3, 2, -1)
    assert nbr[0, 14] == 0 and nbr[0, 12] == 1 and nbr[1, 13 - 3 + 9] == 0 and pairs == 3 and mask[2] == 0
    nbr, mask, pairs = cc.reference_map(parents, kids, 2, 2, -1)
    assert nbr.shape == (3, 8) and nbr[0, 1] == 0 and pairs == 1      # kernel size 2: offsets 0 / +1 only
    assert cc.reference_map(parents, kids, 1, 4, 1)[0].shape == (3, 1)
    # lookup: the smallest row of a duplicate group; absent = -1
    dup = np.array([[0, 5, 5, 5], [2, 1, 1, 1], [0, 5, 5, 5], [2, 1, 1, 1], [0, -5, 5, 5]], dtype=np.int32)
    q = np.array([[2, 1, 1, 1], [0, 5, 5, 5], [0, 5, 5, -5], [0, -5, 5, 5], [1, 5, 5, 5]], dtype=np.int32)
    assert cc.first_lookup(dup, q).tolist() == [1, 0, -1, 4, -1]
    # the voxel key: item 512 sets bit 63, the fields hold the biased coordinates
    k = oc.pack(np.array([[512, 0, 0, 0], [1022, cc.COORD_LIMIT, -cc.COORD_LIMIT, 1]]))
    assert int(k[0]) == (512 << 54) | (1 << 53) | (1 << 35) | (1 << 17) and int(k[0]) >> 63 == 1
    assert int(k[1]) == (1022 << 54) | ((131072 + 130000) << 36) | ((131072 - 130000) << 18) | 131073
    assert np.array_equal(oc.unpack(k), [[512, 0, 0, 0], [1022, cc.COORD_LIMIT, -cc.COORD_LIMIT, 1]])
    assert cc.popcount(np.array([0, 1, 0x7FFFFFF, 0x80000000], dtype=np.uint32)).tolist() == [0, 1, 27, 1]
    assert [cc.capacity_for(n) for n in (0, 4, 5, 300, 512, 513)] == [8, 8, 16, 1024, 1024, 2048]
    assert [cc.table_shift(s) for s in (1, 2, 3, 6, 8, 16)] == [0, 1, 0, 0, 3, 4]


def test_order_reference_on_examples_and_against_a_plain_restatement():
    """order_key (the one copy, which tests/test_hip_parity.py imports): offset 1 is rarer than offset 0, so it is the top bit;
    descending in the permuted mask, equal keys keep their row order"""
    import test_hip_parity
    assert test_hip_parity.order_key is cc.order_key
    masks = np.array([0b01, 0b11, 0b01, 0b10, 0b00, 0b01], dtype=np.uint32)          # bit 0: four rows, bit 1: two
    # counts: 25 offsets with 0 rows take bits 26 .. 2 (lower offset first), offset 1 (2 rows) bit 1, offset 0 (4 rows) bit 0
    assert cc.order_key(masks).tolist() == [0x7FFFFFF - v for v in (1, 3, 1, 2, 0, 1)]
    order, gmask = cc.reference_order(masks)
    assert order.tolist() == [1, 3, 0, 2, 5, 4] and gmask.tolist() == [0b11]
    rng = np.random.default_rng(5)
    palette = rng.integers(0, 1 << 27, size=9, dtype=np.int64)
    m = palette[rng.integers(0, 9, size=300)]
    cnt = [int(((m >> b) & 1).sum()) for b in range(27)]
    by_rarity = sorted(range(27), key=lambda b: (cnt[b], b))                        # the rarest first = the most significant
    plain = np.array([int("".join(str((int(v) >> b) & 1) for b in by_rarity), 2) for v in m])
    order, gmask = cc.reference_order(m.astype(np.uint32))
    assert np.array_equal(order, np.argsort(-plain, kind="stable")) and gmask.shape == (10,)
    assert int(gmask[9]) == int(np.bitwise_or.reduce(m[order[288:]]))
    assert cc.reference_order(np.zeros(0, np.uint32))[0].shape == (0,)


def test_constants_are_the_librarys():
    from pcc_amd import _lib
    assert (_lib.PCC.COORD_LIMIT, _lib.PCC.BATCH_LIMIT) == (cc.COORD_LIMIT, cc.BATCH_LIMIT)
    assert cc.BATCH_EDGES[-1] == cc.BATCH_LIMIT and cc.BATCH_EDGES[1] + 1 == cc.BATCH_EDGES[2] == 512
    assert cc.COORD_LIMIT + 512 < (1 << 17) - 1                        # a probe one step past the limit stays inside its field
    assert (1 << cc.table_shift(cc.POOL_STRIDE)) == cc.POOL_STRIDE and cc.LANE_TABLE_CAP // cc.PROBE_STEP == 128
    assert cc.LANE_ROWS_MIN > 128 and 2 * cc.LANE_ROWS <= cc.LANE_TABLE_CAP and 4 * cc.STRIDE_PARENTS <= cc.LANE_TABLE_CAP


# ---- host: the tables --------------------------------------------------------------------------------------------------------
def test_tables_sit_on_both_sides_of_every_boundary():
    assert len({c.id for c in MAP_CASES}) == len(MAP_CASES)
    by = {p: [c for c in MAP_CASES if c.path == p] for p in cc.PATHS}
    assert all(by[p] for p in cc.PATHS)
    for c in MAP_CASES:
        step, sign = cc.case_step_sign(c)
        if c.path.startswith("small"):
            assert c.path == "small_map_kernel<%d>" % c.ksize and (c.kind == "same" and c.n or c.n_out) <= cc.SMALL_MAP_MAX, c.id
        else:
            assert cc.map_kernel(c.ksize, step, sign) == c.path, c.id
        assert c.n < 5000 and (c.kind != "up" or c.ts % 2 == 0)
    P27, N27, GEN, S3, S2 = (by[p] for p in cc.PATHS)
    whole = lambda cases: {(c.kind, c.ts) for c in cases if c.n_out is None and c.grid == c.ts}
    assert whole(P27) >= {(k, ts) for k in ("same", "down", "cross") for ts in (1, 2, 8)} | {("up", 2), ("up", 4), ("up", 16), ("same", 3)}
    assert {(c.grid, c.ts) for c in P27 if c.grid != c.ts} == {(8, 1), (1, 8)}
    assert whole(N27) == {("up", 6)} and all(cc.table_shift(c.ts) == 0 for c in N27)
    assert {(c.ksize, cc.case_step_sign(c)[1]) for c in GEN} == {(2, -1), (2, 1), (1, 1)}
    assert {c.ts for c in GEN if c.kind == "up"} >= {2, 8, 6}
    rows = lambda cases: {c.n_out for c in cases if c.n_out is not None}
    b = cc.MAP_BLOCK_ROWS
    edges = {0, 1, b - 1, b, b + 1, 2 * b - 1, cc.SMALL_MAP_MAX - 1, cc.SMALL_MAP_MAX, cc.SMALL_MAP_MAX + 1}
    assert rows(P27) >= edges and rows(GEN) >= edges and rows(N27) >= {1, b + 1, cc.SMALL_MAP_MAX + 1}
    for cases in (P27, GEN, N27):
        assert any(n > 4 * b and n % b for n in rows(cases))                         # several workgroups, a partial last one
    assert rows(S3) >= edges - {cc.SMALL_MAP_MAX + 1} and rows(S2) >= edges - {cc.SMALL_MAP_MAX + 1}
    for cases in (S3, S2):
        assert {cc.case_step_sign(c)[1] for c in cases} == {1, -1} and any(c.ts == 6 for c in cases)
    for cases in by.values():
        assert any(set(c.items) == set(cc.BATCH_EDGES) for c in cases) and any(c.limits for c in cases)
    assert {cc.case_step_sign(c)[0] for c in MAP_CASES if c.limits and c.ksize == 3} >= {1, 8}
    assert cc.LOOKUP_SIZES == (0, 1, 255, 256, 257) and cc.SMALL_CAPS == (8, 16, 32, 64)


def _neighbours_in_other_items(c, out, ksize, step, sign):
    """(row, offset) pairs whose xyz exists in the input set under ANOTHER item only"""
    any_item = c.copy()
    any_item[:, 0] = 0
    found = 0
    for off in oc.kernel_offsets(ksize) * step * sign:
        q = out.astype(np.int64)
        q[:, 1:] += off
        q0 = q.copy()
        q0[:, 0] = 0
        found += int(((oc.lookup(any_item, q0) >= 0) & (oc.lookup(c, q) < 0)).sum())
    return found


def test_builders_plant_what_the_cases_need():
    limit = cc.COORD_LIMIT
    for case in MAP_CASES:
        c, out, ksize, step, sign = cc.map_inputs(case)
        nbr, mask, pairs, order, gmask = cc.map_reference(case)
        K = ksize ** 3
        assert c.shape == (case.n, 4) and np.unique(oc.pack(c)).size == case.n and (c[:, 1:] % case.grid == 0).all()
        assert np.unique(oc.pack(out)).size == out.shape[0] and cc.in_range(out).all()
        assert out.shape[0] == (case.n_out if case.n_out is not None else out.shape[0]) < 5000 and nbr.shape == (out.shape[0], K)
        assert set(c[:, 0].tolist()) == set(case.items) and c[:, 1:].min() < 0 < c[:, 1:].max()
        if case.n >= 100:
            assert (np.diff(oc.pack(c).astype(np.float64)) < 0).sum() > case.n // 4                 # rows in random order
        hit = nbr >= 0
        assert (c[nbr[hit], 0] == np.repeat(out[:, 0], K).reshape(-1, K)[hit]).all()                # no hit crosses items
        if case.n_out is not None:
            continue
        # the whole derived set: everything that was planted shows in the reference
        bits = cc.popcount(mask)
        assert case.n >= cc.planted_rows(case.items, case.limits) and (out.shape[0] >= 300 or case.path.startswith("small")), case.id
        if case.grid == case.ts:
            # (the children of a kernel-2 map have one candidate parent each, their own: nothing to cross to)
            assert _neighbours_in_other_items(c, out, ksize, step, sign) >= 1 or (case.kind, ksize) == ("up", 2), case.id
            if case.kind == "same":
                assert bits.min() == 1 and bits.max() == K and len(set(bits.tolist())) >= (8 if ksize == 3 else 5), case.id
            elif case.kind == "cross":
                assert bits.min() == 0 and bits.max() == K, case.id
            elif case.kind == "up":                                                      # children on every parity class
                assert {tuple(v) for v in ((out[:, 1:] % case.ts) // step).tolist()} == {(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)}
                assert bits.min() >= 1 and bits.max() == (8 if ksize == 3 else 1), case.id
            else:
                assert bits.min() >= 1 and bits.max() >= 8, case.id
        else:                                                                            # a foreign stride: hits all the same
            assert pairs > out.shape[0] // 2 and bits.min() == 0
        if case.limits:
            top = limit // case.grid * case.grid
            for axis in (1, 2, 3):
                assert (c[:, axis] == top).any() and (c[:, axis] == -top).any(), case.id
            if case.kind in ("same", "up") and limit % step == 0:
                assert limit % case.grid == 0
                for axis in (1, 2, 3):
                    for s in (1, -1):
                        rows = np.nonzero(out[:, axis] == s * limit)[0]
                        assert rows.size and (bits[rows] >= (2 if case.kind == "same" else 1)).all(), (case.id, axis, s)
                        beyond = np.nonzero(oc.kernel_offsets(ksize)[:, axis - 1] * sign * s > 0)[0]
                        assert (nbr[np.ix_(rows, beyond)] == -1).all()
    assert {cc.case_step_sign(c)[0] for c in MAP_CASES if c.limits and c.kind in ("same", "up") and c.n_out is None} >= {1, 8}
    # the table cases
    pool = cc.pool_voxels()
    assert pool.shape == (cc.POOL_ROWS, 4) and np.unique(oc.pack(pool)).size == cc.POOL_ROWS and (pool[:, 1:] % cc.POOL_STRIDE == 0).all()
    assert pool[:, 1:].min() < 0 < pool[:, 1:].max() and set(pool[:, 0].tolist()) == {0, 1}
    dup = cc.with_duplicates(pool[:700], 90, seed=1)
    groups = np.unique(oc.pack(dup), return_counts=True)[1]
    assert dup.shape[0] == 790 and groups.size == 700 and groups.max() >= 3 and (groups == 2).sum() > 40
    src = cc.stride_sources(pool[:cc.STRIDE_PARENTS])
    assert src.shape == (2 * cc.STRIDE_PARENTS, 4) and np.unique(oc.pack(src)).size == 2 * cc.STRIDE_PARENTS
    assert np.array_equal(np.unique(oc.pack(oc.stride_map(src, 1))), np.unique(oc.pack(pool[:cc.STRIDE_PARENTS])))
    # the helpers that read a table back: a hand-made table of 16 slots
    keys = np.full(16, KEY_EMPTY, dtype=np.uint64)
    keys[[3, 11, 5]] = oc.pack(pool[:3])
    slots = cc.slots_of(keys.view(np.int64), pool[:4])
    assert slots.tolist() == [3, 11, 5, -1] and cc.fullest_lane(slots[:3], 5)[0] == 3 and cc.fullest_lane(slots[:3], 5)[1].tolist() == [0, 1]
    assert cc.lane_is_full(keys, 3) and not cc.lane_is_full(keys, 5)
    for q in cc.RANGE_QUERIES:                                                           # outside the range, aliasing under the field masks
        assert not (0 <= q[0] <= cc.BATCH_LIMIT and max(abs(v) for v in q[1:]) <= limit)
    masked = lambda r: (r[0] & 0x3FF,) + tuple((v + (1 << 17)) & 0x3FFFF for v in r[1:])
    assert [masked(q) in {masked(r) for r in cc.RANGE_TABLE} for q in cc.RANGE_QUERIES] == [True, True, True, False]


# ---- device: helpers ---------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    a = np.array(a, copy=True, order="C")                            # (the shared inputs are read-only)
    return torch.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)).to(DEV)      # (addressable when empty)


def guarded(size, dtype, fill):
    import torch
    return torch.full((G + size + G,), fill, dtype=dtype, device=DEV)


def body(buf, size, fill, name):
    h = buf.cpu().numpy()
    assert (h[:G] == fill).all() and (h[G + size:] == fill).all(), name + ": guard elements"
    return h[G:G + size]


class Table:
    """a hashed-voxel table built by pcc_hash_build between guard slots; .keys / .vals are the device views of the slots"""

    def __init__(self, pcc, coords, tensor_stride, cap=None):
        import torch
        from pcc_amd import _lib
        L = pcc.lib()
        self.n, self.ts, self.cap = coords.shape[0], tensor_stride, cap or cc.capacity_for(coords.shape[0])
        self._keys, self._vals = guarded(self.cap, torch.int64, KEY_FILL), guarded(self.cap, torch.int32, WORD_FILL)
        self.keys, self.vals = self._keys[G:], self._vals[G:]
        dup = torch.full((3,), WORD_FILL, dtype=torch.int32, device=DEV)
        self.coords = dev(coords)
        _lib.check(L.pcc_hash_build(_lib.ptr(self.coords), self.n, _lib.ptr(self.keys), _lib.ptr(self.vals), self.cap, tensor_stride,
                                    _lib.ptr(dup[1:]), _lib.stream()))
        h = dup.cpu().numpy()
        assert h[0] == h[2] == WORD_FILL
        self.dup_count = int(h[1])
        self.host_keys = body(self._keys, self.cap, KEY_FILL, "table keys").view(np.uint64)
        vals = body(self._vals, self.cap, WORD_FILL, "table values")
        used = self.host_keys != KEY_EMPTY
        assert used.sum() == self.n - self.dup_count and (vals[~used] == 0x7FFFFFFF).all()

    def lookup(self, pcc, query, tensor_stride=None):
        import torch
        from pcc_amd import _lib
        nq = query.shape[0]
        out = guarded(nq, torch.int32, WORD_FILL)
        q = dev(query)
        _lib.check(pcc.lib().pcc_hash_lookup(_lib.ptr(self.keys), _lib.ptr(self.vals), self.cap, tensor_stride or self.ts, _lib.ptr(q), nq,
                                             _lib.ptr(out[G:]), _lib.stream()))
        return body(out, nq, WORD_FILL, "lookup")


def run_kernel_map(pcc, table, out, ksize, step, sign, want):
    """pcc_kernel_map with its three output-argument variants; ``want`` = reference_map(...)"""
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    want_nbr, want_mask, want_pairs = want[:3]
    n, K = out.shape[0], ksize ** 3
    assert table.ts == (step if sign > 0 else 2 * step)               # the stride pcc_kernel_map derives for its probes
    d_out = dev(out)
    for with_mask, with_count in ((True, True), (False, True), (False, False)):
        nbr, mask = guarded(n * K, torch.int32, WORD_FILL), guarded(n, torch.int32, WORD_FILL)
        count = torch.full((3,), WORD_FILL, dtype=torch.int64, device=DEV)
        _lib.check(L.pcc_kernel_map(ptr(d_out), n, ptr(table.keys), ptr(table.vals), table.cap, ksize, step, sign, ptr(nbr[G:]),
                                    ptr(mask[G:]) if with_mask else None, ptr(count[1:]) if with_count else None, _lib.stream()))
        got = body(nbr, n * K, WORD_FILL, "nbr").reshape(n, K)
        bad = np.nonzero(got != want_nbr)
        assert bad[0].size == 0, ("nbr", with_mask, with_count, bad[0].size, bad[0][:4].tolist(), bad[1][:4].tolist(),
                                  got[bad][:4].tolist(), want_nbr[bad][:4].tolist())
        got_mask = body(mask, n, WORD_FILL, "row_mask")
        if with_mask:
            assert np.array_equal(got_mask.view(np.uint32), want_mask), "row_mask"
        else:
            assert (got_mask == WORD_FILL).all(), "row_mask written though NULL"
        assert count.cpu().numpy().tolist() == [WORD_FILL, want_pairs if with_count else WORD_FILL, WORD_FILL], (with_mask, with_count)
    return 3


def run_small_map(pcc, table, out, ksize, step, sign, want, expect_rc=0):
    """pcc_small_kernel_map: nbr, row_mask, order and group_mask32 against the references; with ``expect_rc`` < 0 the call must be
    refused with that code and write nothing"""
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    want_nbr, want_mask, _, want_order, want_gmask = want
    n, K = out.shape[0], ksize ** 3
    groups = (n + 31) // 32
    assert table.ts == (step if sign > 0 else 2 * step)
    d_out = dev(out)
    nbytes = L.pcc_order_scratch_bytes(n)
    nbr, mask, order = (guarded(size, torch.int32, WORD_FILL) for size in (n * K, n, n))
    gmask, scratch = guarded(groups, torch.int32, WORD_FILL), guarded(nbytes, torch.uint8, BYTE_FILL)
    rc = L.pcc_small_kernel_map(ptr(d_out), n, ptr(table.keys), ptr(table.vals), table.cap, ksize, step, sign, ptr(nbr[G:]), ptr(mask[G:]),
                                ptr(order[G:]), ptr(gmask[G:]), ptr(scratch[G:]), nbytes, _lib.stream())
    if expect_rc == 0:
        _lib.check(rc)
    else:
        assert rc == expect_rc, (rc, L.pcc_last_error())
    got = [body(nbr, n * K, WORD_FILL, "nbr").reshape(n, K), body(mask, n, WORD_FILL, "row_mask"), body(order, n, WORD_FILL, "order"),
           body(gmask, groups, WORD_FILL, "group_mask32")]
    body(scratch, nbytes, BYTE_FILL, "scratch")
    if expect_rc:
        assert all((g == WORD_FILL).all() for g in got), "a refused call wrote its outputs"
        return
    assert np.array_equal(got[0], want_nbr), ("nbr", int((got[0] != want_nbr).sum()))
    assert np.array_equal(got[1].view(np.uint32), want_mask), "row_mask"
    assert np.array_equal(got[2], want_order), "order"
    assert np.array_equal(got[3].view(np.uint32), want_gmask), "group_mask32"


_SLOWEST = [0.0, ""]


def _timed(name, t0):
    dt = time.perf_counter() - t0
    if dt > _SLOWEST[0]:
        _SLOWEST[:] = [dt, name]
    print(f"{name}: {dt:.3f} s (slowest so far {_SLOWEST[1]} {_SLOWEST[0]:.3f} s)")


# ---- device: kernel maps -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", MAP_CASES, ids=[c.id for c in MAP_CASES])
def test_kernel_map_equals_the_reference(pcc, case):
    t0 = time.perf_counter()
    c, out, ksize, step, sign = cc.map_inputs(case)
    want = cc.map_reference(case)
    assert out.shape[0] == (case.n_out if case.n_out is not None else out.shape[0])

    def run():
        table = Table(pcc, c, case.ts)
        assert table.dup_count == 0
        if case.path.startswith("small"):
            run_small_map(pcc, table, out, ksize, step, sign, want)
        else:
            run_kernel_map(pcc, table, out, ksize, step, sign, want)

    device_call(run)
    _timed(case.id, t0)


@pytest.mark.gpu
def test_small_map_refuses_one_row_above_its_limit(pcc):
    """257 rows: PCC_ERR_ARG before any launch, nothing written (the separate launches take such a map: the k27pow2 / generic
    cases with 257 rows)"""
    from pcc_amd import _lib
    assert pcc.lib().pcc_small_map_max() in (0, cc.SMALL_MAP_MAX)      # (0: switched off by the environment; the entry point still runs)
    for case in (c for c in MAP_CASES if c.n_out == cc.SMALL_MAP_MAX + 1 and c.ksize in (2, 3)):
        c, out, ksize, step, sign = cc.map_inputs(case)
        want = cc.map_reference(case)
        device_call(lambda: run_small_map(pcc, Table(pcc, c, case.ts), out, ksize, step, sign, want, expect_rc=_lib.PCC.ERR_ARG))
        fits = out[:cc.SMALL_MAP_MAX]
        ref = cc.reference_map(c, fits, ksize, step, sign)
        device_call(lambda: run_small_map(pcc, Table(pcc, c, case.ts), fits, ksize, step, sign, ref + cc.reference_order(ref[1])))


@pytest.mark.gpu
def test_python_reaches_the_non_power_of_two_pitch(pcc):
    """CoordMap(c, 6).up(3) and its transposed map: kernel_map27_kernel<false> (parent pitch 6) behind the Python classes, children
    built on the device (unique_small_kernel<GenChildren>)"""
    import torch
    c = cc.build_set(160, 6, seed=3, items=(0, 1, 2), limits=False)
    assert cc.map_kernel(3, 3, -1) == "kernel_map27_kernel<false>"

    def run():
        parents = pcc.CoordMap(torch.from_numpy(c).to(DEV), 6)
        kids = parents.up(3)
        nbr, row_mask, pairs = parents.kernel_map(kids, 3, True)
        return kids.coords.cpu().numpy(), nbr.cpu().numpy(), row_mask.cpu().numpy(), int(pairs.item())

    out, nbr, row_mask, pairs = device_call(run)
    assert np.array_equal(np.unique(oc.pack(out)), oc.pack(oc.children(c, 6, 3))) and out.shape[0] > 1000
    want_nbr, want_mask, want_pairs = cc.reference_map(c, out, 3, 3, -1)
    assert np.array_equal(nbr, want_nbr) and np.array_equal(row_mask.view(np.uint32), want_mask) and pairs == want_pairs


# ---- device: the table -------------------------------------------------------------------------------------------------------
def _queries(rows, absent_from, nq, seed):
    """nq queries: two thirds rows of the table (repeats included), the rest voxels that are not in it"""
    rng = np.random.default_rng([nq, seed, 17])
    present = rows[rng.integers(0, rows.shape[0], nq - nq // 3)]
    away = absent_from[rng.integers(0, absent_from.shape[0], nq // 3)]
    return cc.shuffled(np.concatenate([present, away]), seed) if nq else rows[:0]


@pytest.mark.gpu
@pytest.mark.parametrize("nq", cc.LOOKUP_SIZES)
def test_build_with_duplicates_and_lookup(pcc, nq):
    pool = cc.pool_voxels()
    rows = cc.with_duplicates(pool[:700], 90, seed=nq)
    q = _queries(rows, pool[700:], nq, seed=nq)

    def run():
        table = Table(pcc, rows, cc.POOL_STRIDE)
        return table.dup_count, table.lookup(pcc, q), table.lookup(pcc, rows)

    dups, got, got_rows = device_call(run)
    assert dups == 90
    assert np.array_equal(got, cc.first_lookup(rows, q)) and (nq < 3 or ((got >= 0).any() and (got < 0).any()))
    want_rows = cc.first_lookup(rows, rows)
    assert np.array_equal(got_rows, want_rows) and (want_rows != np.arange(rows.shape[0])).sum() == 90


@pytest.mark.gpu
@pytest.mark.parametrize("cap", cc.SMALL_CAPS)
def test_small_capacities_at_half_load(pcc, cap):
    """any power of two >= 2 n is a capacity: a lane of 1, 2, 4 and 8 slots (kernel_map27's phase B reads four slots ahead and
    must stop at the lane's end)"""
    n = cap // 2
    sets = [cc.cube_voxels(n, seed) for seed in range(8)]
    assert sum(cc.reference_map(c, c, 3, 1, 1)[2] for c in sets) > 8 * n          # neighbours beside the rows themselves
    for seed, c in enumerate(sets):
        q = cc.cube_voxels(96, 50 + seed, side=5)                       # some in the table, most not
        ref3, ref2 = cc.reference_map(c, c, 3, 1, 1), cc.reference_map(c, c, 2, 1, 1)

        def run():
            table = Table(pcc, c, 1, cap=cap)
            assert table.cap == cap == 2 * table.n and table.dup_count == 0
            assert np.array_equal(table.lookup(pcc, q), cc.first_lookup(c, q))
            run_kernel_map(pcc, table, c, 3, 1, 1, ref3)
            run_kernel_map(pcc, table, c, 2, 1, 1, ref2)
            run_small_map(pcc, table, c, 3, 1, 1, ref3 + cc.reference_order(ref3[1]))

        device_call(run)


@pytest.fixture(scope="module")
def lane_pool(pcc):
    """the pool's table at pcc_hash_capacity(4096), read back: (pool rows, the most populated lane, its row indices)"""
    pool = cc.pool_voxels()

    def run():
        cap = pcc.lib().pcc_hash_capacity(cc.POOL_ROWS)
        table = Table(pcc, pool, cc.POOL_STRIDE, cap=cap)
        assert cap == 8192 and table.dup_count == 0
        return cc.slots_of(table.host_keys, pool)

    slots = device_call(run)
    assert (slots >= 0).all()
    lane, rows = cc.fullest_lane(slots, cc.POOL_ROWS)
    assert rows.size >= cc.LANE_ROWS + 50, "the pool's fullest lane is too thin: the planting must be redone"
    others = np.nonzero((slots & (cc.PROBE_STEP - 1)) != lane)[0]
    return pool, lane, rows, others


def _full_lane_table(pcc, rows, lane, distinct):
    """a table of LANE_TABLE_CAP slots over ``rows``; the precondition: the lane's 128 slots are all taken, the other keys sit
    outside it (lanes only fill: whoever does not fit overflows slot by slot)"""
    table = Table(pcc, rows, cc.POOL_STRIDE, cap=cc.LANE_TABLE_CAP)
    slots = cc.slots_of(table.host_keys, rows)
    in_lane = (table.host_keys[lane::cc.PROBE_STEP] != KEY_EMPTY).sum()
    msg = "the planted lane is not full: the hash has changed and the planting must be redone"
    assert (slots >= 0).all() and cc.lane_is_full(table.host_keys, lane) and in_lane == cc.LANE_TABLE_CAP // cc.PROBE_STEP, msg
    overflowed = (slots & (cc.PROBE_STEP - 1)) != lane
    assert np.unique(slots[overflowed]).size == distinct - in_lane >= cc.LANE_ROWS_MIN - 128, msg
    return table, overflowed


@pytest.mark.gpu
def test_full_lane_lookup(pcc, lane_pool):
    pool, lane, lane_rows, others = lane_pool
    members = lane_rows[:cc.LANE_ROWS]
    assert members.size >= cc.LANE_ROWS_MIN
    S = pool[members]
    unused = pool[lane_rows[cc.LANE_ROWS:]]                              # same lane, not in the table: a walk through the full lane
    elsewhere = pool[others[:400]]
    q = cc.shuffled(np.concatenate([S, unused, elsewhere]), 2)
    with_dups = cc.with_duplicates(S, 60, seed=4)

    def run():
        table, overflowed = _full_lane_table(pcc, S, lane, distinct=S.shape[0])
        got = table.lookup(pcc, q)
        dup_table, _ = _full_lane_table(pcc, with_dups, lane, distinct=S.shape[0])
        return int(overflowed.sum()), got, dup_table.dup_count, dup_table.lookup(pcc, q)

    n_over, got, dups, got_dup = device_call(run)
    want = cc.first_lookup(S, q)
    assert unused.shape[0] >= 50 and (want >= 0).sum() == S.shape[0] and n_over == S.shape[0] - 128
    assert np.array_equal(got, want)
    assert dups == 60 and np.array_equal(got_dup, cc.first_lookup(with_dups, q))


@pytest.mark.gpu
def test_full_lane_kernel_maps(pcc, lane_pool):
    """out = S + (step, 0, 0): the hit at offset -x (kernel 3, sign +1, step 2) or +x (kernel 2, sign -1, step 1: c_in = c_out - off)
    is the row of S itself — for the overflowed rows, which come first, reachable only through table_find's slot-by-slot walk
    behind a full lane (kernel_map27: phase A, phase B and the lane walk all fail first)"""
    pool, lane, lane_rows, others = lane_pool
    S = pool[lane_rows[:cc.LANE_ROWS]]

    def run():
        table, overflowed = _full_lane_table(pcc, S, lane, distinct=S.shape[0])
        first = np.concatenate([np.nonzero(overflowed)[0], np.nonzero(~overflowed)[0]])
        n_over = int(overflowed.sum())
        for ksize, step, sign, col in ((3, 2, 1, 12), (2, 1, -1, 1)):
            out = S[first] + np.array([0, step, 0, 0], dtype=np.int32)
            want = cc.reference_map(S, out, ksize, step, sign)
            assert np.array_equal(want[0][:, col], first)                               # every row has the hit, the first n_over the cold one
            run_kernel_map(pcc, table, out, ksize, step, sign, want)
            small = out[:200]
            ref = cc.reference_map(S, small, ksize, step, sign)
            run_small_map(pcc, table, small, ksize, step, sign, ref + cc.reference_order(ref[1]))
        return n_over

    assert device_call(run) >= cc.LANE_ROWS_MIN - 128


@pytest.mark.gpu
@pytest.mark.parametrize("small", [True, False], ids=["unique_small_kernel", "seven_launches"])
def test_full_lane_stride_map(pcc, lane_pool, small):
    """200 parents of one lane of the stride-2 table, two source rows each: pcc_stride_map's insert walks the full lane and
    overflows; rows in order of first appearance, the returned table indexes them"""
    import torch
    from pcc_amd import _lib
    from test_first_rows_order import first_rows, stride_candidates
    pool, lane, lane_rows, others = lane_pool
    parents = pool[lane_rows[:cc.STRIDE_PARENTS]]
    src = cc.stride_sources(parents, seed=1)
    m = src.shape[0]
    cap = cc.LANE_TABLE_CAP
    want = first_rows(stride_candidates(src, 1))
    assert want.shape[0] == cc.STRIDE_PARENTS and m == 2 * cc.STRIDE_PARENTS and cap >= 2 * m
    L, ptr = pcc.lib(), _lib.ptr

    def run():
        keys, vals = guarded(cap, torch.int64, KEY_FILL), guarded(cap, torch.int32, WORD_FILL)
        ne = L.pcc_scan_scratch_elems(m)
        scratch, rows = guarded(ne, torch.int32, WORD_FILL), guarded(4 * m, torch.int32, WORD_FILL)
        count = torch.full((3,), WORD_FILL, dtype=torch.int64, device=DEV)
        d_src = dev(src)
        before = L.pcc_small_paths(-1)
        try:
            L.pcc_small_paths((before | cc.UNIQUE_SMALL_BIT) if small else (before & ~cc.UNIQUE_SMALL_BIT))
            _lib.check(L.pcc_stride_map(ptr(d_src), m, 1, ptr(keys[G:]), ptr(vals[G:]), cap, ptr(scratch[G:]), ptr(rows[G:]), ptr(count[1:]),
                                        _lib.stream()))
            torch.cuda.synchronize()
        finally:
            L.pcc_small_paths(before)
        assert count.cpu().numpy().tolist() == [WORD_FILL, want.shape[0], WORD_FILL]
        got = body(rows, 4 * m, WORD_FILL, "out_coords")
        body(scratch, ne, WORD_FILL, "scratch")
        host_keys = body(keys, cap, KEY_FILL, "table keys").view(np.uint64)
        body(vals, cap, WORD_FILL, "table values")
        n = want.shape[0]
        assert np.array_equal(got[:4 * n].reshape(n, 4), want), "rows in order of first appearance"
        assert (got[4 * n:] == WORD_FILL).all(), "rows behind the count were written"
        slots = cc.slots_of(host_keys, want)
        msg = "the planted lane is not full: the hash has changed and the planting must be redone"
        assert (slots >= 0).all() and cc.lane_is_full(host_keys, lane) and ((slots & 7) != lane).sum() == n - 128, msg
        assert (host_keys != KEY_EMPTY).sum() == n
        out = guarded(n + 100, torch.int32, WORD_FILL)
        q = dev(np.concatenate([want, pool[others[:100]]]))
        _lib.check(L.pcc_hash_lookup(ptr(keys[G:]), ptr(vals[G:]), cap, 2, ptr(q), n + 100, ptr(out[G:]), _lib.stream()))
        found = body(out, n + 100, WORD_FILL, "lookup")
        assert np.array_equal(found[:n], np.arange(n)) and (found[n:] == -1).all(), "the returned table indexes the rows"

    device_call(run)


# ---- device: a query outside the key range -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("query", cc.RANGE_QUERIES, ids=["x+2^18", "y-2^18", "item1024", "item-1"])
def test_lookup_of_a_query_outside_the_key_range_is_minus_one(pcc, query):
    """include/pcc_hip.h: nothing is answered through an aliased key.  pack_key masks every field, so (0, 5 + 2^18, 4, 5) has the key
    of (0, 5, 4, 5): lookup_kernel tests the range first"""
    rows = np.array(cc.RANGE_TABLE, dtype=np.int32)
    q = np.array([rows[0], query, rows[1], query], dtype=np.int32)

    def run():
        table = Table(pcc, rows, 1)
        return table.lookup(pcc, q)

    assert device_call(run).tolist() == [0, -1, 1, -1]

