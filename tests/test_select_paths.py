"""Top-k selection, row compaction and the small row kernels beside them, on every launch path, held to EQUALITY with numpy
references of the documented contract (tests/_select_cases.py).

pcc_topk_mask (csrc/select.hip) through the C-ABI on its five paths — one workgroup (topk_small_kernel), one large item
(topk_hist1_kernel / topk_pick1_kernel / topk_tail_kernel), the generic kernels with one item (bit 1 of pcc_small_paths off),
the LDS histogram for 2..16 items and the global-atomic histogram for 17 or more — with row counts on both sides of every
boundary of the launch code (32,768 rows; the grid-stride loop of topk_hist above 131,072; the second iteration of
topk_hist1_kernel above 1,048,576).  Logit families: normal, a third of exact ties plus +-0, all equal, two values, specials
(NaN of both signs and two payloads, +-inf, +-1e-40, +-FLT_MAX, FLT_MIN) and same_exponent (one bin in the first three radix
passes); ld = 1 (the decoder's [n, 1] logits) and wider.  Several items: interleaved rows, an empty item with k > 0, items
that resolve in pass 0 beside items resolved only by the voxel key, rows with item index -1 and nbatch.  Every case: the k
values 0, -3, 1, count // 3, count - 1, count, count + 5 and the three boundaries of every tie group; the mask between guard
bytes; a state of exactly pcc_topk_state_elems(nbatch) words in front of guard words; twice (same bytes); and on permuted
rows (the permuted mask).

pcc_compact_rows (csrc/coords.hip) at 0, 1, 1023 .. 1025, 262,144 / 262,145 (the second iteration of scan_of_block_sums) and
524,289 rows, six mask kinds, c in {0, 1, 3, 4, 6, 64}, every combination of NULL coords / feats / new_index, c = 4 on a
misaligned pointer (the scalar copy) — rows [0, m) equal boolean indexing, rows [m, n) and the guards keep their sentinel,
the device count equals m.  pcc_count_per_batch against np.bincount (64 distinct items in a wave, indices -1 and nbatch),
pcc_pair_count against a popcount sum, pcc_gather_rows / pcc_scatter_rows / pcc_scatter_add_rows up to the shape that takes
their grid-stride loop (131,073 x 128), scatter-add with up to 64 hits on one row on small integers.

The oracle (oracle/codec.py:topk_mask) orders logits with the same key as the references here (oracle.coords.float_key): NaN
above +inf, as include/pcc_hip.h documents and torch.topk does; the host tests hold the two together and against torch.topk.

Decided and pinned: with nbatch == 1 every row must belong to item 0 (include/pcc_hip.h) — the logit passes of the one-item
paths never read the coordinates; test_one_item_selection_only_sees_item_zero checks that the wrapper and
GenerativeUpBlock never pass anything else.

No device case failed when this module first ran: kernels and header agree on all five paths (NaN rows are kept first, the
tie-break holds inside the NaN, +inf and denormal groups); the side that was wrong was the oracle, which sorted NaN last.

Measured on an MI355X box (16 host cores): the module 10.4 s of wall time (160 tests: 11 host-only, 76 top-k cases of 15 to 48
launches each — the slowest, 1,048,577 rows of specials, 1.25 s, most of it the numpy reference —, 48 + 2 + 1 compaction
cases, none above 0.12 s, 21 row-kernel cases, none above 0.31 s, and the up-block test).  Kernel names launched: 19 —
topk_small_kernel, topk_init, topk_hist1_kernel, topk_pick1_kernel, topk_tail_kernel, topk_hist (LDS with ballots, LDS per
item, global atomics), topk_pick, topk_write_mask; mask_to_flags, scan_block_sums, scan_of_block_sums (one and two
iterations), scan_apply, compact_index_kernel, compact_feats_kernel (float4 and scalar); count_batch_kernel,
pair_count_kernel, gather_rows_kernel, scatter_rows_kernel, scatter_add_rows_kernel.
"""
import numpy as np
import pytest

import _select_cases as sc
from _select_cases import COMPACT_CASES, TOPK_CASES

DEV = "cuda:0"
G = 64                                   # guard elements on both sides of every output
MASK_FILL, WORD_FILL, FLOAT_FILL_BITS = 0xA5, -777777, 0xCDCDCDCD

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


# ---- host: the references ----------------------------------------------------------------------------------------------------
def _three_items(n, seed):
    c = sc.build_coords(n, 3, seed=seed)
    assert set(np.unique(c[:, 0]).tolist()) == {0, 1, 2}
    return c


def _oracle_mask(logits, coords, ks):
    import torch
    from oracle import nn as on
    from oracle.codec import topk_mask
    return topk_mask(on.SparseTensor(coords, torch.from_numpy(np.ascontiguousarray(logits[:, None])), 1), [int(k) for k in ks])


def _k_sweep(logits, coords, nbatch, family):
    vecs = sc.k_vectors(logits, coords, nbatch, None)
    per = [sc.ks_for(logits[coords[:, 0] == b], family) for b in range(nbatch)]
    for j in range(max(len(p) for p in per)):
        vecs.append(np.array([p[j % len(p)] for p in per], dtype=np.int32))
    return vecs


@pytest.mark.parametrize("family", ["normal", "ties", "all_equal", "two_values", "same_exponent", "ties+inf+denormals"])
def test_reference_equals_the_oracle_on_nan_free_logits(family):
    n = 3001
    coords = _three_items(n, 11)
    if family == "ties+inf+denormals":
        logits = sc.build_logits("ties", n, seed=1)
        rng = np.random.default_rng(8)
        for v in (np.inf, -np.inf, 1e-40, -1e-40, 1e-45):
            logits[rng.integers(0, n, 40)] = v
        base = "ties"
    else:
        logits, base = sc.build_logits(family, n, seed=1), family
    assert not np.isnan(logits).any()
    for ks in _k_sweep(logits, coords, 3, base):
        want = sc.reference_topk(logits, coords, ks, 3)
        assert np.array_equal(_oracle_mask(logits, coords, ks), want.astype(bool)), (family, ks.tolist())
        assert np.array_equal(sc.kept_per_item(want, coords, 3), np.clip(np.minimum(ks, np.bincount(coords[:, 0])), 0, None))


def test_oracle_follows_the_documented_order_on_specials():
    """NaN sorts above +inf (include/pcc_hip.h, torch.topk): the oracle and reference_topk agree on the specials family, and with
    7 NaN rows in an item and k = 5 the kept rows are NaN rows — the order the oracle had before (lexsort on -logit) kept none"""
    n = 3001
    coords = _three_items(n, 12)
    logits = sc.build_logits("specials", n, seed=2)
    assert np.isnan(logits).sum() >= 12
    for ks in _k_sweep(logits, coords, 3, "specials"):
        want = sc.reference_topk(logits, coords, ks, 3)
        assert np.array_equal(_oracle_mask(logits, coords, ks), want.astype(bool)), ks.tolist()
    logits = np.random.default_rng(3).normal(size=n).astype(np.float32)
    for b in range(3):
        logits[np.nonzero(coords[:, 0] == b)[0][:7]] = np.nan
    got = _oracle_mask(logits, coords, [5, 5, 5])
    assert got.sum() == 15 and np.isnan(logits[got]).all()
    assert np.array_equal(got, sc.reference_topk(logits, coords, [5, 5, 5], 3).astype(bool))


def test_reference_selects_what_torch_topk_selects_on_tie_free_logits():
    import torch
    assert torch.topk(torch.tensor([1.0, float("nan"), float("inf"), -1.0]), 2).indices.tolist() == [1, 2]
    n = 2000
    coords = _three_items(n, 13)
    rng = np.random.default_rng(5)
    logits = rng.permutation(np.linspace(-4, 4, n)).astype(np.float32)              # distinct
    for b in range(3):
        rows = np.nonzero(coords[:, 0] == b)[0]
        logits[rows[:3]] = (np.nan, np.inf, -np.inf)                                  # one of each per item: still no ties
    for ks in ([1, 2, 3], [50, 0, 7], [400, 10 ** 6, 5]):
        want = sc.reference_topk(logits, coords, ks, 3)
        for b in range(3):
            rows = np.nonzero(coords[:, 0] == b)[0]
            k = min(ks[b], rows.size)
            picked = rows[torch.topk(torch.from_numpy(logits[rows]), k).indices.numpy()] if k else rows[:0]
            assert set(picked.tolist()) == set(np.nonzero((want != 0) & (coords[:, 0] == b))[0].tolist()), (ks, b)


def test_float_key_is_strictly_monotone():
    f = np.float32
    tiny = np.array([1], dtype=np.uint32).view(f)[0]                                   # the smallest denormal
    fixed = [-np.inf, -np.finfo(f).max, -1.0, -np.finfo(f).tiny, -1e-40, -tiny, 0.0, tiny, 1e-40, np.finfo(f).tiny, 1.0, np.finfo(f).max, np.inf]
    rng = np.random.default_rng(0)
    sample = np.unique(np.concatenate([np.array(fixed, dtype=f), rng.normal(size=2000).astype(f),
                                       (rng.normal(size=500) * 1e-41).astype(f), (rng.normal(size=500) * 1e30).astype(f)]))
    keys = sc.float_key(sample).astype(np.int64)
    assert sample.size > 2900 and (np.diff(keys) > 0).all()
    assert sc.float_key(np.array([-0.0], dtype=f))[0] == sc.float_key(np.array([0.0], dtype=f))[0] == 0x80000000
    nans = np.array(sc.SPECIAL_BITS[:4], dtype=np.uint32).view(f)
    assert np.isnan(nans).all() and (sc.float_key(nans) == 0xFFFFFFFF).all() and keys.max() < 0xFFFFFFFF


# ---- host: the tables --------------------------------------------------------------------------------------------------------
def test_tables_sit_on_both_sides_of_every_boundary():
    """from the constants of the case module (each with the source line it mirrors): every path is reached, with row counts on
    both sides of each boundary of the launch code"""
    assert len({c.id for c in TOPK_CASES}) == len(TOPK_CASES) and len({c.id for c in COMPACT_CASES}) == len(COMPACT_CASES)
    for c in TOPK_CASES:                      # the path each row names is the dispatcher's choice
        assert sc.topk_path(c.nbatch, c.n, 7 if c.small else 7 & ~sc.TOPK_SMALL_BIT) == c.path, c.id
        assert 1 <= c.nbatch <= sc.BATCH_MAX
    by = {p: [c for c in TOPK_CASES if c.path == p] for p in sc.PATHS}
    rows = {p: {c.n for c in by[p]} for p in sc.PATHS}
    assert all(by[p] for p in sc.PATHS)
    # one workgroup: up to TK_SMALL_N inclusive, one more row leaves it; around a wave and the 1024 threads of the group
    assert rows["small"] == {1, 63, 64, 65, 1023, 1025, sc.TK_SMALL_N} and sc.TK_SMALL_N + 1 in rows["large1"]
    assert {c.family for c in by["small"]} == set(sc.FAMILIES)
    for family in sc.FAMILIES:
        assert {c.ld for c in by["small"] if c.family == family} == {1, 5}
    # one large item: the second iteration of topk_hist1_kernel starts at TK1_ROWS_PER_ITER + 1 rows
    assert rows["large1"] == {32769, 150001, sc.TK1_ROWS_PER_ITER + 1, 1100003} and min(rows["large1"]) <= sc.TK1_ROWS_PER_ITER
    for n in rows["large1"]:
        assert {c.family for c in by["large1"] if c.n == n} >= {"ties", "specials", "same_exponent"}
    assert {c.n for c in by["large1"] if c.family == "all_equal"} == {32769} and {c.ld for c in by["large1"]} == {1, 2}
    # generic kernels with one item: below and at the one-workgroup size, and past the 512 x 256 rows of one grid sweep
    assert rows["generic1"] == {65, sc.TK_SMALL_N, sc.TK_GRID_ROWS + 1}
    assert all({c.family for c in by["generic1"] if c.n == n} == {"ties", "specials"} for n in rows["generic1"])
    # several items: both histogram forms on both sides of TK_LDS_BATCHES, both with the grid-stride loop
    assert {c.nbatch for c in by["lds"]} == {2, 3, sc.TK_LDS_BATCHES} and {c.nbatch for c in by["global"]} == {sc.TK_LDS_BATCHES + 1, 64, sc.BATCH_MAX}
    assert rows["lds"] == {300, 40000, sc.TK_GRID_ROWS + 8} and rows["global"] == {5000, 140001}
    assert min(rows["lds"] | rows["global"]) <= sc.TK_GRID_ROWS < max(rows["lds"]) and max(rows["global"]) > sc.TK_GRID_ROWS
    assert {(c.nbatch, c.n) for c in by["lds"]} == {(b, n) for b in sc.LDS_ITEMS for n in sc.LDS_ROWS}
    assert {(c.nbatch, c.n) for c in by["global"]} == {(b, n) for b in sc.GLOBAL_ITEMS for n in sc.GLOBAL_ROWS}
    assert all(c.empty is not None for c in by["lds"] + by["global"] if c.nbatch > 2) and any(c.empty is not None for c in by["lds"] if c.nbatch == 2)
    # compaction: the scan's tile and the second iteration of scan_of_block_sums; every mask kind at every row count
    crow = {c.n for c in COMPACT_CASES}
    assert crow == {0, 1, sc.SCAN_TILE - 1, sc.SCAN_TILE, sc.SCAN_TILE + 1, sc.SCAN_SECOND_ROWS, sc.SCAN_SECOND_ROWS + 1, 524289}
    assert {(c.n, c.mask) for c in COMPACT_CASES} == {(n, k) for n in sc.COMPACT_ROWS for k in sc.MASK_KINDS}
    assert {c.c for c in COMPACT_CASES} == set(sc.COMPACT_C)
    assert {(c.coords, c.feats, c.index) for c in COMPACT_CASES if c.c > 0} == set(sc.NULL_COMBOS)
    for side in (lambda n: 0 < n <= sc.SCAN_SECOND_ROWS, lambda n: n > sc.SCAN_SECOND_ROWS):        # both scan loop counts ...
        assert any(c.feats and c.c % 4 == 0 and side(c.n) for c in COMPACT_CASES)                   # ... with the float4 copy
        assert any(c.feats and c.c % 4 != 0 and side(c.n) for c in COMPACT_CASES)                   # ... and the scalar copy
        assert any(side(n) for n in sc.MISALIGNED_ROWS)                                             # ... and c = 4 misaligned
    # the row kernels
    assert min(sc.COUNT_ITEMS) == 1 and {sc.COUNT_WAVE, sc.COUNT_WAVE + 1} <= set(sc.COUNT_ITEMS) and max(sc.COUNT_ITEMS) == sc.BATCH_MAX
    assert {sc.COUNT_WAVE - 1, sc.COUNT_WAVE + 1, 257} <= set(sc.COUNT_ROWS)
    assert min(sc.PAIR_ROWS) == 1 and {4095, 4097} <= set(sc.PAIR_ROWS) and max(sc.PAIR_ROWS) > sc.PAIR_GRID_ROWS
    elems = sorted(n * c for n, c in sc.MOVER_SHAPES)
    assert elems[-2] <= sc.ROW_GRID_ELEMS < elems[-1] and sc.MOVER_SHAPES[0] == (1, 1)


def test_builders_plant_what_the_cases_need():
    for n in (63, 1025, 32769):
        logits = sc.build_logits("specials", n, seed=5)
        ks = sc.ks_for(logits, "specials")
        for value in sc.tie_values("specials"):                   # a boundary strictly inside the NaN, +inf and denormal groups
            above, tie = sc.tie_group(logits, value)
            assert tie >= 3 and any(above < k < above + tie for k in ks), (n, value, above, tie)
        bits = set(logits.view(np.uint32).tolist())
        assert bits >= set(sc.SPECIAL_BITS)
        assert {0, -3, 1, n // 3, n - 1, n, n + 5} <= set(ks)
    logits = sc.build_logits("same_exponent", 5000, seed=5)
    assert (sc.float_key(logits) >> 8 == sc.float_key(logits)[0] >> 8).all() and np.unique(logits).size == 256
    logits = sc.build_logits("ties", 5000, seed=5)
    assert 0.2 < (logits == 0.25).mean() < 0.34 and np.signbit(logits[logits == 0]).any() and not np.signbit(logits[logits == 0]).all()
    for case in (c for c in TOPK_CASES if c.nbatch > 1 and c.n <= 40000):
        logits, coords, ks = sc.topk_inputs(case)
        assert np.unique(coords, axis=0).shape[0] == case.n and coords[:, 1:].min() < 0
        b = coords[:, 0]
        assert (b == -1).any() and (b == case.nbatch).any()
        if case.empty is not None:
            assert not (b == case.empty).any() and all(k[case.empty] > 0 for k in ks)
        counts = np.bincount(b[(b >= 0) & (b < case.nbatch)], minlength=case.nbatch)
        mixed = ks[3]
        live = np.nonzero(counts > 0)[0]
        if live.size < 2:                                                            # (two items, one of them empty)
            continue
        assert (np.diff(b[:64]) != 0).sum() > 8                                      # interleaved, not contiguous
        assert any(mixed[i] >= counts[i] for i in live)                              # resolves in pass 0
        tied = [i for i in live if sc.tie_group(logits[b == i], 0.25)[1] >= 2 and
                sc.tie_group(logits[b == i], 0.25)[0] < mixed[i] < sum(sc.tie_group(logits[b == i], 0.25))]
        assert tied or case.n / case.nbatch < 10, case.id                            # the boundary inside the 0.25 ties of an item
    c1 = sc.build_coords(1100003, 1, seed=3)
    assert np.unique(sc.oc.pack(c1)).size == 1100003 and c1[:, 1:].min() < 0 and (c1[:, 0] == 0).all()


# ---- device: top-k -----------------------------------------------------------------------------------------------------------
def run_topk(pcc, case):
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    logits, coords, ks = sc.topk_inputs(case)
    n, nb, ld = case.n, case.nbatch, case.ld
    order = sc.topk_order(logits, coords, nb)
    counts = order[3]
    wants = [sc.reference_topk(logits, coords, k, nb, order) for k in ks]
    rng = np.random.default_rng([n, nb, 17])
    perm = rng.permutation(n)
    full = np.full((n, ld), np.nan, dtype=np.float32)                 # the other columns: NaN and large values, never read
    full[:, 1::2] = 1e30
    full[:, 0] = logits
    rows = (np.arange(n), perm)
    d_log = [torch.from_numpy(np.ascontiguousarray(full[r])).to(DEV) for r in rows]
    d_co = [torch.from_numpy(np.ascontiguousarray(coords[r])).to(DEV) for r in rows]
    d_ks = torch.from_numpy(np.stack(ks)).to(DEV)
    elems = L.pcc_topk_state_elems(nb)
    runs = [(ki, which) for ki in range(len(ks)) for which in (0, 0, 1)]          # twice as given, once permuted
    masks = torch.full((len(runs), G + n + G), MASK_FILL, dtype=torch.uint8, device=DEV)
    states = torch.full((len(runs), elems + G), WORD_FILL, dtype=torch.int32, device=DEV)
    before = L.pcc_small_paths(-1)
    try:
        L.pcc_small_paths((before | sc.TOPK_SMALL_BIT) if case.small else (before & ~sc.TOPK_SMALL_BIT))
        assert sc.topk_path(nb, n, L.pcc_small_paths(-1)) == case.path
        for r, (ki, which) in enumerate(runs):
            rc = L.pcc_topk_mask(ptr(d_log[which]), ld, ptr(d_co[which]), n, nb, ptr(d_ks[ki]), ptr(masks[r, G:]), ptr(states[r]),
                                 _lib.stream())
            assert rc == 0, (rc, L.pcc_last_error())
        torch.cuda.synchronize()
    finally:
        L.pcc_small_paths(before)
    mh, sh = masks.cpu().numpy(), states.cpu().numpy()
    assert (sh[:, elems:] == WORD_FILL).all(), "state guard words"
    assert (mh[:, :G] == MASK_FILL).all() and (mh[:, G + n:] == MASK_FILL).all(), "mask guard bytes"
    bad, first = [], {}
    for r, (ki, which) in enumerate(runs):
        got = mh[r, G:G + n]
        want = wants[ki][rows[which]]
        expect = np.clip(np.minimum(ks[ki].astype(np.int64), counts), 0, None)
        kept = sc.kept_per_item((got == 1), coords[rows[which]], nb)
        ok = np.array_equal(got, want) and np.array_equal(kept, expect)
        if which == 0 and ki in first:
            ok = ok and np.array_equal(got, first[ki])                                 # the second run: the same bytes
        first.setdefault(ki, got)
        if not ok:
            diff = np.nonzero(got != want)[0]
            bad.append((ks[ki][:4].tolist(), "permuted" if which else "as given", int(diff.size), diff[:4].tolist(),
                        int((got == 1).sum()), int(want.sum()), sorted(set(got.tolist()) - {0, 1})))
    assert not bad, (case.id, len(bad), bad[:6])
    return len(runs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TOPK_CASES, ids=[c.id for c in TOPK_CASES])
def test_topk_mask_equals_the_documented_selection(pcc, case):
    launches = device_call(run_topk, pcc, case)
    print(case.id, case.path, launches)


@pytest.mark.gpu
def test_one_item_selection_only_sees_item_zero(pcc, monkeypatch):
    """the precondition of the one-item case (include/pcc_hip.h: every row belongs to item 0), checked where the selection is
    called: whatever sparse.topk_mask receives from GenerativeUpBlock has all item indices inside [0, nbatch) — a CoordMap
    derives nbatch from its rows when the caller declared none (CoordMap.nbatch) — and each item keeps min(k, candidates)"""
    import torch
    from pcc_amd import sparse as sp
    seen = []
    real = sp.topk_mask

    def checked(logits, coords, k_per_batch, nbatch):
        b = coords[:, 0].cpu().numpy()
        assert b.min() >= 0 and b.max() < nbatch, (int(b.min()), int(b.max()), nbatch)
        mask = real(logits, coords, k_per_batch, nbatch)
        seen.append((nbatch, b, [int(v) for v in k_per_batch], mask.cpu().numpy()))
        return mask

    monkeypatch.setattr(sp, "topk_mask", checked)
    torch.manual_seed(0)
    block = pcc.GenerativeUpBlock(64, 64, predict=True).to(DEV)
    for items in (1, 2):
        c = sc.build_coords(400, max(items, 1), seed=21)
        c[:, 1:] = (c[:, 1:] // 3 % 24) * 2                                # a few hundred voxels of a stride-2 grid
        c = np.unique(c, axis=0).astype(np.int32)
        m = pcc.CoordMap(torch.from_numpy(c).to(DEV), 2)                   # no nbatch declared
        assert m.nbatch == items
        x = pcc.SparseTensor(torch.randn(c.shape[0], 64, device=DEV), coordinate_map=m)
        ks = [150, 10 ** 6][:items]
        with torch.no_grad():
            out, pred, up_map = device_call(block, x, k=ks)
        nbatch, b, k_seen, mask = seen[-1]
        assert nbatch == items and k_seen == ks
        want = np.minimum(np.array(ks), np.bincount(b, minlength=items))
        assert np.array_equal(sc.kept_per_item(mask, np.stack([b] * 4, axis=1), items), want)
        assert up_map.n == int(want.sum()) == out.F.shape[0]
    assert [s[0] for s in seen] == [1, 2]


# ---- device: compaction ------------------------------------------------------------------------------------------------------
def run_compact(pcc, n, mask, c, has_coords, has_feats, has_index, offset=0):
    """-> (kept feature rows as uint32 bits or None); asserts everything else"""
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    rng = np.random.default_rng([n, c, 31])
    coords = rng.integers(-100000, 100000, size=(n, 4)).astype(np.int32)
    feats = rng.integers(0, 1 << 32, size=(n, max(c, 1)), dtype=np.uint32)[:, :c]           # any bits: the rows are only moved
    want_c, want_f, want_x, m = sc.reference_compact(mask, coords, feats)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    d_mask = t(np.concatenate([mask, np.zeros(1, np.uint8)]))                             # (addressable when n == 0)
    d_coords = t(np.concatenate([coords.reshape(-1), np.zeros(4, np.int32)]))
    d_feats = t(np.concatenate([np.zeros(offset, np.int32), feats.reshape(-1).view(np.int32), np.zeros(8, np.int32)]))[offset:]
    out_c = torch.full((G + 4 * n + G,), WORD_FILL, dtype=torch.int32, device=DEV)
    out_f = torch.full((G + n * c + G,), WORD_FILL, dtype=torch.int32, device=DEV)
    out_x = torch.full((G + n + G,), WORD_FILL, dtype=torch.int32, device=DEV)
    ne = L.pcc_scan_scratch_elems(n)
    scratch = torch.full((ne + G,), WORD_FILL, dtype=torch.int32, device=DEV)
    count = torch.full((3,), WORD_FILL, dtype=torch.int64, device=DEV)
    assert d_feats.data_ptr() % 16 == 4 * offset and out_f[G:].data_ptr() % 16 == 0
    rc = L.pcc_compact_rows(ptr(d_mask), n, ptr(d_coords) if has_coords else None, ptr(out_c[G:]) if has_coords else None,
                            ptr(d_feats) if has_feats else None, c, ptr(out_f[G:]) if has_feats else None,
                            ptr(out_x[G:]) if has_index else None, ptr(scratch), ptr(count[1:]), _lib.stream())
    assert rc == 0, (rc, L.pcc_last_error())
    torch.cuda.synchronize()
    hc, hf, hx, hs, hn = out_c.cpu().numpy(), out_f.cpu().numpy(), out_x.cpu().numpy(), scratch.cpu().numpy(), count.cpu().numpy()
    assert hn.tolist() == [WORD_FILL, m, WORD_FILL], (hn.tolist(), m)
    assert (hs[ne:] == WORD_FILL).all(), "scratch guard"
    for name, h, width, used in (("coords", hc, 4, has_coords), ("feats", hf, c, has_feats), ("new_index", hx, 1, has_index)):
        assert (h[:G] == WORD_FILL).all() and (h[G + n * width:] == WORD_FILL).all(), name + " guards"
        body = h[G:G + n * width]
        if not used:
            assert (body == WORD_FILL).all(), name + " written though NULL"
    if has_coords:
        assert np.array_equal(hc[G:G + 4 * m].reshape(m, 4), want_c) and (hc[G + 4 * m:G + 4 * n] == WORD_FILL).all()
    if has_index:
        assert np.array_equal(hx[G:G + n], want_x)
    if has_feats:
        got = hf[G:G + m * c].view(np.uint32).reshape(m, c)
        assert np.array_equal(got, want_f) and (hf[G + m * c:G + n * c] == WORD_FILL).all()
        return got
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("case", COMPACT_CASES, ids=[c.id for c in COMPACT_CASES])
def test_compact_rows_equals_boolean_indexing(pcc, case):
    mask = sc.build_mask(case.mask, case.n)
    if case.mask == "bytes" and case.n > 100:
        assert {0, 1, 2, 255} == set(np.unique(mask).tolist())
    device_call(run_compact, pcc, case.n, mask, case.c, case.coords, case.feats, case.index)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sc.MISALIGNED_ROWS)
def test_compact_rows_scalar_copy_on_a_misaligned_pointer(pcc, n):
    """c = 4, the features one float off a 16-byte boundary: the scalar copy; the same bits as the float4 copy"""
    mask = sc.build_mask("random", n, seed=1)
    aligned = device_call(run_compact, pcc, n, mask, 4, True, True, True, offset=0)
    shifted = device_call(run_compact, pcc, n, mask, 4, True, True, True, offset=1)
    assert aligned.shape[0] > n // 5 and np.array_equal(aligned, shifted)


@pytest.mark.gpu
def test_compact_rows_wrapper_and_its_expected_count(pcc, monkeypatch):
    import torch
    from pcc_amd import sparse as sp
    n, c = 5003, 6
    rng = np.random.default_rng(41)
    mask = sc.build_mask("random", n, seed=2)
    coords = rng.integers(-1000, 1000, size=(n, 4)).astype(np.int32)
    feats = rng.normal(size=(n, c)).astype(np.float32)
    want_c, want_f, want_x, m = sc.reference_compact(mask, coords, feats)
    d = lambda a: torch.from_numpy(a).to(DEV)

    def same(res):
        rc, rf, rx, rm = res
        return rm == m and np.array_equal(rc.cpu().numpy(), want_c) and np.array_equal(rf.cpu().numpy(), want_f) and \
            np.array_equal(rx.cpu().numpy(), want_x)

    assert same(device_call(sp.compact_rows, d(mask), d(coords), d(feats), want_index=True))
    assert same(device_call(sp.compact_rows, d(mask), d(coords), d(feats), want_index=True, expected=m))     # the count is not read
    monkeypatch.setattr(sp, "CHECK_EXPECTED_COUNTS", True)
    assert same(device_call(sp.compact_rows, d(mask), d(coords), d(feats), want_index=True, expected=m))     # read and compared
    with pytest.raises(RuntimeError, match="expected"):
        sp.compact_rows(d(mask), d(coords), d(feats), expected=m + 1)


# ---- device: the row kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nbatch", sc.COUNT_ITEMS)
def test_count_per_batch_equals_bincount(pcc, nbatch):
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr

    def run():
        for n in sc.COUNT_ROWS:
            rng = np.random.default_rng([nbatch, n])
            coords = rng.integers(-50, 50, size=(n, 4)).astype(np.int32)
            b = rng.permutation(nbatch)[np.arange(n) % nbatch]             # interleaved: 64 distinct items in a wave from 64 items on
            if n >= 63:
                b[rng.integers(0, n, n // 20)] = -1
                b[rng.integers(0, n, n // 20)] = nbatch
                assert nbatch < sc.COUNT_WAVE or len(set(b[:64].tolist()) - {-1, nbatch}) > 50
            coords[:, 0] = b
            out = torch.full((G + nbatch + G,), WORD_FILL, dtype=torch.int32, device=DEV)
            d_coords = torch.from_numpy(coords).to(DEV)
            assert L.pcc_count_per_batch(ptr(d_coords), n, nbatch, ptr(out[G:]), _lib.stream()) == 0
            h = out.cpu().numpy()
            assert np.array_equal(h[G:G + nbatch], np.bincount(b[(b >= 0) & (b < nbatch)], minlength=nbatch)), (nbatch, n)
            assert (h[:G] == WORD_FILL).all() and (h[G + nbatch:] == WORD_FILL).all()

    device_call(run)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sc.PAIR_ROWS)
def test_pair_count_equals_the_popcount_sum(pcc, n):
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    words = np.random.default_rng(n).integers(0, 1 << 32, size=n, dtype=np.uint32)
    words[-1] = 0xFFFFFFFF

    def run():
        out = torch.full((3,), WORD_FILL, dtype=torch.int64, device=DEV)
        d_words = torch.from_numpy(words.view(np.int32)).to(DEV)
        assert L.pcc_pair_count(ptr(d_words), n, ptr(out[1:]), _lib.stream()) == 0
        return out.cpu().numpy()

    got = device_call(run)
    assert got.dtype == np.int64 and got.tolist() == [WORD_FILL, sc.popcount_sum(words), WORD_FILL]


def _guarded(values, fill_rows=None):
    """device float32 buffer [G + size + G]; the body holds ``values`` (or the sentinel bits)"""
    import torch
    buf = np.full(G + values.size + G, FLOAT_FILL_BITS, dtype=np.uint32)
    if fill_rows is None:
        buf[G:G + values.size] = values.reshape(-1).view(np.uint32)
    return torch.from_numpy(buf.view(np.float32)).to(DEV)


def _body(buf, shape):
    h = buf.cpu().numpy().view(np.uint32)
    size = int(np.prod(shape))
    assert (h[:G] == FLOAT_FILL_BITS).all() and (h[G + size:] == FLOAT_FILL_BITS).all(), "guards"
    return h[G:G + size].reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("n,c", sc.MOVER_SHAPES)
def test_gather_rows_plain_and_accumulate(pcc, n, c):
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    rng = np.random.default_rng([n, c, 51])
    n_src = n // 2 + 1
    src = rng.normal(size=(n_src, c)).astype(np.float32)
    idx = rng.integers(0, n_src, size=n).astype(np.int32)
    idx[rng.integers(0, n, n // 7)] = -1
    base = rng.normal(size=(n, c)).astype(np.float32)
    picked = np.where(idx[:, None] >= 0, src[np.maximum(idx, 0)], np.float32(0))

    def run():
        d_src, d_idx = torch.from_numpy(src).to(DEV), torch.from_numpy(idx).to(DEV)
        plain, acc = _guarded(np.empty((n, c), np.float32), fill_rows=True), _guarded(base)
        assert L.pcc_gather_rows(ptr(d_src), c, ptr(d_idx), n, ptr(plain[G:]), 0, _lib.stream()) == 0
        assert L.pcc_gather_rows(ptr(d_src), c, ptr(d_idx), n, ptr(acc[G:]), 1, _lib.stream()) == 0
        return _body(plain, (n, c)), _body(acc, (n, c))

    plain, acc = device_call(run)
    assert np.array_equal(plain, picked.view(np.uint32)) and (plain[idx < 0] == 0).all()             # idx = -1: a zero row
    assert np.array_equal(acc.view(np.float32), base + picked)                                       # one IEEE add per element
    assert np.array_equal(acc[idx < 0], base.view(np.uint32)[idx < 0])                               # idx = -1: unchanged


@pytest.mark.gpu
@pytest.mark.parametrize("n,c", sc.MOVER_SHAPES)
def test_scatter_rows_to_unique_targets(pcc, n, c):
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    rng = np.random.default_rng([n, c, 52])
    n_out = n + n // 3 + 1
    src = rng.normal(size=(n, c)).astype(np.float32)
    idx = rng.permutation(n_out)[:n].astype(np.int32)
    idx[rng.integers(0, n, n // 7)] = -1
    want = np.full((n_out, c), FLOAT_FILL_BITS, dtype=np.uint32)
    want[idx[idx >= 0]] = src.view(np.uint32)[idx >= 0]

    def run():
        out = _guarded(np.empty((n_out, c), np.float32), fill_rows=True)
        d_src, d_idx = torch.from_numpy(src).to(DEV), torch.from_numpy(idx).to(DEV)
        assert L.pcc_scatter_rows(ptr(d_src), c, ptr(d_idx), n, ptr(out[G:]), _lib.stream()) == 0
        return _body(out, (n_out, c))

    assert np.array_equal(device_call(run), want)                                  # rows nobody targets keep the sentinel


@pytest.mark.gpu
@pytest.mark.parametrize("n,c", sc.MOVER_SHAPES)
def test_scatter_add_rows_with_repeated_targets(pcc, n, c):
    """small integers: the sum is exact in any order; the reference is a per-column np.bincount with weights"""
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    rng = np.random.default_rng([n, c, 53])
    n_out = max(1, n // 8)
    src = rng.integers(-3, 4, size=(n, c)).astype(np.float32)
    idx = rng.integers(0, n_out, size=n).astype(np.int32)
    idx[rng.integers(0, n, n // 7)] = -1
    idx[rng.permutation(n)[:64]] = n_out - 1                                        # up to 64 hits (and more) on one row
    base = rng.integers(-3, 4, size=(n_out, c)).astype(np.float32)
    live = idx >= 0
    hits = np.bincount(idx[live], minlength=n_out)
    assert hits.max() * 3 + 3 < 2 ** 24 and (n < 64 or hits[n_out - 1] >= 64)
    want = base.astype(np.float64)
    for col in range(c):
        want[:, col] += np.bincount(idx[live], weights=src[live, col], minlength=n_out)

    def run():
        out = _guarded(base)
        d_src, d_idx = torch.from_numpy(src).to(DEV), torch.from_numpy(idx).to(DEV)
        assert L.pcc_scatter_add_rows(ptr(d_src), c, ptr(d_idx), n, ptr(out[G:]), _lib.stream()) == 0
        return _body(out, (n_out, c)).view(np.float32)

    got = device_call(run)
    assert np.array_equal(got.astype(np.float64), want)
