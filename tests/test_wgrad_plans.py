"""Every weight-gradient kernel `plan_wgrad` (csrc/conv_bwd.hip) can pick, per launch, held to EQUALITY with a float64
reference: the thin kernel, the one-offset kernel (one and two row groups per iteration), the slice kernel at every (O, AHEAD),
the bf16 one-offset kernel (one and two groups) and the bf16 slice kernel at every O; and the two map helpers of the
backward-data path (pcc_kernel_map_transpose, pcc_permute_map_rows).

The case table (tests/_wgrad_plan_cases.py) names the kernel, the split count and the number of partial images each row
expects; every GPU case first asserts that `pcc_conv_wgrad_kernel_name` returns them, and a host test sweeps that query over a
grid of shapes and fails when the plan can emit a launch no row reaches.  Row counts sit on both sides of every boundary of the
plan: the first split above the minimum, the cap, and the first row at which a workgroup loads group masks a second time.
Inputs are synthetic (seeded numpy) with planted corners, from the two operand families whose sums are exact in any order
(small integers; wide mantissas times +-1, +-2 — the case builder asserts the condition), so the comparison is
np.array_equal.  Every case also runs twice (same bits), with gmask == NULL and with all-ones masks (same bits), into a dw
and a scratch with guard bands (nothing outside dw; nothing outside the plan's partial images).

The kernels behind the once-per-process switches run in child processes, one per (PCC_WGRAD_SLICE_O, PCC_WGRAD_AHEAD) pair
and one for PCC_WGRAD_SLICE=0, PCC_WGRAD_BF16_SLICE_O riding along.

Measured on an MI355X box (16 host cores): the module 62.9 s of wall time (444 tests: 21 host-only, 368 table cases — none above
0.7 s —, 11 child processes, four shells, 36 + 3 map-helper cases, the refusals), of which the children 3.8 - 5.2 s each (34 cases
per child).  Kernel names launched: 16 — conv_wgrad_thin_kernel, conv_wgrad_kernel (one group and two groups per iteration),
conv_wgrad_slice_kernel<3 | 4 | 5 | 6 | 9, 1 | 2>, conv_wgrad_bf16_kernel (one group and two), conv_wgrad_bf16_slice_kernel<3 | 5 | 9>
— and both second-stage reductions.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _wgrad_plan_cases as wc
from _wgrad_plan_cases import CASES, CHILD_ENVS, DEFAULT_ENV

DEV = "cuda:0"

# Measured wall time of the slowest child process of test_switched_kernels_in_a_child (five runs: 3.8 .. 5.2 s per child, 6.4 s once); the
# timeout is three times that, because load on a shared box varies.
CHILD_WALL_S = 6.4
CHILD_TIMEOUT_S = math.ceil(3 * CHILD_WALL_S)


def launch_key(name, split, partials, cin, cout):
    """what tells two launches apart: the kernel and whether it takes two row groups per iteration — the fp32 one-offset
    kernel then writes 4 partials per split (one per wave); the bf16 one does so on 64 x 64 blocks"""
    two = partials // split == 4 or (name == "conv_wgrad_bf16_kernel" and cin <= 64 and cout <= 64)
    return name, 2 if two else 1


# ---- the table itself (host only) ------------------------------------------------------------------------------------
def test_row_counts_sit_on_the_plan_boundaries(pcc):
    """the boundaries are computed from the plan (the query), not copied: the last row count of split 8 and of the split
    below the cap, and the last row count without a second mask load — and the table has both sides of each"""
    L = pcc.lib()

    def last_with_split(bf16, cin, cout, s):               # bisect the query for the largest n_out whose split is still s
        lo, hi = 1, 1 << 22
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if wc.planned(L, bf16, 27, cin, cout, mid)[1] <= s else (lo, mid - 1)
        return lo

    for bf16, one, slc in ((False, (128, 128), (64, 64)), (True, (128, 128), (64, 64))):
        assert (last_with_split(bf16, *one, 8), last_with_split(bf16, *one, 127)) == (13792, 196576) == (wc.ONE_STEP[0], wc.ONE_CAPPED[0])
        assert (last_with_split(bf16, *slc, 8), last_with_split(bf16, *slc, 255)) == (6880, 196576) == (wc.SLICE_STEP[0], wc.SLICE_CAPPED[0])
        cap_one, cap_slice = wc.planned(L, bf16, 27, *one, 1 << 22)[1], wc.planned(L, bf16, 27, *slc, 1 << 22)[1]
        assert (cap_one, cap_slice) == (128, 256)
        assert (32 * wc.MASKS_PER_LOAD * cap_one, 32 * wc.MASKS_PER_LOAD * cap_slice) == (262144, 524288) == (wc.ONE_SECOND[0], wc.SLICE_SECOND[0])
    rows = {}
    for c in CASES:
        rows.setdefault(c.kernel, set()).add(c.n_out)
    one_rows = {1, 31, 32, 33, 256, 257, 13792, 13793, 196576, 196577, 200003, 262144, 262145, 270001}
    slice_rows = {1, 31, 32, 33, 256, 257, 512, 6880, 6881, 196576, 196577, 524288, 524289, 530003}
    assert rows["conv_wgrad_kernel"] >= one_rows and rows["conv_wgrad_bf16_kernel"] >= one_rows
    assert rows["conv_wgrad_slice_kernel<5, 2>"] >= slice_rows and rows["conv_wgrad_bf16_slice_kernel<3>"] >= slice_rows
    assert rows["conv_wgrad_thin_kernel"] == {1, 255, 256, 257, 5000}
    # the split counts on both sides of the steps, as numbers
    by = {(c.kernel, c.n_out): c.split for c in CASES if c.K == 27}
    assert [by["conv_wgrad_kernel", n] for n in (13792, 13793, 196576, 196577, 200003, 270001)] == [8, 9, 127, 128, 128, 128]
    assert [by["conv_wgrad_slice_kernel<5, 2>", n] for n in (6880, 6881, 196576, 196577, 530003)] == [8, 9, 255, 256, 256]


def test_case_table_names_what_the_plan_picks(pcc):
    """every row's kernel, split and partial count are the plan's answer for that row (a wrong table fails here, without a
    GPU); ids are unique; the table holds the shapes and forms it claims"""
    L = pcc.lib()
    assert len({c.id for c in CASES}) == len(CASES)
    for c in CASES:
        assert wc.planned(L, c.bf16, c.K, c.cin, c.cout, c.n_out) == (c.kernel, c.split, c.partials), c.id
    f32_one = [c for c in CASES if c.kernel == "conv_wgrad_kernel" and c.partials == c.split]
    assert {(c.cin, c.cout) for c in f32_one} == set(wc.ONE_SHAPES) and {c.K for c in f32_one} == {27, 8, 1}
    chunks = lambda ch: {min(4, (ch - b) // 32) for b in range(0, ch, 128)}                 # live chunks of each 128-wide block
    assert set().union(*(chunks(c.cin) for c in f32_one)) == {1, 2, 3, 4} == set().union(*(chunks(c.cout) for c in f32_one))
    assert any(c.cin > 128 for c in f32_one) and any(c.cout > 128 for c in f32_one)
    two = [c for c in CASES if c.kernel == "conv_wgrad_kernel" and c.partials == 4 * c.split]
    assert {c.K for c in two} == {8, 1} and max(c.n_out for c in two) > wc.ONE_SECOND[0]
    assert {(c.cin, c.cout) for c in CASES if c.kernel == "conv_wgrad_slice_kernel<5, 2>"} == set(wc.SLICE_SHAPES)
    bf = [c for c in CASES if c.kernel == "conv_wgrad_bf16_kernel"]
    assert {(c.cin, c.cout) for c in bf} == set(wc.BF16_ONE_SHAPES) | {(64, 64)} and {c.K for c in bf if (c.cin, c.cout) == (64, 64)} == {8, 1}
    thin = [c for c in CASES if c.kernel == "conv_wgrad_thin_kernel"]
    assert {(c.cin, c.cout) for c in thin} == set(wc.THIN_SHAPES) and {c.K for c in thin} == {27, 8} and {c.form for c in thin} == {"order", "null"}
    assert {c.cin * c.cout for c in thin} >= {1, 255, 256, 257, 4095, 4032}
    for kernel in ("conv_wgrad_kernel", "conv_wgrad_slice_kernel<5, 2>", "conv_wgrad_bf16_kernel", "conv_wgrad_bf16_slice_kernel<3>"):
        assert any(c.form == "null" for c in CASES if c.kernel == kernel), kernel
    assert {c.kind for c in CASES} == {"dense", "sparse", "steps"}
    assert {c.n_in for c in CASES} >= {1, 97} and any(c.n_in > c.n_out for c in CASES) and any(97 < c.n_in < c.n_out for c in CASES)
    # the child processes: every (O, AHEAD) and bf16 O the launch code accepts, and the switched-off slice kernel
    assert {(e.O, e.ahead) for e in CHILD_ENVS if e.slice} == {(o, a) for o in wc.SLICE_OS for a in wc.AHEADS}
    assert {e.bf16_O for e in CHILD_ENVS} | {DEFAULT_ENV.bf16_O} == set(wc.BF16_OS) and any(not e.slice for e in CHILD_ENVS)
    for env in CHILD_ENVS:
        cases = wc.child_cases(env)
        assert len({c.id for c in cases}) == len(cases)
        assert max(c.n_out for c in cases if not c.bf16) > wc.SLICE_SECOND[0] and max(c.n_out for c in cases if c.bf16) > wc.SLICE_SECOND[0]
        assert {c.n_out for c in cases} >= set(wc.SLICE_STEP + wc.ONE_STEP + wc.STEP_ROWS)


def _plan_sweep(L):
    """every launch the plan emits on a grid of shapes: cin, cout 32 .. 256 by 32 and thin widths, K 27 / 8 / 1, fp32 and
    bf16, the table's row counts"""
    rows = sorted({c.n_out for c in CASES})
    widths = list(range(32, 257, 32)) + [1, 2, 3, 5, 16, 63, 65, 85]
    emitted = set()
    for bf16 in (False, True):
        for K in (27, 8, 1):
            for cin in widths:
                for cout in widths:
                    for n_out in rows:
                        plan = wc.planned(L, bf16, K, cin, cout, n_out)
                        if isinstance(plan, tuple):            # (an error code: the entry point refuses the shape)
                            assert plan == wc.expected_plan(bf16, K, cin, cout, n_out), (bf16, K, cin, cout, n_out, plan)
                            emitted.add(launch_key(*plan, cin, cout))
    return emitted


def unreached(emitted, cases):
    return sorted(emitted - {launch_key(c.kernel, c.split, c.partials, c.cin, c.cout) for c in cases})


def test_table_reaches_every_launch_the_plan_can_emit(pcc):
    """fails, naming the kernels, when plan_wgrad can emit a launch no table row runs — until the table follows a changed
    plan; and the check itself works: without its rows, a kernel is reported by name"""
    emitted = _plan_sweep(pcc.lib())
    assert len(emitted) == 7, sorted(emitted)
    assert not unreached(emitted, CASES), unreached(emitted, CASES)
    assert unreached(emitted, [c for c in CASES if "bf16_slice" not in c.kernel]) == [("conv_wgrad_bf16_slice_kernel<3>", 1)]
    assert unreached(emitted, [c for c in CASES if c.partials != 4 * c.split]) == [("conv_wgrad_kernel", 2)]
    assert unreached(emitted, [c for c in CASES if not (c.bf16 and c.K != 27 and c.cin == 64)]) == [("conv_wgrad_bf16_kernel", 2)]


def test_refused_shapes_have_no_plan(pcc):
    L = pcc.lib()
    for bf16, K, cin, cout in ((True, 27, 96, 64), (True, 27, 64, 32), (False, 28, 64, 64), (False, 0, 64, 64), (False, 27, 4097, 1),
                               (False, 27, 17, 241), (True, 28, 64, 64)):
        assert isinstance(wc.planned(L, bf16, K, cin, cout, 1000), int) and wc.planned(L, bf16, K, cin, cout, 1000) != 0
    assert wc.planned(L, False, 27, 64, 64, 0) == ("", 0, 0)
    assert L.pcc_conv_wgrad_kernel_name(0, 27, 64, 64, 1000, None, 0, None, None) == 0
    import ctypes
    small = ctypes.create_string_buffer(8)
    assert L.pcc_conv_wgrad_kernel_name(0, 27, 64, 64, 1000, small, len(small), None, None) != 0


@pytest.mark.parametrize("n_out,n_in,K,kind", [(13793, 6903, 27, "dense"), (6881, 97, 27, "dense"), (530003, 531004, 27, "sparse"),
                                               (270001, 1, 27, "sparse"), (262145, 131079, 8, "sparse"), (257, 135, 8, "dense"),
                                               (33, 1034, 27, "dense"), (1, 1, 1, "dense")])
def test_synthetic_map_has_the_planted_corners(n_out, n_in, K, kind):
    m = wc.build_map(n_out, n_in, K, kind)
    nbr, gm, P = m.nbr, m.gmask, m.planted
    groups, full = (n_out + 31) // 32, n_out // 32
    assert nbr.shape == (n_out, K) and nbr.dtype == np.int32 and nbr.min() >= -1 and nbr.max() < n_in
    assert np.array_equal(np.sort(m.order), np.arange(n_out)) and gm.shape == (groups,)
    rm = wc.row_masks(nbr)
    assert all(int(gm[g]) == int(np.bitwise_or.reduce(rm[32 * g:32 * g + 32])) for g in {0, groups // 2, groups - 1})
    assert nbr[-1, 0] >= 0 and nbr[-1, K - 1] >= 0 and gm[-1] != 0                             # the final group keeps data, in its last row too
    if n_out % 32 > 1:
        assert (rm[32 * (groups - 1):] != 0).sum() * 2 >= n_out % 32
    if full < 12:
        return
    assert all(gm[g] == 0 for g in P["empty"]) and P["empty"][0] == 0 and P["empty"][2] in (groups - 2, full - 1 if n_out % 32 else full - 2)
    assert gm[P["only_first"]] == 1 and gm[P["only_last"]] == 1 << (K - 1)
    if K == 27:
        sets5 = lambda g: [(int(gm[g]) >> (5 * j)) & 31 for j in range(6)]
        assert sets5(P["one_of_set"]) == [0, 4, 0, 0, 0, 0]                                     # exactly offset 7 of the set 5 .. 9
        assert sets5(P["all_of_set"]) == [0, 0, 31, 0, 0, 0]
        assert sets5(P["none_of_set"])[1] == 0 and all(v for j, v in enumerate(sets5(P["none_of_set"])) if j != 1)
        assert [int(rm[r]) for r in P["last_set_rows"]] == [1 << 25, 1 << 26, 3 << 25]         # rows present only in the last set
    if K >= 5:
        row, k = P["lone"]
        assert int((nbr[:, k] >= 0).sum()) == 1 and nbr[row, k] >= 0                           # an offset one row has
    flat = nbr[nbr >= 0]
    assert np.unique(flat).shape[0] < flat.shape[0]                                             # repeated input rows
    pairs = int(flat.shape[0])
    if kind == "sparse":
        assert 150_000 * K // 27 < pairs < 600_000 and (gm == 0).mean() > 0.8           # a few hundred thousand pairs at K = 27
        for start in (wc.MASKS_PER_LOAD * wc.ONE_CAP, wc.MASKS_PER_LOAD * wc.SLICE_CAP):       # work behind the second mask load
            if groups > start:
                assert (gm[start:] != 0).sum() >= min(groups - start, 150) and gm[start] != 0
    else:
        assert 0.2 < float((nbr >= 0).mean()) < 0.3 and int(wc.pairs_per_offset(nbr).max()) <= wc.WIDE_MAX_PAIRS


@pytest.mark.parametrize("n_out,O", [(256, 5), (512, 5), (768, 5), (768, 3), (512, 9), (768, 4), (256, 6)])
def test_step_patterns_give_every_step_count(n_out, O):
    """the "steps" maps: with a split of 8 the workgroups of the slice kernels run 0, 1, 2, 3, 4 and O steps on their first
    group, and at 512 / 768 rows meet an empty group in front of, behind and between populated ones"""
    m = wc.build_map(n_out, n_out // 2 + 7, 27, "steps", O)
    groups, sets = n_out // 32, (27 + O - 1) // O
    steps = np.array([[bin((int(m.gmask[g]) >> (j * O)) & ((1 << O) - 1)).count("1") for j in range(sets)] for g in range(groups)])
    assert all(steps[g, j] == wc.step_count(g, j, min(O, 27 - j * O)) for g in range(groups) for j in range(sets))
    per_wg = {tuple(steps[s::8, j]) for s in range(8) for j in range(sets - 1)}               # (the ragged last set aside)
    assert {p[0] for p in per_wg} == {0, 1, 2, 3, 4, O} - ({4} if O == 3 else set())
    if n_out >= 512:
        assert any(p[0] == 0 and p[1] > 0 for p in per_wg) and any(p[0] > 0 and p[1] == 0 for p in per_wg)
    if n_out >= 768:
        assert any(p[0] > 0 and p[1] == 0 and p[2] > 0 for p in per_wg)
    assert any(int((m.nbr[32 * g:32 * g + 32, k] >= 0).sum()) == 1 for g in range(groups) for k in range(27))    # a single row of a group


def test_second_pop_of_an_iteration_reloads_the_masks():
    """the two-groups form of conv_wgrad_kernel behind its cap: in the cases above 262,144 rows, workgroup (offset 0, split 0)
    meets an odd number of live groups in its first 64 masks and live groups behind them, so the iteration's second pop()
    is the one that loads masks again — by construction of the map, not by chance"""
    two = [c for c in CASES if c.kernel == "conv_wgrad_kernel" and c.partials == 4 * c.split and c.n_out > wc.ONE_SECOND[0]]
    assert len(two) >= 2 and all(c.split == wc.ONE_CAP for c in two)
    for c in two:
        gm = wc.case_map(c).gmask
        assert wc.second_pop_reloads(gm), c.id
        assert int((gm[wc.MASKS_PER_LOAD * wc.ONE_CAP::wc.ONE_CAP] & 1).sum()) >= 1, c.id          # offset 0 behind the reload
    assert not wc.second_pop_reloads(np.full(9000, 0xFFFFFFFF, dtype=np.uint32))                    # (all 64 live: even)


def test_operand_families_are_exact_by_construction():
    """the condition, on the cases with the most pairs per offset of each family; and that the wide families carry the bits
    they claim (fp32: 12-bit mantissas; bf16: 8-bit, unchanged by the conversion)"""
    import torch
    for pick in ("f32-128x128-n13793-", "bf16-128x128-n13793-", "f32-64x64-n530003-", "f32-96x160-n270001-"):
        case = next(c for c in CASES if c.id.startswith(pick))
        m = wc.case_map(case)
        fams = wc.families_of(case, m)
        assert fams == (("int", "wide", "mirror") if case.n_out < 20000 else ("int",))
        for family in fams:
            X, G, unit_product = wc.operands(case, family)
            wc.assert_exact(case, m, family, unit_product)
            assert X.shape == (case.n_in, case.cin) and G.shape == (case.n_out, case.cout) and X.dtype == G.dtype == np.float32
            if case.bf16:
                assert np.array_equal(torch.from_numpy(X).to(torch.bfloat16).float().numpy(), X)
                assert np.array_equal(torch.from_numpy(G).to(torch.bfloat16).float().numpy(), G)
            if family == "wide":
                wide = X * (16 if case.bf16 else 256)
                assert np.array_equal(wide, np.rint(wide)) and np.abs(wide).max() == (255 if case.bf16 else 2047)
                assert (wide.astype(np.int64) & 1).any() and set(np.unique(G).tolist()) == {-2.0, -1.0, 1.0, 2.0}
    # the reference notices one dropped and one doubled pair
    case = next(c for c in CASES if c.id.startswith("f32-64x64-n6881-"))
    m = wc.case_map(case)
    X, G, _ = wc.operands(case, "int")
    want = wc.reference(m.nbr, m.order, X, G)
    pos = int(np.nonzero(m.nbr[:, 13] >= 0)[0][5])
    dropped = m.nbr.copy()
    dropped[pos, 13] = -1
    assert not np.array_equal(wc.reference(dropped, m.order, X, G)[13], want[13])
    again = np.full((1, 27), -1, dtype=np.int32)              # one more position that repeats the pair
    again[0, 13] = m.nbr[pos, 13]
    doubled = wc.reference(np.concatenate([m.nbr, again]), np.append(m.order, m.order[pos]), X, G)
    assert not np.array_equal(doubled[13], want[13]) and all(np.array_equal(doubled[k], want[k]) for k in range(27) if k != 13)


# ---- on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_planned_kernel_matches_its_exact_reference(pcc, case):
    pairs = wc.run_case(pcc, case)
    print(case.id, case.kernel, case.split, case.partials, pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("env", CHILD_ENVS, ids=["slice%d-O%d-ahead%d-bf16O%d" % e for e in CHILD_ENVS])
def test_switched_kernels_in_a_child(pcc, env):
    """the kernel instances behind the once-per-process switches, each in a process of its own, on the 64-channel-class rows
    of the table (wc.child_cases): small row counts, step patterns, both split steps, a launch with a second mask load"""
    cases = wc.child_cases(env)
    f32 = wc.expected_plan(False, 27, 64, 64, 1000, env)[0]
    bf16 = wc.expected_plan(True, 27, 64, 64, 1000, env)[0]
    assert f32 == (f"conv_wgrad_slice_kernel<{env.O}, {env.ahead}>" if env.slice else "conv_wgrad_kernel")
    assert bf16 == (f"conv_wgrad_bf16_slice_kernel<{env.bf16_O}>" if env.bf16_O else "conv_wgrad_bf16_kernel")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_wgrad_plan_child.py")
    try:
        r = subprocess.run([sys.executable, child, f32, bf16], env=dict(os.environ, **wc.env_vars(env)), capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"the child ran past {CHILD_TIMEOUT_S} s; its last lines:\n" + "\n".join(out.splitlines()[-10:]))
    tail = "\n".join((r.stdout + "\n" + r.stderr).splitlines()[-25:])
    print(tail)
    assert r.returncode == 0, tail
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("OK ")]
    assert len(ok) == len(cases) and any(ln.startswith(f"RAN {len(cases)} ") for ln in r.stdout.splitlines()), tail
    assert {ln.split(" ", 2)[2] for ln in ok} == {f32, bf16}


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,bf16,kernel", [(64, 64, False, "conv_wgrad_slice_kernel<5, 2>"), (128, 128, False, "conv_wgrad_kernel"),
                                                  (64, 64, True, "conv_wgrad_bf16_slice_kernel<3>"), (128, 128, True, "conv_wgrad_bf16_kernel")])
def test_library_map_and_order_on_a_shell(pcc, cin, cout, bf16, kernel):
    """the library's own kernel map, mask order and permuted table (CoordMap.position_ordered_table) on a shuffled 63 k-row
    shell — a split above the minimum — on small-integer data: equality with a BLAS reference over oracle.coords.kernel_map
    (float32 is exact here: every sum stays below 2^24)"""
    import torch
    from oracle import coords as oc
    from pcc_amd import _lib
    L = pcc.lib()
    p = pcc.synthetic.sphere_shell(128, 50.0, 1.0)[:, :3]
    c = np.concatenate([np.zeros((p.shape[0], 1)), p], axis=1).astype(np.int32)
    c = c[np.random.default_rng(128).permutation(c.shape[0])]
    n = c.shape[0]
    name, split, partials = wc.planned(L, bf16, 27, cin, cout, n)
    assert name == kernel and split > wc.SPLIT_MIN, (n, name, split)
    rng = np.random.default_rng([cin, cout, 9])
    X = rng.integers(-3, 4, size=(n, cin)).astype(np.float32)
    G = rng.integers(-3, 4, size=(n, cout)).astype(np.float32)
    assert n * 9 < 2 ** 24
    m = pcc.CoordMap(torch.from_numpy(c).to(DEV), 1)
    nbr_sorted, order, gmask, _ = m.position_ordered_table(m, 3)
    dt = torch.bfloat16 if bf16 else torch.float32
    x, g = torch.from_numpy(X).to(DEV).to(dt), torch.from_numpy(G).to(DEV).to(dt)
    dw = torch.empty((27, cin, cout), dtype=torch.float32, device=DEV)
    ne = L.pcc_conv_wgrad_scratch_elems(27, cin, cout)
    scratch = torch.empty(ne, dtype=torch.float32, device=DEV)
    fn = L.pcc_conv_wgrad_bf16 if bf16 else L.pcc_conv_wgrad
    _lib.check(fn(_lib.ptr(x), n, cin, _lib.ptr(g), n, cout, _lib.ptr(nbr_sorted), _lib.ptr(order), _lib.ptr(gmask), 27, _lib.ptr(dw),
                  _lib.ptr(scratch), ne, _lib.stream()))
    got = dw.cpu().numpy()
    nbr = oc.kernel_map(c, c, 3, 1)
    want = np.zeros((27, cin, cout), dtype=np.float32)
    for k in range(27):
        rows = np.nonzero(nbr[:, k] >= 0)[0]
        want[k] = X[nbr[rows, k]].T @ G[rows]
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, (kernel, split, bad.tolist(), float(np.abs(got - want).max()))


# ---- the two map helpers of the backward-data path ---------------------------------------------------------------------
def injective_map(n_out, n_in, K, seed=0):
    """nbr [n_out, K]: every (input row, offset) is read by at most one output row, as in a real map; the input rows of the
    last tenth (at least one, when there are two) are read by nobody"""
    rng = np.random.default_rng([n_out, n_in, K, seed, 23])
    nbr = np.full((n_out, K), -1, dtype=np.int32)
    readable = n_in - max(1, n_in // 10) if n_in >= 2 else n_in
    for k in range(K if readable else 0):
        cnt = int(min(n_out, readable) * rng.uniform(0.2, 0.9)) if min(n_out, readable) > 1 else min(n_out, readable)
        nbr[rng.choice(n_out, cnt, replace=False), k] = rng.choice(readable, cnt, replace=False)
    return nbr, readable


def transpose_reference(nbr, n_in):
    n_out, K = nbr.shape
    nbr_t = np.full((n_in, K), -1, dtype=np.int32)
    mask_t = np.zeros(n_in, dtype=np.uint32)
    j, k = np.nonzero(nbr >= 0)
    nbr_t[nbr[j, k], k] = j
    np.bitwise_or.at(mask_t, nbr[j, k], (np.uint32(1) << k.astype(np.uint32)))
    return nbr_t, mask_t


TRANSPOSE_SHAPES = [(1, 1), (1, 7), (255, 255), (255, 97), (257, 300), (257, 1), (100003, 100003), (100003, 60001), (60001, 100003),
                    (0, 33), (33, 0), (0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [27, 8, 1])
@pytest.mark.parametrize("n_out,n_in", TRANSPOSE_SHAPES)
def test_map_transpose_and_row_permutation_match_numpy(pcc, n_out, n_in, K):
    import torch
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    nbr, readable = injective_map(n_out, n_in, K)
    want_t, want_m = transpose_reference(nbr, n_in)
    assert (want_m[readable:] == 0).all() and (n_in < 2 or n_out == 0 or want_m.any())
    G = 64                                                      # guard elements around both outputs
    d_nbr = torch.from_numpy(nbr).to(DEV)
    t_whole = torch.full((G + n_in * K + G,), 12345, dtype=torch.int32, device=DEV)
    m_whole = torch.full((G + n_in + G,), 12345, dtype=torch.int32, device=DEV)
    _lib.check(L.pcc_kernel_map_transpose(ptr(d_nbr), n_out, K, n_in, ptr(t_whole[G:]), ptr(m_whole[G:]), _lib.stream()))
    t_host, m_host = t_whole.cpu().numpy(), m_whole.cpu().numpy()
    assert np.array_equal(t_host[G:G + n_in * K].reshape(n_in, K), want_t)
    assert np.array_equal(m_host[G:G + n_in].view(np.uint32), want_m)
    assert (t_host[:G] == 12345).all() and (t_host[G + n_in * K:] == 12345).all() and (m_host[:G] == 12345).all() and (m_host[G + n_in:] == 12345).all()
    # unread input rows: all -1, mask 0 (also when nothing reads anything)
    assert (want_t[readable:] == -1).all() and (t_host[G + readable * K:G + n_in * K] == -1).all()
    # pcc_permute_map_rows against nbr[order]
    # (the entry point wants non-null tables also for an empty map: one spare element keeps the empty ones addressable)
    order = np.random.default_rng([n_out, K]).permutation(n_out).astype(np.int32)
    d_order = torch.from_numpy(np.append(order, np.int32(0))).to(DEV)
    d_table = torch.from_numpy(np.append(nbr.reshape(-1), np.int32(0))).to(DEV)
    s_whole = torch.full((G + n_out * K + G,), 12345, dtype=torch.int32, device=DEV)
    _lib.check(L.pcc_permute_map_rows(ptr(d_table), ptr(d_order), n_out, K, ptr(s_whole[G:]), _lib.stream()))
    s_host = s_whole.cpu().numpy()
    assert np.array_equal(s_host[G:G + n_out * K].reshape(n_out, K), nbr[order])
    assert (s_host[:G] == 12345).all() and (s_host[G + n_out * K:] == 12345).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,n_out,n_in", [(64, 64, 5003, 3001), (64, 128, 3001, 5003), (64, 128, 257, 255)])
def test_backward_data_over_the_transposed_map_is_exact(pcc, cin, cout, n_out, n_in):
    """dX[i] = sum_k dY[j(i, k)] W[k]^T: the transposed map through pcc_order_rows_by_mask and pcc_conv_fwd with W[k]^T on
    small integers (at most 27 * cout terms of magnitude <= 9: exact in any order) equals the float64 sum"""
    import torch
    from pcc_amd import _lib
    L, ptr, check = pcc.lib(), _lib.ptr, _lib.check
    K = 27
    nbr, _ = injective_map(n_out, n_in, K, seed=1)
    rng = np.random.default_rng([cin, cout, n_out])
    dY = rng.integers(-3, 4, size=(n_out, cout)).astype(np.float32)
    W = rng.integers(-3, 4, size=(K, cin, cout)).astype(np.float32)
    assert K * cout * 9 < 2 ** 24
    want = np.zeros((n_in, cin))
    for k in range(K):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        want[nbr[j, k]] += dY[j].astype(np.float64) @ W[k].T.astype(np.float64)
    d_nbr = torch.from_numpy(nbr).to(DEV)
    nbr_t = torch.empty((n_in, K), dtype=torch.int32, device=DEV)
    mask_t = torch.empty(n_in, dtype=torch.int32, device=DEV)
    check(L.pcc_kernel_map_transpose(ptr(d_nbr), n_out, K, n_in, ptr(nbr_t), ptr(mask_t), _lib.stream()))
    order = torch.empty(n_in, dtype=torch.int32, device=DEV)
    gmask = torch.empty((n_in + 31) // 32, dtype=torch.int32, device=DEV)
    nbytes = L.pcc_order_scratch_bytes(n_in)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    check(L.pcc_order_rows_by_mask(ptr(mask_t), None, n_in, -1, 1, ptr(order), ptr(gmask), ptr(scratch), nbytes, _lib.stream()))
    wt = torch.from_numpy(np.ascontiguousarray(W.transpose(0, 2, 1))).to(DEV)            # [K, cout, cin]
    wp = torch.empty(L.pcc_conv_packed_elems(K, cout, cin), dtype=torch.float32, device=DEV)
    check(L.pcc_conv_pack_weights(ptr(wt), K, cout, cin, ptr(wp), _lib.stream()))
    bias = torch.zeros(cin, dtype=torch.float32, device=DEV)
    dx = torch.full((n_in, cin), wc.SENTINEL, dtype=torch.float32, device=DEV)
    g = torch.from_numpy(dY).to(DEV)
    check(L.pcc_conv_fwd(ptr(g), n_out, cout, ptr(wt), ptr(wp), ptr(bias), ptr(nbr_t), ptr(order), ptr(gmask), K, ptr(dx), n_in, cin, 0,
                         None, None, _lib.stream()))
    got = dx.cpu().numpy().astype(np.float64)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:8].tolist(), float(np.abs(got - want).max()))


# ---- refusals: a nonzero code and nothing launched -----------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_launches_touch_nothing(pcc):
    import torch
    case = wc.make_case(False, 64, 64, 257)
    m = wc.case_map(case)
    X, G, _ = wc.operands(case, "int")
    want = wc.reference(m.nbr, m.order, X, G)

    def refused(run, **kw):
        rc, _ = run.launch(**kw)
        assert rc != 0 and bool((run.dw_whole == wc.SENTINEL).all()), (run.case.id, kw, rc)

    run = wc.Runner(pcc, case, m, X, G)
    rc, dw = run.launch()
    assert rc == 0 and np.array_equal(dw.cpu().numpy(), want)                                  # (the launcher itself works)
    refused(run, scratch_elems=run.scratch_elems - 1)                                          # scratch one element too small
    xpad = torch.zeros(case.n_in * case.cin + 4, dtype=torch.float32, device=DEV)
    refused(run, x=xpad[1:])                                                                   # fin misaligned by 4 bytes on an MFMA shape
    refused(run, nbr=None)                                                                     # nbr = NULL
    for bf16, cin, cout, K in ((False, 4097, 1, 27), (True, 96, 64, 27), (False, 64, 64, 28), (True, 64, 64, 28)):
        c = wc.Case("refused", bf16, cin, cout, 257, case.n_in, K, "order", "dense", "", 8, 8)
        mm = wc.build_map(257, case.n_in, min(K, 27))
        r = wc.Runner(pcc, c._replace(K=min(K, 27)), mm, np.zeros((case.n_in, cin), np.float32), np.zeros((257, cout), np.float32))
        r.case, r.elems = c, 27 * cin * cout
        refused(r)
    # bf16: its own scratch bound (split x K x cin x cout)
    cb = wc.make_case(True, 64, 64, 257)
    rb = wc.Runner(pcc, cb, m, X, G)
    refused(rb, scratch_elems=cb.partials * rb.elems - 1)
    refused(rb, nbr=None)
    # no output rows: dw is zero-filled, nothing else is written
    for bf16 in (False, True):
        c0 = wc.make_case(bf16, 64, 64, 257)._replace(n_out=0, partials=0)
        r0 = wc.Runner(pcc, c0, m, X, G)
        rc, dw = r0.launch()
        assert rc == 0 and bool((dw == 0).all())
