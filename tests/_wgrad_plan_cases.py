"""Case table, synthetic maps, exact references and the launch driver of tests/test_wgrad_plans.py (and of its child
processes, tests/_wgrad_plan_child.py): the weight-gradient kernels of csrc/conv_bwd.hip, per launch.

    dW[k] = sum over positions p with nbr[p, k] >= 0 of X[nbr[p, k]]^T dY[order[p]]

`nbr` is indexed by execution position, `order` maps a position to its dY row, `gmask` holds one offset mask per 32 positions.

The table names, per row, the kernel, the split count and the number of partial images the plan (`plan_wgrad`) must pick;
`expected_plan` restates the plan from its constants, so the row counts sit where the plan changes its mind.

References are EXACT.  A floating-point sum does not depend on its order when every partial sum is representable, so the
inputs come from two families for which that holds, and the case builder asserts the condition (`assert_exact`: the largest
number of pairs of one offset times the largest |x| times the largest |g|, in units of the grid, is below 2^24):
  int      X, dY in {-3 .. 3}                      (exact in bf16 too; up to 1.8 M pairs per offset)
  wide     X = m / 256, |m| < 2048, dY in {+-1, +-2}   (fp32 kernels; bf16 kernels: m / 16, |m| < 256); at most 4,096 pairs per
  mirror   the same with the roles swapped              offset: an fp32 path that drops operand bits fails these
The reference is a float64 matmul per offset, compared with np.array_equal: no tolerance anywhere.
"""
import collections
import ctypes
import functools

import numpy as np

from _conv_plan_cases import SENTINEL, group_masks, row_masks

# ---- the plan's constants (csrc/conv_bwd.hip) ---------------------------------------------------------------------------
SPLIT_MIN = 8
ONE_GROUPS, ONE_CAP = 48, 128          # wgrad_splits: clamp(groups / 48, 8, 128)        (one-offset kernels, fp32 and bf16)
SLICE_GROUPS, SLICE_CAP = 24, 256      # wgrad_slice_splits: clamp(groups / 24, 8, 256)  (slice kernels, fp32 and bf16)
THIN_SPLIT = 256                       # WG_SPLIT_THIN: row ranges of the thin kernel, per = ceil(n_out / 256)
MASKS_PER_LOAD = 64                    # group masks a workgroup inspects per load
WIDE_MAX_PAIRS = 4096                  # pairs per offset up to which the wide-mantissa families are exact

Env = collections.namedtuple("Env", "slice O ahead bf16_O")     # PCC_WGRAD_SLICE, _SLICE_O, _AHEAD, PCC_WGRAD_BF16_SLICE_O
DEFAULT_ENV = Env(1, 5, 2, 3)
SLICE_OS, AHEADS, BF16_OS = (3, 4, 5, 6, 9), (1, 2), (0, 3, 5, 9)       # what the launch code accepts


def splits(n_out, per, cap):
    return min(max(((n_out + 31) // 32) // per, SPLIT_MIN), cap)


def last_rows_of_split(per, s):
    """largest n_out whose split count is still s (SPLIT_MIN <= s < cap)"""
    return 32 * (per * (s + 1) - 1)


def first_second_load(cap):
    """largest n_out at which no workgroup of a capped launch loads masks a second time"""
    return 32 * MASKS_PER_LOAD * cap


def expected_plan(bf16, K, cin, cout, n_out, env=DEFAULT_ENV):
    """(kernel name, split, partials) of a launch — the plan restated"""
    sixty4 = cin <= 64 and cout <= 64
    if bf16:
        if env.bf16_O and (cin, cout, K) == (64, 64, 27):
            s = splits(n_out, SLICE_GROUPS, SLICE_CAP)
            return f"conv_wgrad_bf16_slice_kernel<{env.bf16_O}>", s, s
        s = splits(n_out, ONE_GROUPS, ONE_CAP)
        return "conv_wgrad_bf16_kernel", s, s
    if cin % 32 or cout % 32:
        return "conv_wgrad_thin_kernel", THIN_SPLIT, THIN_SPLIT
    if env.slice and sixty4 and K == 27:
        s = splits(n_out, SLICE_GROUPS, SLICE_CAP)
        return f"conv_wgrad_slice_kernel<{env.O}, {env.ahead}>", s, s
    s = splits(n_out, ONE_GROUPS, ONE_CAP)
    return "conv_wgrad_kernel", s, s * (4 if sixty4 else 1)


def planned(L, bf16, K, cin, cout, n_out):
    """pcc_conv_wgrad_kernel_name -> (name, split, partials), or the error code"""
    buf = ctypes.create_string_buffer(96)
    split, partials = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = L.pcc_conv_wgrad_kernel_name(int(bf16), K, cin, cout, n_out, buf, len(buf), ctypes.byref(split), ctypes.byref(partials))
    return (buf.value.decode(), split.value, partials.value) if rc == 0 else rc


# ---- the case table --------------------------------------------------------------------------------------------------
# form: "order" = a random order with exact masks, "natural" = order NULL with exact masks, "null" = order NULL and gmask NULL.
# kind: "dense" (25 % neighbour density, planted corners), "sparse" (large row counts: most groups empty), "steps" (masks
# that give the slice kernels' workgroups 0, 1, 2, 3, 4 and O steps).
Case = collections.namedtuple("Case", "id bf16 cin cout n_out n_in K form kind kernel split partials")

ONE_ROWS_SMALL = (1, 31, 32, 33, 256, 257)
ONE_STEP = (last_rows_of_split(ONE_GROUPS, 8), last_rows_of_split(ONE_GROUPS, 8) + 1)                  # 13,792 / 13,793
ONE_CAPPED = (last_rows_of_split(ONE_GROUPS, ONE_CAP - 1), last_rows_of_split(ONE_GROUPS, ONE_CAP - 1) + 1)   # 196,576 / 196,577
ONE_SECOND = (first_second_load(ONE_CAP), first_second_load(ONE_CAP) + 1)                              # 262,144 / 262,145
SLICE_ROWS_SMALL = (1, 31, 32, 33, 256, 257, 512)
SLICE_STEP = (last_rows_of_split(SLICE_GROUPS, 8), last_rows_of_split(SLICE_GROUPS, 8) + 1)            # 6,880 / 6,881
SLICE_CAPPED = (last_rows_of_split(SLICE_GROUPS, SLICE_CAP - 1), last_rows_of_split(SLICE_GROUPS, SLICE_CAP - 1) + 1)   # 196,576 / 196,577
SLICE_SECOND = (first_second_load(SLICE_CAP), first_second_load(SLICE_CAP) + 1)                        # 524,288 / 524,289
THIN_ROWS = (1, 255, 256, 257, 5000)
STEP_ROWS = (256, 512, 768)            # 8, 16 and 24 groups: one, two and three groups per workgroup of a split of 8

ONE_SHAPES = ((128, 128), (96, 160), (160, 96), (32, 128), (256, 32), (256, 256), (64, 192))
SLICE_SHAPES = ((64, 64), (32, 64), (64, 32), (32, 32))
BF16_ONE_SHAPES = ((128, 128), (64, 128), (192, 256), (256, 64))
THIN_SHAPES = ((1, 1), (2, 2), (3, 5), (16, 16), (3, 85), (1, 257), (63, 65), (64, 63), (4, 64), (64, 1))


def n_in_form(n_out, i):
    """input row counts that differ from the output's: about half, one row, far fewer, more"""
    return (n_out // 2 + 7, 1, 97, n_out + 1001)[i % 4]


def make_case(bf16, cin, cout, n_out, K=27, form="order", kind=None, n_in=None, env=DEFAULT_ENV):
    kind = kind or ("dense" if n_out <= 20000 else "sparse")
    if n_in is None:                                        # from the row's own fields: adding a row changes no other row
        n_in = n_in_form(n_out, (cin // 32 + cin + 3 * (cout // 32 + cout) + 5 * n_out + K + 2 * bool(bf16)) % 4)
    kernel, split, partials = expected_plan(bf16, K, cin, cout, n_out, env)
    cid = f"{'bf16' if bf16 else 'f32'}-{cin}x{cout}-n{n_out}-in{n_in}-K{K}-{form}-{kind}"
    return Case(cid, bool(bf16), cin, cout, n_out, n_in, K, form, kind, kernel, split, partials)


def _build_cases():
    C = []
    add = lambda *a, **k: C.append(make_case(*a, **k))
    # one-offset fp32: every count of live chunks per block (cbi, cbo = 1 .. 4), two blocks per dimension
    for cin, cout in ONE_SHAPES:
        for n in ONE_ROWS_SMALL:
            add(False, cin, cout, n)
    for cin, cout in ((128, 128), (96, 160)):
        for K in (8, 1):
            for n in (33, 257):
                add(False, cin, cout, n, K=K)
    for cin, cout in ONE_SHAPES:                            # the partial layout at another split; the second mask load
        for n in ONE_STEP + ((ONE_SECOND[1],) if cin * cout < 65536 else ()):
            add(False, cin, cout, n)
    add(False, 128, 128, 257, form="null")
    add(False, 160, 96, 256, form="natural")
    for n in ONE_CAPPED:
        add(False, 128, 128, n)
    add(False, 160, 96, 200003)
    add(False, 128, 128, ONE_SECOND[0])
    add(False, 32, 128, ONE_SECOND[0])
    add(False, 256, 32, 270001)
    add(False, 96, 160, 270001)
    # 64-channel-class blocks of another kernel size: the one-offset kernel's two-groups-per-iteration form (4 x split partials)
    for cin, cout in ((64, 64), (32, 64), (64, 32)):
        for K in (8, 1):
            for n in (1, 33, 256, 257, 13000, ONE_STEP[1]):
                add(False, cin, cout, n, K=K)
    add(False, 64, 64, ONE_SECOND[1], K=8)
    add(False, 32, 32, 270001, K=8)
    # slice fp32: 64 x 64 and the shapes with dead tiles
    for cin, cout in SLICE_SHAPES:
        for n in SLICE_ROWS_SMALL:
            add(False, cin, cout, n)
    for cin, cout in SLICE_SHAPES:
        for n in SLICE_STEP + (SLICE_SECOND[1],):
            add(False, cin, cout, n)
    add(False, 64, 64, 512, form="null")
    add(False, 64, 32, 257, form="natural")
    for cin, cout in ((64, 64), (32, 32)):
        for n in STEP_ROWS:
            add(False, cin, cout, n, kind="steps")
    for n in SLICE_CAPPED + SLICE_SECOND[:1]:
        add(False, 64, 64, n)
    add(False, 64, 64, 530003)
    add(False, 32, 32, 530003)
    # bf16 one-offset
    for cin, cout in BF16_ONE_SHAPES:
        for n in ONE_ROWS_SMALL:
            add(True, cin, cout, n)
    for K in (8, 1):                                       # 64 x 64: two row groups per iteration, odd and even numbers of live groups
        for n in (1, 33, 256, 257, 13000, ONE_STEP[1]):
            add(True, 64, 64, n, K=K)
    add(True, 128, 128, 257, form="null")
    for cin, cout in BF16_ONE_SHAPES:
        for n in ONE_STEP + (ONE_SECOND[1],):
            add(True, cin, cout, n)
    add(True, 128, 128, ONE_SECOND[0])
    for n in ONE_CAPPED:
        add(True, 64, 128, n)
    add(True, 256, 64, 200003)
    add(True, 192, 256, 270001)
    add(True, 64, 64, 270001, K=8)
    # bf16 slice
    for n in SLICE_ROWS_SMALL + SLICE_STEP + SLICE_CAPPED + SLICE_SECOND + (530003,):
        add(True, 64, 64, n)
    for n in STEP_ROWS:
        add(True, 64, 64, n, kind="steps")
    add(True, 64, 64, 512, form="null")
    # thin: the edges of pairs = cin * cout (255 / 256 / 257, 4095, no power of two) and of per = ceil(n_out / 256).  The shapes
    # with pairs < 256 (row lanes summed through LDS) run the whole cross of K and order form at every row count; the others
    # alternate, so that each of those shapes still sees both K and both forms, but not at every row count
    for si, (cin, cout) in enumerate(THIN_SHAPES):
        for ri, n in enumerate(THIN_ROWS):
            if cin * cout < 256:
                for K in (27, 8):
                    for form in ("order", "null"):
                        add(False, cin, cout, n, K=K, form=form)
            else:
                add(False, cin, cout, n, K=(27, 8)[(si + ri) % 2], form=("order", "null")[((si + ri) // 2) % 2])
    return C


CASES = _build_cases()


def child_cases(env):
    """the 64-channel-class rows a child process runs under the switches `env`: the small row counts, the step patterns, both
    split steps, and one launch whose workgroups load masks a second (one-offset kernel: a third) time"""
    C = []
    add = lambda *a, **k: C.append(make_case(*a, env=env, **k))
    for n in SLICE_ROWS_SMALL:
        add(False, 64, 64, n)
    for cin, cout in SLICE_SHAPES[1:]:
        for n in (33, 257, 512):
            add(False, cin, cout, n)
    for n in STEP_ROWS:
        add(False, 64, 64, n, kind="steps")
        add(True, 64, 64, n, kind="steps")
    add(False, 32, 32, 768, kind="steps")
    for n in SLICE_STEP + ONE_STEP:
        add(False, 64, 64, n)
    add(False, 64, 64, SLICE_SECOND[1])
    for n in (33, 257, 512, SLICE_STEP[1], ONE_STEP[1], SLICE_SECOND[1]):
        add(True, 64, 64, n)
    return C


# (O, AHEAD, bf16 O) per child; PCC_WGRAD_SLICE=0 is one more child.  The bf16 switch is independent of the fp32 ones, so its
# values ride along.
CHILD_ENVS = [Env(1, O, ahead, BF16_OS[(2 * i + j) % 4]) for i, O in enumerate(SLICE_OS) for j, ahead in enumerate(AHEADS)] + [Env(0, 5, 2, 0)]


def env_vars(env):
    return {"PCC_WGRAD_SLICE": str(env.slice), "PCC_WGRAD_SLICE_O": str(env.O), "PCC_WGRAD_AHEAD": str(env.ahead),
            "PCC_WGRAD_BF16_SLICE_O": str(env.bf16_O)}


# ---- synthetic maps --------------------------------------------------------------------------------------------------
Map = collections.namedtuple("Map", "nbr order gmask planted")


def _fill_groups(nbr, groups, n_in, density, rng):
    n_out, K = nbr.shape
    rows = (np.asarray(groups, dtype=np.int64)[:, None] * 32 + np.arange(32)[None, :]).reshape(-1)
    rows = rows[rows < n_out]
    present = rng.random((rows.shape[0], K)) < density
    nbr[rows] = np.where(present, rng.integers(0, n_in, size=(rows.shape[0], K), dtype=np.int32), np.int32(-1))


def _only(nbr, g, offsets, n_in, rng, every_row=False):
    """group g holds exactly `offsets`: each in a random half of its rows (at least one)"""
    rows = np.arange(32 * g, min(32 * g + 32, nbr.shape[0]))
    nbr[rows] = -1
    for k in offsets:
        on = rows if every_row else rows[rng.random(rows.shape[0]) < 0.5]
        if on.size == 0:
            on = rows[:1]
        nbr[on, k] = rng.integers(0, n_in, size=on.shape[0])


@functools.lru_cache(maxsize=4)
def build_map(n_out, n_in, K, kind="dense", O=5, seed=0):
    """nbr [n_out, K] by execution position (-1 = absent), a random order, exact group masks, and the planted corners
    (`planted`: name -> group / row / (row, offset)):
      - whole groups without a neighbour: the first, a middle one and the last full one in front of the final group; the final
        group (the ragged tail) keeps data, and the last row holds offsets 0 and K - 1;
      - (K = 27) groups that hold exactly one offset of a slice set (7), all offsets of one (10 .. 14) and all but one set's
        (none of 5 .. 9); a group with only offset 0, one with only offset K - 1;
      - (K >= 5) offset 3 present in a single row of the whole map; (K = 27) rows present only in the last set (25, 26);
      - repeated input rows (n_in below the number of pairs).
    kind "sparse": most groups are empty: one dense stretch of 200 groups, 900 scattered ones, and — so that every
    workgroup finds work behind its second mask load — up to 200 of the groups from 64 x 128 and from 64 x 256 on.
    kind "steps": see steps_map."""
    rng = np.random.default_rng([n_out, n_in, K, seed, 11])
    groups, full = (n_out + 31) // 32, n_out // 32
    if kind == "steps":
        nbr, planted = steps_map(n_out, n_in, K, O, rng), {}
    else:
        nbr = np.full((n_out, K), -1, dtype=np.int32)
        planted = {}
        if kind == "dense":
            _fill_groups(nbr, np.arange(groups), n_in, 0.25 if n_out >= 256 else 0.5, rng)
        else:
            live = [np.arange(groups // 3, groups // 3 + 200), rng.choice(groups, 900, replace=False), np.arange(groups - 3, groups)]
            for start in (MASKS_PER_LOAD * ONE_CAP, MASKS_PER_LOAD * SLICE_CAP):
                if groups > start:
                    behind = np.arange(start, groups)
                    live.append(behind if behind.size <= 200 else np.concatenate([behind[:4], behind[-2:], rng.choice(behind, 194, replace=False)]))
            _fill_groups(nbr, np.unique(np.concatenate(live)), n_in, 0.25, rng)
        if full >= 12:
            last = full - 1 if n_out % 32 else full - 2          # the last full group in front of the final one, which keeps data
            free = [g for g in rng.permutation(np.arange(1, last)).tolist() if g != full // 2]
            planted.update(empty=(0, full // 2, last))
            for g in planted["empty"]:
                nbr[32 * g:32 * g + 32] = -1
            planted["only_first"], planted["only_last"] = free[0], free[1]
            _only(nbr, free[0], [0], n_in, rng)
            _only(nbr, free[1], [K - 1], n_in, rng)
            if K == 27:
                planted["one_of_set"], planted["all_of_set"], planted["none_of_set"] = free[2], free[3], free[4]
                _only(nbr, free[2], [7], n_in, rng)
                _only(nbr, free[3], [10, 11, 12, 13, 14], n_in, rng)
                _only(nbr, free[4], [k for k in range(27) if not 5 <= k <= 9], n_in, rng, every_row=True)
                rows = 32 * free[5] + np.array([3, 17, 30])
                nbr[rows] = -1
                nbr[rows[0], 25], nbr[rows[1], 26] = rng.integers(0, n_in, 2)
                nbr[rows[2], 25:27] = rng.integers(0, n_in, 2)
                planted["last_set_rows"] = tuple(int(r) for r in rows)
            if K >= 5:
                row = 32 * free[6] + 9
                nbr[:, 3] = -1
                nbr[row, 3] = rng.integers(0, n_in)
                planted["lone"] = (int(row), 3)
        # the one-offset kernel at its cap, two row groups per iteration: workgroup (offset 0, split 0) finds an ODD number of
        # live groups behind its first mask load, so the second pop() of an iteration is what loads masks again
        start = MASKS_PER_LOAD * ONE_CAP
        if groups > start and not second_pop_reloads(group_masks(row_masks(nbr))):
            taken = {v for val in planted.values() for v in (val if isinstance(val, tuple) else (val,))} | {r // 32 for r in planted.get("last_set_rows", ())} | {planted.get("lone", (0,))[0] // 32}
            g = next(g for g in range(ONE_CAP, start, ONE_CAP) if g not in taken and nbr[32 * g:32 * g + 32, 0].max() < 0)
            nbr[32 * g + 5, 0] = rng.integers(0, n_in)
        # the ragged tail keeps data; the last row holds the first and the last offset
        tail = np.arange(32 * (groups - 1), n_out)
        nbr[tail[::2], K - 1] = rng.integers(0, n_in, size=tail[::2].shape[0])
        nbr[n_out - 1, 0] = rng.integers(0, n_in)
        nbr[n_out - 1, K - 1] = rng.integers(0, n_in)
    order = rng.permutation(n_out).astype(np.int32)
    return Map(nbr, order, group_masks(row_masks(nbr)), planted)


def second_pop_reloads(gmask, k=0, s=0, split=ONE_CAP):
    """true when the groups s, s + split, ... of the first mask load that hold offset k number an odd count (and masks remain
    behind): in the two-groups form of conv_wgrad_kernel the iteration's second pop() then triggers the next load"""
    first = gmask[s:MASKS_PER_LOAD * split:split]
    return gmask.shape[0] > MASKS_PER_LOAD * split + s and int(((first >> np.uint32(k)) & 1).sum()) % 2 == 1


STEP_PATTERN = (0, 1, 2, 3, 4, -1)        # -1: every offset of the set


def step_count(g, j, width):
    p = STEP_PATTERN[(g + j) % len(STEP_PATTERN)]
    return width if p < 0 else min(p, width)


def steps_map(n_out, n_in, K, O, rng):
    """group g holds step_count(g, j, .) offsets of slice set j (offsets j O .. j O + O - 1), each in a random half of its rows:
    with a split of 8, workgroup (set j, s) owns groups s, s + 8, s + 16 and so runs 0, 1, 2, 3, 4 or O steps on one group, on
    two groups (an empty one in front, behind), on three (an empty one between)"""
    nbr = np.full((n_out, K), -1, dtype=np.int32)
    for g in range((n_out + 31) // 32):
        rows = np.arange(32 * g, min(32 * g + 32, n_out))
        for j in range((K + O - 1) // O):
            width = min(O, K - j * O)
            for k in j * O + rng.choice(width, step_count(g, j, width), replace=False):
                on = rows[rng.random(rows.shape[0]) < (0.5 if (g + k) % 3 else 0.04)]
                if on.size == 0:
                    on = rows[int(rng.integers(0, rows.shape[0]))][None]
                nbr[on, k] = rng.integers(0, n_in, size=on.shape[0])
                if rows[-1] == n_out - 1:                                  # the last row of the map holds every offset of its group
                    nbr[n_out - 1, k] = rng.integers(0, n_in)
    return nbr


def case_map(case, O=5):
    return build_map(case.n_out, case.n_in, case.K, case.kind, O if case.kind == "steps" else 5)


# ---- operands of the two exact families ----------------------------------------------------------------------------------
POOL = 8191


@functools.lru_cache(maxsize=None)
def _pool(what, seed):
    rng = np.random.default_rng([seed, 5])
    if what == "int":
        return rng.integers(-3, 4, size=(POOL, 256)).astype(np.float32)
    if what == "pm":
        return rng.choice(np.array([-2, -1, 1, 2], dtype=np.float32), size=(POOL, 256))
    if what == "wide32":
        return (rng.integers(-2047, 2048, size=(POOL, 256)) / 256.0).astype(np.float32)
    return (rng.integers(-255, 256, size=(POOL, 256)) / 16.0).astype(np.float32)      # wide16: 8-bit mantissas, exact in bf16


def _rows_of(pool, n, cols, mul, add):
    return np.ascontiguousarray(pool[:, :cols])[(np.arange(n, dtype=np.int64) * mul + add) % POOL]


# family -> (X pool, dY pool, largest |x| and |g| in units of the grid); "wide" stands for wide32 (fp32) / wide16 (bf16)
def operands(case, family):
    wide = "wide16" if case.bf16 else "wide32"
    wmax = 255 if case.bf16 else 2047
    xs, gs, mx, mg = {"int": ("int", "int", 3, 3), "wide": (wide, "pm", wmax, 2), "mirror": ("pm", wide, 2, wmax)}[family]
    cols = lambda c: max(c, 1)
    X = _rows_of(_pool(xs, 1), case.n_in, cols(case.cin), 7, 3) if case.cin <= 256 else None
    G = _rows_of(_pool(gs, 2), case.n_out, cols(case.cout), 5, 1) if case.cout <= 256 else None
    if X is None:                                           # (1 x 257: wider than the pool)
        X = _rows_of(np.concatenate([_pool(xs, 1), _pool(xs, 3)], axis=1), case.n_in, case.cin, 7, 3)
    if G is None:
        G = _rows_of(np.concatenate([_pool(gs, 2), _pool(gs, 4)], axis=1), case.n_out, case.cout, 5, 1)
    return X, G, mx * mg


def pairs_per_offset(nbr):
    return (nbr >= 0).sum(axis=0)


def families_of(case, m):
    return ("int", "wide", "mirror") if int(pairs_per_offset(m.nbr).max()) <= WIDE_MAX_PAIRS else ("int",)


def assert_exact(case, m, family, unit_product):
    """the condition under which the sums do not depend on their order: max over (k, ci, co) of sum |x| |g| < 2^24 grid units
    (bounded by the offset's pair count times the largest product)"""
    worst = int(pairs_per_offset(m.nbr).max()) * unit_product
    assert worst < 2 ** 24, (case.id, family, worst)
    if family != "int":
        assert int(pairs_per_offset(m.nbr).max()) <= WIDE_MAX_PAIRS, case.id


def reference(nbr, order, X, G):
    """float64, one matmul per offset"""
    K = nbr.shape[1]
    want = np.zeros((K, X.shape[1], G.shape[1]))
    for k in range(K):
        pos = np.nonzero(nbr[:, k] >= 0)[0]
        if pos.size:
            rows = pos if order is None else order[pos]
            want[k] = X[nbr[pos, k]].astype(np.float64).T @ G[rows].astype(np.float64)
    return want


# ---- the launches ----------------------------------------------------------------------------------------------------
FRONT, BACK = 64, 4096        # guard floats (256 bytes in front: the buffers stay 16-byte aligned)


def describe_mismatch(case, what, got, want, m):
    bad = got != want
    ks = np.nonzero(bad.any(axis=(1, 2)))[0]
    k = int(ks[0])
    ci, co = (int(v[0]) for v in np.nonzero(bad[k]))
    last = np.nonzero(m.nbr[-1] >= 0)[0].tolist()
    return (f"{case.id}: {case.kernel} (split {case.split}, {case.partials} partials), {what}: offsets {ks.tolist()} differ "
            f"({int(bad.sum())} of {bad.size} values; pairs of those offsets {pairs_per_offset(m.nbr)[ks].tolist()[:9]}); first at "
            f"dW[{k}, {ci}, {co}]: got {got[k, ci, co]!r}, want {want[k, ci, co]!r}; max |diff| {float(np.abs(got - want).max()):.6g}; "
            f"the last row (position {case.n_out - 1}) holds offsets {last}")


class Runner:
    """one case and operand family on the device: uploaded once, launched under the mask forms"""

    def __init__(self, pcc, case, m, X, G, dev="cuda:0"):
        import torch
        from pcc_amd import _lib
        self.torch, self._lib, self.L, self.case, self.dev = torch, _lib, pcc.lib(), case, dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.x, self.g = t(X), t(G)
        if case.bf16:
            self.x, self.g = self.x.to(torch.bfloat16), self.g.to(torch.bfloat16)
        self.nbr = t(m.nbr)
        self.order = None if case.form != "order" else t(m.order)
        self.masks = {"exact": t(m.gmask.view(np.int32)), "null": None,
                      "ones": torch.full((m.gmask.shape[0],), -1, dtype=torch.int32, device=dev)}
        self.elems = case.K * case.cin * case.cout
        self.scratch_elems = self.L.pcc_conv_wgrad_scratch_elems(case.K, case.cin, case.cout)

    def launch(self, masks="exact", scratch_elems=None, x=None, nbr="given"):
        """one launch into guarded buffers -> (return code, dw on the device); the guards are checked when it ran"""
        torch, case, L, ptr = self.torch, self.case, self.L, self._lib.ptr
        se = self.scratch_elems if scratch_elems is None else scratch_elems
        dw_whole = torch.full((FRONT + self.elems + BACK,), SENTINEL, dtype=torch.float32, device=self.dev)
        sc_whole = torch.full((FRONT + max(se, 0) + BACK,), SENTINEL, dtype=torch.float32, device=self.dev)
        dw, scratch = dw_whole[FRONT:FRONT + self.elems], sc_whole[FRONT:]
        assert dw.data_ptr() % 16 == 0 and scratch.data_ptr() % 16 == 0
        fn = L.pcc_conv_wgrad_bf16 if case.bf16 else L.pcc_conv_wgrad
        rc = fn(ptr(self.x if x is None else x), case.n_in, case.cin, ptr(self.g), case.n_out, case.cout,
                ptr(self.nbr) if nbr == "given" else None, ptr(self.order), ptr(self.masks[masks]), case.K, ptr(dw), ptr(scratch), se,
                self._lib.stream())
        torch.cuda.synchronize()
        self.dw_whole = dw_whole
        if rc != 0:
            return rc, dw
        used = case.partials * self.elems if case.n_out > 0 else 0
        who = f"{case.id}: {case.kernel} (masks '{masks}')"
        assert bool((dw_whole[:FRONT] == SENTINEL).all()) and bool((dw_whole[FRONT + self.elems:] == SENTINEL).all()), who + " wrote outside dw"
        assert bool((sc_whole[:FRONT] == SENTINEL).all()), who + " wrote in front of the scratch"
        assert bool((sc_whole[FRONT + used:] == SENTINEL).all()), who + f" wrote past the {case.partials} partials of its scratch"
        return rc, dw.view(case.K, case.cin, case.cout)


def run_case(pcc, case, O=None):
    """every check of one table row; raises AssertionError naming the case, the kernel and where the values differ"""
    import torch
    L = pcc.lib()
    got_plan = planned(L, case.bf16, case.K, case.cin, case.cout, case.n_out)
    assert got_plan == (case.kernel, case.split, case.partials), f"{case.id}: the plan is {got_plan}, the table says {case[-3:]}"
    m = case_map(case, O or (DEFAULT_ENV.bf16_O if case.bf16 else DEFAULT_ENV.O))
    order = m.order if case.form == "order" else None
    first = "null" if case.form == "null" else "exact"
    with torch.no_grad():
        for family in families_of(case, m):
            X, G, unit_product = operands(case, family)
            assert_exact(case, m, family, unit_product)
            want = reference(m.nbr, order, X, G)
            run = Runner(pcc, case, m, X, G)
            rc, dw = run.launch(first)
            assert rc == 0, (case.id, rc, L.pcc_last_error())
            got = dw.cpu().numpy()
            assert np.array_equal(got, want), describe_mismatch(case, f"family '{family}', masks '{first}'", got.astype(np.float64), want, m)
            if family != "int":
                continue
            rc, again = run.launch(first)
            assert rc == 0 and torch.equal(again, dw), f"{case.id}: {case.kernel}: two launches differ"
            for masks in ("exact", "null", "ones"):
                if masks != first:
                    rc, other = run.launch(masks)
                    assert rc == 0 and torch.equal(other, dw), describe_mismatch(case, f"masks '{masks}' against '{first}'",
                                                                                 other.cpu().numpy().astype(np.float64), want, m)
    return int(pairs_per_offset(m.nbr).sum())
