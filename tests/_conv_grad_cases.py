"""Geometries, operand families, exact references and the case table of tests/test_conv_grad_exact.py: the layer backward
of the sparse convolutions (`SparseConvFn` in autograd.py, `CoordMap.transposed_ordered_map` / `conv_map(adjoint=True)` in
sparse.py, `pcc_kernel_map_transpose` in csrc/conv_bwd.hip) against float64 numpy on `oracle.coords.kernel_map`.

    out   = b + sum_k X[nbr[:, k]] W[k]
    dX[i] = sum over (j, k) with nbr[j, k] = i of dY[j] W[k]^T
    dW[k] = X[nbr[ok, k]]^T dY[ok]
    db    = sum_j dY[j]

References are EXACT.  A floating-point sum does not depend on its order when every partial sum is representable, so the
operands come from grids for which that holds, and `assert_exact` asserts the condition per output tensor: the largest sum of
|a| |b| over the terms of one output element, in units of the product grid, is below 2^24.
  int     X, W, dY, bias in {-3 .. 3}                          (exact in fp32, bf16 and x3 arithmetic at every size used here)
  wideX   X = m / 256, |m| < 2048; W, dY in {+-1, +-2}          a path that drops operand bits fails these; fp32 and x3 are
  wideG   dY = m / 256, |m| < 2048; X, W in {+-1, +-2}          exact on them, a bf16 launch computes the float64 value of the
  wideW   W = m / 256, |m| < 2048; X, dY in {+-1, +-2}          operands rounded to bf16 (still on the grid: still exact)
Which launches round is the documented rule, restated in `expected_mode` / `taken_width` / `launches`:
  forward  bf16 iff asked for and cin % 64 == 0; x3 iff asked for, cin % 32 == 0 and the output width rounded up to 32 is a
           multiple of 64; else fp32                                  (sparse.launch_mode, csrc/conv.hip: check_shape, plan_conv)
  dW       bf16 iff the forward ran in bf16: X and dY rounded        (autograd.py: the saved input is the bf16 copy)
  dX       the same rule on the adjoint shape (dY width -> cin), the dY width being the first one >= cout that the fp32 plan
           takes (a multiple of 32, or a thin width whose weights fit the LDS): dY and W^T rounded
  db       always from the unrounded dY
Every comparison is np.array_equal: no tolerance anywhere.
"""
import collections
import functools

import numpy as np

from oracle import coords as oc

MODE_F32, MODE_BF16, MODE_X3 = 0, 1, 2
MODES = ("f32", "bf16", "x3")                      # neither switch, set_bf16, set_x3
EXACT_LIMIT = 2 ** 24

# ---- geometries ------------------------------------------------------------------------------------------------------------
SIZES = ("one", "five", "patch70", "shell1k", "shell9k")
TINY = ("one", "five", "patch70")
KINDS = ("same3", "k1", "down", "up2", "up3", "pruned", "batch")


def shell(grid, radius, thick):
    g = np.stack(np.meshgrid(*[np.arange(grid)] * 3, indexing="ij"), -1).reshape(-1, 3)
    keep = np.abs(np.linalg.norm(g - (grid - 1) / 2, axis=1) - radius) < thick
    return g[keep].astype(np.int32)


@functools.lru_cache(maxsize=None)
def points(size):
    """[n, 3] voxels of a geometry (stride 1), at an odd origin so that stride-2 cells straddle the set, in shuffled row order"""
    if size == "one":
        p = np.array([[0, 0, 0]], dtype=np.int32)
    elif size == "five":                              # a bent chain: neighbours along every axis
        p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 1, 0], [2, 1, 1]], dtype=np.int32)
    elif size == "patch70":                           # 7 x 5 x 2
        p = np.stack(np.meshgrid(np.arange(7), np.arange(5), np.arange(2), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    elif size == "shell1k":
        p = shell(20, 6.0, 1.2)                       # 1,088 rows
    elif size == "shell9k":
        p = shell(48, 22.0, 0.75)                     # 9,224 rows
    else:
        raise KeyError(size)
    p = p + np.array([3, 5, 7], dtype=np.int32)
    return p[np.random.default_rng([len(p), 3]).permutation(len(p))]


def with_batch(p, b=0):
    return np.concatenate([np.full((p.shape[0], 1), b, dtype=np.int32), p.astype(np.int32)], axis=1)


# in: input coordinates [n_in, 4] and their tensor stride; out: output coordinates in the ORACLE's row order; nbr [n_out, K]
# (None for kernel size 1); layer: "conv" | "up"; own_out: the output set is handed to the layer as `out_map`
Sets = collections.namedtuple("Sets", "kind size coords stride out nbr ksize layer lstride own_out")


@functools.lru_cache(maxsize=None)
def sets_of(kind, size):
    p = points(size)
    c = with_batch(p)
    if kind == "same3":
        return Sets(kind, size, c, 1, c, oc.kernel_map(c, c, 3, 1), 3, "conv", 1, False)
    if kind == "k1":
        return Sets(kind, size, c, 1, c, None, 1, "conv", 1, False)
    if kind == "down":
        out = oc.stride_map(c, 1)
        return Sets(kind, size, c, 1, out, oc.kernel_map(c, out, 3, 1), 3, "conv", 2, False)
    if kind in ("up2", "up3"):
        k = int(kind[-1])
        c2 = c * np.array([1, 2, 2, 2], dtype=np.int32)
        out = oc.children(c2, 2, k)
        return Sets(kind, size, c2, 2, out, oc.kernel_map(c2, out, k, 1, transposed=True), k, "up", 2, False)
    if kind == "pruned":                              # a full set onto a pruned subset of itself (about 60 %, at least one row)
        keep = np.random.default_rng([len(c), 17]).random(len(c)) < 0.6
        keep[0] = True
        out = c[keep][::-1].copy()
        return Sets(kind, size, c, 1, out, oc.kernel_map(c, out, 3, 1), 3, "conv", 1, True)
    if kind == "batch":                               # two items that overlap in (x, y, z): item 1 = item 0 moved by one voxel, a third dropped
        q = (p + np.array([1, 0, 0], dtype=np.int32))[: max(1, (2 * len(p)) // 3)] if len(p) > 1 else p
        c = np.concatenate([with_batch(p, 0), with_batch(q, 1)], axis=0)
        c = c[np.random.default_rng([len(c), 19]).permutation(len(c))]
        return Sets(kind, size, c, 1, c, oc.kernel_map(c, c, 3, 1), 3, "conv", 1, False)
    raise KeyError(kind)


def table_of(s):
    """the map as a table also for kernel size 1 (every row reads itself)"""
    return np.arange(s.coords.shape[0], dtype=np.int64)[:, None] if s.nbr is None else s.nbr


# ---- numpy transposition of a kernel map -------------------------------------------------------------------------------------
def transpose_reference(nbr, n_in):
    """for every (j, k) with i = nbr[j, k] >= 0: nbr_t[i, k] = j and mask_t[i] |= 1 << k; everything else -1 / 0"""
    K = nbr.shape[1]
    nbr_t = np.full((n_in, K), -1, dtype=np.int32)
    mask_t = np.zeros(n_in, dtype=np.uint32)
    for k in range(K):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        i = nbr[j, k]
        assert np.unique(i).size == i.size, "an (input row, offset) pair is read by two output rows"
        nbr_t[i, k] = j
        mask_t[i] |= np.uint32(1 << k)
    return nbr_t, mask_t


def group_or(mask, order):
    """OR of `mask` over the rows order[32 g : 32 g + 32]"""
    m = np.zeros((order.shape[0] + 31) // 32 * 32, dtype=np.uint32)
    m[:order.shape[0]] = mask[order]
    return np.bitwise_or.reduce(m.reshape(-1, 32), axis=1)


def injective_map(n_out, n_in, K, unread=0, seed=0):
    """synthetic nbr [n_out, K]: every (input row, offset) is read by at most one output row, as in a real map; the last `unread`
    input rows are read by nobody"""
    rng = np.random.default_rng([n_out, n_in, K, seed, 29])
    nbr = np.full((n_out, K), -1, dtype=np.int32)
    readable = n_in - unread
    for k in range(K):
        cnt = min(n_out, readable)
        cnt = cnt if cnt <= 1 else max(1, int(cnt * rng.uniform(0.3, 1.0)))
        nbr[rng.choice(n_out, cnt, replace=False), k] = rng.choice(readable, cnt, replace=False)
    return nbr


# ---- operand families --------------------------------------------------------------------------------------------------------
FAMILIES = ("int", "wideX", "wideG", "wideW")
WIDE = ("wideX", "wideG", "wideW")
Operands = collections.namedtuple("Operands", "X W b dY grids")           # float32 arrays; grids: unit of X, W, dY


def _draw(rng, what, shape):
    if what == "int":
        return rng.integers(-3, 4, size=shape).astype(np.float32)
    if what == "pm":
        return rng.choice(np.array([-2, -1, 1, 2], dtype=np.float32), size=shape)
    return (rng.integers(-2047, 2048, size=shape) / 256.0).astype(np.float32)          # "wide": 11-bit mantissas


def operands(s, cin, cout, family, bias=True):
    """X [n_in, cin], W [K, cin, cout], bias [cout] (integers in every family), dY [n_out, cout] in the oracle's row order"""
    roles = {"int": ("int", "int", "int"), "wideX": ("wide", "pm", "pm"), "wideW": ("pm", "wide", "pm"), "wideG": ("pm", "pm", "wide")}[family]
    K = s.ksize ** 3
    rng = np.random.default_rng([s.coords.shape[0], s.out.shape[0], cin, cout, K, FAMILIES.index(family)])
    X = _draw(rng, roles[0], (s.coords.shape[0], cin))
    W = _draw(rng, roles[1], (K, cin, cout))
    dY = _draw(rng, roles[2], (s.out.shape[0], cout))
    b = rng.integers(-3, 4, size=cout).astype(np.float32) if bias else None
    return Operands(X, W, b, dY, tuple(1.0 / 256 if r == "wide" else 1.0 for r in roles))


def bf16_round(a):
    """round to nearest even onto bf16, returned as float32 (numpy on the bits; NaN and infinities do not occur here)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


# ---- float64 references ------------------------------------------------------------------------------------------------------
def ref_out(nbr, X, W, b, n_out):
    out = np.zeros((n_out, W.shape[2]))
    X, W = X.astype(np.float64), W.astype(np.float64)
    for k in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        if j.size:
            out[j] += X[nbr[j, k]] @ W[k]
    return out if b is None else out + b.astype(np.float64)[None, :]


def ref_dx(nbr, dY, W, n_in):
    dX = np.zeros((n_in, W.shape[1]))
    dY, W = dY.astype(np.float64), W.astype(np.float64)
    for k in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        if j.size:
            dX[nbr[j, k]] += dY[j] @ W[k].T            # (input rows of one offset are distinct: transpose_reference asserts it)
    return dX


def ref_dw(nbr, X, dY):
    dW = np.zeros((nbr.shape[1], X.shape[1], dY.shape[1]))
    X, dY = X.astype(np.float64), dY.astype(np.float64)
    for k in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        if j.size:
            dW[k] = X[nbr[j, k]].T @ dY[j]
    return dW


def ref_db(dY):
    return dY.astype(np.float64).sum(axis=0)


def assert_exact(s, ops, who=""):
    """the condition under which no sum depends on its order, per output tensor: the largest sum of |a| |b| over the terms of one
    output element, in units of the product grid, is below 2^24.  A cheap upper bound first (term count times the largest
    product); the sum itself where the bound does not settle it.  -> {tensor: units}"""
    nbr = table_of(s)
    n_in, n_out = s.coords.shape[0], s.out.shape[0]
    X, W, dY = np.abs(ops.X), np.abs(ops.W), np.abs(ops.dY)
    b = None if ops.b is None else np.abs(ops.b)
    gx, gw, gg = ops.grids
    mx, mw, mg = float(X.max()), float(W.max()), float(dY.max())
    mb = 0.0 if b is None else float(b.max())
    per_out = int((nbr >= 0).sum(axis=1).max())
    per_in = int(np.bincount(nbr[nbr >= 0].ravel(), minlength=n_in).max())
    pairs = int((nbr >= 0).sum(axis=0).max())
    bound = {"out": ((per_out * X.shape[1] * mx * mw + mb) / (gx * gw), lambda: ref_out(nbr, X, W, b, n_out).max() / (gx * gw)),
             "dX": (per_in * dY.shape[1] * mg * mw / (gg * gw), lambda: ref_dx(nbr, dY, W, n_in).max() / (gg * gw)),
             "dW": (pairs * mx * mg / (gx * gg), lambda: ref_dw(nbr, X, dY).max() / (gx * gg)),
             "db": (n_out * mg / gg, lambda: ref_db(dY).max() / gg)}
    worst = {}
    for name, (cheap, exact) in bound.items():
        worst[name] = cheap if cheap < EXACT_LIMIT else float(exact())
        assert worst[name] < EXACT_LIMIT, f"{who or (s.kind, s.size)}: {name} is not exact: a sum of |a||b| reaches {worst[name]:.0f} grid units (>= 2^24)"
    return worst


# ---- the launch rule, restated -------------------------------------------------------------------------------------------------
THIN_CIN = (1, 2, 3, 4, 6, 8, 12, 16, 24)
THIN_LDS_BYTES = 160 * 1024


def round_up(v, unit):
    return (v + unit - 1) // unit * unit


def fp32_takes(cin, cout, K):
    if cin % 32 == 0:
        return cin <= 256
    return cin in THIN_CIN and K * cin * cout * 4 <= THIN_LDS_BYTES


def expected_mode(bf16, x3, cin, cout):
    """the arithmetic of a forward-kernel launch of input width cin (the first asked-for mode whose kernel takes the shape)"""
    if bf16 and cin % 64 == 0 and cin <= 256:
        return MODE_BF16
    if x3 and cin % 32 == 0 and cin <= 256 and round_up(cout, 32) % 64 == 0:
        return MODE_X3
    return MODE_F32


def taken_width(cout, cin, K):
    """the width backward-data reads dY at: the first one >= cout that the fp32 plan takes"""
    return next((c for c in range(cout, cout + 32) if fp32_takes(c, cin, K)), cout)


Launches = collections.namedtuple("Launches", "fwd adj width wgrad_bf16 cin_p cout_p db_kernel")


def launches(mode, cin, cout, K):
    """what one forward + backward of a layer launches under `mode` ("f32" | "bf16" | "x3")"""
    bf16, x3 = mode == "bf16", mode == "x3"
    fwd = expected_mode(bf16, x3, cin, cout)
    width = taken_width(cout, cin, K)
    adj = expected_mode(bf16, x3, width, cin)
    unit = 64 if fwd == MODE_BF16 else 32
    return Launches(fwd, adj, width, fwd == MODE_BF16, round_up(cin, unit), round_up(cout, unit), cout % 4 == 0 and cout <= 1024)


def expected(s, ops, mode, cin, cout):
    """{out, dX, dW, db} in float64, with the operands of exactly the bf16 launches rounded to bf16"""
    nbr = table_of(s)
    n_in, n_out = s.coords.shape[0], s.out.shape[0]
    ln = launches(mode, cin, cout, nbr.shape[1])
    r = bf16_round
    X, W, dY = ops.X, ops.W, ops.dY
    return {"out": ref_out(nbr, r(X), r(W), ops.b, n_out) if ln.fwd == MODE_BF16 else ref_out(nbr, X, W, ops.b, n_out),
            "dX": ref_dx(nbr, r(dY), r(W), n_in) if ln.adj == MODE_BF16 else ref_dx(nbr, dY, W, n_in),
            "dW": ref_dw(nbr, r(X), r(dY)) if ln.wgrad_bf16 else ref_dw(nbr, X, dY),
            "db": None if ops.b is None else ref_db(dY)}


# ---- the case table ----------------------------------------------------------------------------------------------------------
SHAPES = ((128, 128), (64, 64), (64, 128), (192, 64), (96, 160), (4, 64), (2, 128), (64, 3), (128, 2), (32, 3), (2, 2), (64, 100), (64, 4))
SIZE_SUBSET = ((128, 128), (64, 64), (64, 3), (4, 64))
WIDE_SHAPES = ((128, 128), (64, 64), (64, 128), (4, 64), (64, 3))
WIDE_KINDS = ("same3", "down", "up3")
WIDE_SIZES = ("shell1k", "patch70")
VARIANT_SHAPES = ((128, 128), (4, 64))               # one wide, one thin
VARIANT_KINDS = ("same3", "down", "up3")
EPILOGUE_ACTS = (0, 1, 2)                             # identity, ReLU, leaky ReLU (sparse.ACT_*)


def shapes_of(size):
    return SHAPES if size == "shell1k" else SIZE_SUBSET


def int_cases():
    """(kind, mode, size) in an order that keeps the cases of one (kind, size) together: their references are shared"""
    return [(kind, mode, size) for kind in KINDS for size in SIZES for mode in MODES]


def wide_cases():
    return [(kind, mode, size) for kind in WIDE_KINDS for size in WIDE_SIZES for mode in MODES]


def all_layer_cases():
    """(kind, size, mode, cin, cout, family) of every plain layer case of the table"""
    for kind, mode, size in int_cases():
        for cin, cout in shapes_of(size):
            yield kind, size, mode, cin, cout, "int"
    for kind, mode, size in wide_cases():
        for cin, cout in WIDE_SHAPES:
            for family in WIDE:
                yield kind, size, mode, cin, cout, family


def describe_mismatch(who, name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return f"{who}: {name} has shape {got.shape}, want {want.shape}"
    bad = got != want
    lead = np.nonzero(bad.reshape(bad.shape[0], -1).any(axis=1))[0] if bad.ndim > 1 else np.nonzero(bad)[0]
    first = tuple(int(v[0]) for v in np.nonzero(bad))
    what = "offsets" if name == "dW" else "columns" if name == "db" else "rows"
    return (f"{who}: {name}: {int(bad.sum())} of {bad.size} values differ, in {lead.size} {what} {lead[:12].tolist()}{' ...' if lead.size > 12 else ''}; "
            f"first at {name}{list(first)}: got {got[first]!r}, want {want[first]!r}; max |diff| {float(np.abs(got - want).max()):.6g}")
