"""Case table, synthetic neighbour maps, references and the launch driver of tests/test_conv_plans.py (and of its child
process, tests/_conv_plan_child.py).

The table names, per row, the kernel `plan_conv` (csrc/conv.hip) must pick for that launch; row counts are derived from the
plan's constants below, so the cases sit where the plan changes its mind.  Nothing here reads a geometry: maps are drawn
from a seeded generator with the corners planted by hand (build_map).

References
  fp32   oracle/chain.c (`conv_chain(..., mfma_order=True)`) + the epilogue in numpy float32, every step rounded on its own,
         in the order of the kernels' epilogue (+ bias, * beta, + gamma, activation, + residual; the library is compiled with
         -ffp-contract=off): compared for EQUALITY.
  fp32   a float64 evaluation on sampled rows with the bound derived in `ref64_rows` — independent of the oracle's idea
         of the summation order.
  bf16   the fp32 reference on bf16-rounded operands, tolerances of tests/test_bf16_conv.py.
  x3     float64 on every row, error bounds of tests/test_x3_conv.py.
"""
import collections
import ctypes
import functools
import re

import numpy as np

MODE_F32, MODE_BF16, MODE_X3 = 0, 1, 2
MODE_NAME = ("f32", "bf16", "x3")
MODE_TAG = ("", "[bf16]", "[x3]")

# ---- the plan's constants (csrc/conv.hip: FILL_WGS, ROW32_MAX_WGS, small_max_value) -------------------------------------
FILL_WGS = 768            # 128-wide launches of fewer 64 x 128 workgroups take 64 x 64 tiles
ROW32_MAX_WGS = 3000      # fp32 128-wide launches from FILL_WGS to this take 32 x 128 tiles
SMALL_MAX = 640           # 32 x 32 output tiles the small-launch kernel takes (twice that below 128 columns)
SMALL4_WGS = 256          # ... of which launches up to this many run four chunks per step (cin % 128 == 0)

T64x64, T32x128, T64x128, T128x64, T128x32 = (64, 64), (32, 128), (64, 128), (128, 64), (128, 32)
WAVES = {T64x64: (2, 2), T32x128: (1, 4), T64x128: (2, 2), T128x64: (2, 2), T128x32: (4, 1)}
FP32_TILES = (T64x64, T32x128, T64x128, T128x64, T128x32)


def coutp(cout):
    return (cout + 31) // 32 * 32


def last_rows_64x64(cout):
    """largest n_out of a 128-wide launch still below FILL_WGS workgroups of 64 x 128"""
    return 64 * ((FILL_WGS - 1) // (coutp(cout) // 128))


def last_rows_32x128(cout):
    """largest n_out of a 128-wide fp32 launch still below ROW32_MAX_WGS workgroups of 64 x 128"""
    return 64 * ((ROW32_MAX_WGS - 1) // (coutp(cout) // 128))


def last_rows_small(cout, small=SMALL_MAX):
    """largest n_out the small-launch kernel takes at threshold `small` (doubled for outputs narrower than 128 columns)"""
    cp = coutp(cout)
    return 32 * ((small * (1 if cp % 128 == 0 else 2)) // (cp // 32))


def last_rows_small4(cout):
    return 32 * (SMALL4_WGS // (coutp(cout) // 32))


def tile_name(mode, tile, cch, has_map):
    (bm, bn), (wm, wn) = tile, WAVES[tile]
    return f"conv_mfma_buf_kernel{MODE_TAG[mode]}<{bm}, {bn}, {wm}, {wn}, {cch}, {'true' if has_map else 'false'}>"


def small_name(sc):
    return f"conv_small_kernel<{sc}, {8 if sc == 1 else 3}>"


_BUF = re.compile(r"conv_mfma_buf_kernel<(\d+), (\d+), (\d+), (\d+), \d+, (true|false)>$")


def global_twin(name):
    """the 64-bit-addressed kernel that runs an fp32 tile launch under PCC_CONV_PATH=global (None for any other name)"""
    m = _BUF.match(name)
    return None if m is None else "conv_mfma_kernel<%s, %s, %s, %s, %s>" % m.groups()


def tile_rows(name):
    """output rows per workgroup of a kernel name"""
    m = re.search(r"<(\d+), ", name)
    return 32 if name.startswith("conv_small_kernel") else int(m.group(1))


# ---- the case table --------------------------------------------------------------------------------------------------
# K = 0: no map (nbr == NULL, kernel_size 1, n_in == n_out).  small: the small-launch threshold the case sets.
# epi: bias | film | relu_res | lrelu_film_res.  sub_rows: the first `sub_rows` rows launched on their own must take another
# kernel and give the same values (0 = not run).
Case = collections.namedtuple("Case", "id mode cin cout n_out n_in K small epi kernel sub_rows")
EPILOGUES = ("bias", "film", "relu_res", "lrelu_film_res")
X3_EPILOGUE = "relu_film_res"          # (the form tests/test_x3_conv.py runs)


def _n_in_form(n_out, i):
    """input row counts that differ from the output's: about half, one row, far fewer, more"""
    return (n_out // 2 + 7, 1, 97, n_out + 1001)[i % 4]


def _case(mode, cin, cout, n_out, kernel, K=27, n_in=None, small=SMALL_MAX, epi="bias", sub_rows=0):
    if K == 0:
        n_in = n_out
    elif n_in is None:
        n_in = n_out // 2 + 7
    f = re.findall(r"\d+|true|false", kernel[kernel.index("<"):])
    short = f"small{f[0]}" if kernel.startswith("conv_small") else f"t{f[0]}x{f[1]}c{f[4]}{'m' if f[5] == 'true' else 'n'}"
    cid = f"{MODE_NAME[mode]}-{cin}x{cout}-n{n_out}-in{n_in}-{'K%d' % K if K else 'nomap'}-small{small}-{epi}-{short}"
    return Case(cid, mode, cin, cout, n_out, n_in, K, small, epi, kernel, sub_rows)


def _fp32_tile_shape(tile):
    """(cout, n_out) that plans `tile` in fp32 at the default small threshold, n_out not a multiple of the tile's rows"""
    return {T64x64: (128, last_rows_small(128) + 881),           # 6,001 rows
            T32x128: (128, last_rows_64x64(128) + 915),          # 50,003
            T64x128: (256, last_rows_32x128(256) + 71),          # 96,007
            T128x64: (64, last_rows_small(64) + 101),            # 20,581
            T128x32: (32, last_rows_small(32) + 51)}[tile]       # 41,011


def _build_cases():
    C = []
    # fp32: every chunk count on every tile, with a map and without
    for tile in FP32_TILES:
        cout, n_out = _fp32_tile_shape(tile)
        for has_map in (True, False):
            for cch in range(1, 9):
                if tile in (T32x128, T64x128):
                    sub = 5000                                       # -> the small kernel / the 64 x 64 tile
                else:
                    sub = 5000 if (has_map and tile != T64x64) else 0   # -> the small kernel; no other plan without a map
                C.append(_case(MODE_F32, 32 * cch, cout, n_out, tile_name(MODE_F32, tile, cch, has_map), K=27 if has_map else 0,
                               n_in=_n_in_form(n_out, cch), sub_rows=sub))
    # fp32: both sides of every boundary of the plan
    for cout in (256, 128):
        a, b = last_rows_64x64(cout), last_rows_32x128(cout)         # 24,512 / 95,936 and 49,088 / 191,936
        C += [_case(MODE_F32, 64, cout, a, tile_name(MODE_F32, T64x64, 2, True)),
              _case(MODE_F32, 64, cout, a + 1, tile_name(MODE_F32, T32x128, 2, True)),
              _case(MODE_F32, 64, cout, b, tile_name(MODE_F32, T32x128, 2, True)),
              _case(MODE_F32, 64, cout, b + 1, tile_name(MODE_F32, T64x128, 2, True))]
    for cin, cout, tile in ((96, 128, T64x64), (64, 256, T64x64), (64, 64, T128x64), (32, 32, T128x32), (160, 96, T128x32)):
        s = last_rows_small(cout)                                    # 5,120  2,560  20,480  40,960  13,632
        C += [_case(MODE_F32, cin, cout, s, small_name(2 if cin % 64 == 0 else 1)),
              _case(MODE_F32, cin, cout, s + 1, tile_name(MODE_F32, tile, cin // 32, True))]
    s4 = last_rows_small4(128)                                       # 2,048: four chunks per step up to here
    C += [_case(MODE_F32, 128, 128, s4, small_name(4)), _case(MODE_F32, 128, 128, s4 + 1, small_name(2)),
          _case(MODE_F32, 256, 128, 1000, small_name(4), n_in=1), _case(MODE_F32, 224, 128, 1000, small_name(1), n_in=97)]
    half = last_rows_small(128, 64)                                  # a threshold of the caller's: 64 tiles = 512 rows
    C += [_case(MODE_F32, 128, 128, half, small_name(4), small=64),
          _case(MODE_F32, 128, 128, half + 1, tile_name(MODE_F32, T64x64, 4, True), small=64)]
    # fp32: tiny launches on every tile, the small kernel switched off.  The plan looks at rows x column tiles only, so an
    # output of 768 (3000) column tiles reaches the 32 x 128 (64 x 128) tile with a handful of rows.
    for tile, cin, cout, K in ((T64x64, 64, 128, 27), (T128x64, 64, 64, 27), (T128x32, 96, 32, 27), (T32x128, 32, 128 * FILL_WGS, 3),
                               (T64x128, 32, 128 * ROW32_MAX_WGS, 2)):
        bm = tile[0]
        for n_out in (1, bm - 1, bm, bm + 1):
            C.append(_case(MODE_F32, cin, cout, n_out, tile_name(MODE_F32, tile, cin // 32, True), K=K, n_in=max(5, n_out + 3), small=0))
    # fp32: ragged output widths (padded to 32 columns in the packed weights, never written past `cout`)
    for cin, cout, n_out, tile in ((64, 100, 3001, T64x64), (96, 100, last_rows_64x64(100) + 915, T32x128),
                                   (32, 250, last_rows_32x128(250) + 71, T64x128), (64, 33, 3001, T128x64), (96, 5, 3001, T128x32),
                                   (64, 31, 3001, T128x32), (64, 160, 3001, T128x32), (96, 192, 3001, T128x64)):
        C.append(_case(MODE_F32, cin, cout, n_out, tile_name(MODE_F32, tile, cin // 32, True), small=0))
    C += [_case(MODE_F32, 64, 100, 1000, small_name(2)), _case(MODE_F32, 96, 33, 1000, small_name(1)),
          _case(MODE_F32, 128, 100, 500, small_name(4))]
    # fp32: the fused epilogue forms on every tile and on the small kernel
    for epi in EPILOGUES[1:]:
        for tile in FP32_TILES:
            cout, n_out = _fp32_tile_shape(tile)
            C.append(_case(MODE_F32, 96, cout, n_out, tile_name(MODE_F32, tile, 3, True), epi=epi))
        C.append(_case(MODE_F32, 128, 128, 1500, small_name(4), epi=epi))
        C.append(_case(MODE_F32, 96, 64, 1500, small_name(1), epi=epi))
        C.append(_case(MODE_F32, 64, 128, 50003, tile_name(MODE_F32, T32x128, 2, False), K=0, epi=epi))
    # bf16 (chunks of 64 channels): 64 x 128, 128 x 64 and 128 x 32 at 50 k ragged rows, 64 x 64 below the fill point
    big = last_rows_64x64(128) + 915
    for tile, cout, n_out in ((T64x128, 128, big), (T128x64, 64, big), (T128x32, 32, big), (T64x64, 128, 6001)):
        for has_map in (True, False):
            for cch in range(1, 5):
                C.append(_case(MODE_BF16, 64 * cch, cout, n_out, tile_name(MODE_BF16, tile, cch, has_map), K=27 if has_map else 0,
                               n_in=_n_in_form(n_out, cch), sub_rows=5000 if tile == T64x128 else 0,
                               epi="lrelu_film_res" if cch == 3 else "bias"))
    # x3: 64 x 128 at 50 k rows; 64 x 64 for 64-wide outputs at scale (odd and even chunk counts) and below the fill point
    for tile in (T64x128, T64x64):
        for has_map in (True, False):
            for cch in range(1, 9):
                if tile == T64x128:
                    cout, n_out, sub = 128, big, 5000
                else:
                    cout, n_out, sub = (64, big, 0) if cch in (2, 3) else (128, 6001, 0)
                C.append(_case(MODE_X3, 32 * cch, cout, n_out, tile_name(MODE_X3, tile, cch, has_map), K=27 if has_map else 0,
                               n_in=_n_in_form(n_out, cch), sub_rows=sub, epi=X3_EPILOGUE if cch in (3, 4) else "bias"))
    return C


CASES = _build_cases()


def _in_global_run(c):
    """the rows the 64-bit-addressed run takes: the fp32 chunk sweep (each tile at its `_fp32_tile_shape`, default small
    threshold, bias only) at one even and one odd chunk count, with a map and without"""
    return (c.mode == MODE_F32 and c.epi == "bias" and c.small == SMALL_MAX and c.cin in (64, 96)
            and any(c.kernel == tile_name(MODE_F32, t, c.cin // 32, c.K != 0) and (c.cout, c.n_out) == _fp32_tile_shape(t) for t in FP32_TILES)
            and c.n_in == (c.n_out if c.K == 0 else _n_in_form(c.n_out, c.cin // 32)))


GLOBAL_CASES = [c._replace(kernel=global_twin(c.kernel), sub_rows=0, id=c.id + "-global") for c in CASES if _in_global_run(c)]


def planner_name(L, mode, n_in, cin, cout, n_out, K):
    """pcc_conv_kernel_name, or the negative error code"""
    buf = ctypes.create_string_buffer(160)
    rc = L.pcc_conv_kernel_name(mode, n_in, cin, cout, n_out, K if K else 1, 1 if K else 0, buf, len(buf))
    return buf.value.decode() if rc == 0 else rc


def case_name(L, case, n_out=None):
    n_out = case.n_out if n_out is None else n_out
    return planner_name(L, case.mode, n_out if case.K == 0 else case.n_in, case.cin, case.cout, n_out, case.K)


class small_threshold:
    """sets the small-launch threshold, restores the previous one on the way out"""

    def __init__(self, L, value):
        self.L, self.value = L, value

    def __enter__(self):
        self.was = self.L.pcc_conv_small_max(self.value)

    def __exit__(self, *exc):
        self.L.pcc_conv_small_max(self.was)


# ---- synthetic maps --------------------------------------------------------------------------------------------------
Map = collections.namedtuple("Map", "nbr corners planted lone")


@functools.lru_cache(maxsize=3)
def build_map(n_out, n_in, K, seed=0):
    """nbr [n_out, K] int32 (-1 = absent) at ~25 % density with repeated input rows, and planted:
      - three whole natural groups of 32 rows without any neighbour: the first, the middle one and the last FULL one (the
        ragged tail after it keeps its neighbours, so that a launch's ragged last tile holds rows with data);
      - scattered rows without neighbours, rows whose only neighbour is offset 0, rows whose only neighbour is offset K - 1;
      - a row whose offsets (all but the lone one below) name the same input row;
      - (K >= 3) offset K // 2 present in exactly one row of the launch.
    corners: the planted rows; planted: the three empty groups' rows (None for launches of fewer than 8 groups); lone: (row, k)."""
    rng = np.random.default_rng([n_out, n_in, K, seed])
    present = rng.random((n_out, K)) < 0.25
    nbr = np.where(present, rng.integers(0, n_in, size=(n_out, K), dtype=np.int32), np.int32(-1)).astype(np.int32)
    groups = (n_out + 31) // 32
    corners, planted, lone = [], None, None
    if groups >= 8:
        mid = groups // 2
        last = n_out // 32 - 1
        planted = (np.arange(0, 32), np.arange(32 * mid, 32 * mid + 32), np.arange(32 * last, 32 * last + 32))
        for rows in planted:
            nbr[rows] = -1
            corners += [int(rows[0]), int(rows[-1])]
        free = np.setdiff1d(np.arange(n_out), np.concatenate(planted))
        pick = [int(r) for r in rng.choice(free, 11, replace=False)]
    else:
        pick = list(range(n_out))[:11]
    pick += [None] * 11
    for r in pick[0:3]:
        if r is not None and n_out > 3:
            nbr[r] = -1
    for r in pick[3:6]:
        if r is not None and K >= 2:
            nbr[r] = -1
            nbr[r, 0] = rng.integers(0, n_in)
    for r in pick[6:9]:
        if r is not None and K >= 2:
            nbr[r] = -1
            nbr[r, K - 1] = rng.integers(0, n_in)
    if pick[9] is not None:
        nbr[pick[9]] = rng.integers(0, n_in)
    if K >= 3 and pick[10] is not None:
        nbr[:, K // 2] = -1                            # (also in the row above: every OTHER offset names its one input row)
        nbr[pick[10], K // 2] = rng.integers(0, n_in)
        lone = (pick[10], K // 2)
    corners += [r for r in pick if r is not None]
    return Map(nbr, np.unique(np.array(corners, dtype=np.int64)), planted, lone)


def row_masks(nbr):
    K = nbr.shape[1]
    return np.bitwise_or.reduce((nbr >= 0).astype(np.uint32) << np.arange(K, dtype=np.uint32)[None, :], axis=1).astype(np.uint32)


def group_masks(row_mask, order=None):
    """OR of row_mask over positions 32 g .. 32 g + 31 of the execution order"""
    m = row_mask if order is None else row_mask[order]
    groups = (m.shape[0] + 31) // 32
    pad = np.zeros(32 * groups, dtype=np.uint32)
    pad[:m.shape[0]] = m
    return np.bitwise_or.reduce(pad.reshape(groups, 32), axis=1)


def planted_permutation(n_out, planted, seed=0):
    """a random execution order; the three planted empty groups again fill whole groups of 32 positions: the first, a middle
    one and the last full one, and rows with neighbours fill the ragged tail"""
    rng = np.random.default_rng([n_out, seed, 77])
    if planted is None:
        return rng.permutation(n_out).astype(np.int32)
    first, mid, last = (rng.permutation(p) for p in planted)
    rest = rng.permutation(np.setdiff1d(np.arange(n_out), np.concatenate(planted)))
    a, b = 32 * ((rest.shape[0] // 32) // 2), 32 * (rest.shape[0] // 32)
    order = np.concatenate([mid, rest[:a], first, rest[a:b], last, rest[b:]]).astype(np.int32)
    assert order.shape[0] == n_out
    return order


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _feature_pool(n_in):
    f = np.random.default_rng([n_in, 1]).standard_normal((n_in, 256), dtype=np.float32)
    return f


@functools.lru_cache(maxsize=2)
def _weight_pool(K):
    w = np.random.default_rng([K, 2]).standard_normal((K, 256, 256), dtype=np.float32)
    return w


Inputs = collections.namedtuple("Inputs", "fin w bias nbr film res map")


def make_inputs(case):
    K = case.K if case.K else 1
    fin = np.ascontiguousarray(_feature_pool(case.n_in)[:, :case.cin])
    scale = np.float32(1.0 / np.sqrt(case.cin * 10.0))
    if case.cout <= 256:
        w = np.ascontiguousarray(_weight_pool(K)[:, :case.cin, :case.cout]) * scale
    else:
        w = np.random.default_rng([K, case.cin, case.cout]).standard_normal((K, case.cin, case.cout), dtype=np.float32) * scale
    rng = np.random.default_rng([case.cin, case.cout, case.n_out, 3])
    bias = (rng.standard_normal(case.cout, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    film = res = None
    if "film" in case.epi:
        film = np.concatenate([1 + np.float32(0.1) * rng.standard_normal((case.n_out, case.cout), dtype=np.float32),
                               np.float32(0.1) * rng.standard_normal((case.n_out, case.cout), dtype=np.float32)], axis=1).astype(np.float32)
    if "res" in case.epi:
        res = rng.standard_normal((case.n_out, case.cout), dtype=np.float32)
    m = build_map(case.n_out, case.n_in, case.K) if case.K else None
    return Inputs(fin, w.astype(np.float32), bias, None if m is None else m.nbr, film, res, m)


def act_code(epi):
    return 2 if epi.startswith("lrelu") else 1 if epi.startswith("relu") else 0


def bf16_round(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


# ---- references ------------------------------------------------------------------------------------------------------
def epilogue_f32(c, bias, film, res, act):
    """the kernels' epilogue (csrc/conv.hip, `v = acc + bias; v = v * beta + gamma; v = act(v); v += residual`) in float32,
    one rounding per operation"""
    cout = c.shape[1]
    v = (c + bias[None, :]).astype(np.float32)
    if film is not None:
        v = (v * film[:, :cout]).astype(np.float32)
        v = (v + film[:, cout:]).astype(np.float32)
    if act == 1:
        v = np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    elif act == 2:
        v = np.where(v > 0, v, (np.float32(0.01) * v).astype(np.float32)).astype(np.float32)
    if res is not None:
        v = (v + res).astype(np.float32)
    return v


def reference_f32(case, inp, fin=None, w=None, rows=None):
    """chain oracle + numpy epilogue: what pcc_conv_fwd must give value for value (rows: the first `rows` output rows only)"""
    from oracle import chain
    n = case.n_out if rows is None else rows
    fin = inp.fin if fin is None else fin
    w = inp.w if w is None else w
    c = chain.conv_chain(fin if inp.nbr is not None else fin[:n], w, None if inp.nbr is None else inp.nbr[:n], n, mfma_order=True)
    return epilogue_f32(c, inp.bias, None if inp.film is None else inp.film[:n], None if inp.res is None else inp.res[:n],
                        act_code(case.epi))


U32 = 2.0 ** -24         # unit roundoff of float32


def ref64_rows(case, inp, rows, with_bound=True):
    """float64 value and error bound of output rows `rows`: (ref [len(rows), cout], bound); with_bound=False leaves the sums
    of magnitudes out (bound: None) for the modes that are held to a bound of their own.

    A float32 evaluation of c = bias + sum of L products by fused multiply-adds, in ANY order, makes L + 1 roundings, so
    |c32 - c| <= gamma_{L+1} * S <= (L + 2) * 2^-24 * S with S = sum |x * w| + |bias| (L + 1 <= 6,913 here).  Each later
    operation of the epilogue maps an input error e to |factor| * e (factor: beta for the FiLM product, at most 1 for the
    additions and both activations) and adds one rounding, 2^-24 * |its float64 result| plus the same share of the error
    carried in.  L is the row's number of contracted terms, the sums are taken in float64."""
    rows = np.asarray(rows, dtype=np.int64)
    cout = case.cout
    c = np.zeros((rows.shape[0], cout))
    s = np.zeros((rows.shape[0], cout))
    terms = np.zeros(rows.shape[0])
    w64 = inp.w.astype(np.float64)
    if inp.nbr is None:
        x = inp.fin[rows].astype(np.float64)
        c, terms = x @ w64[0], terms + case.cin
        if with_bound:
            s = np.abs(x) @ np.abs(w64[0])
    else:
        for k in range(inp.nbr.shape[1]):
            idx = inp.nbr[rows, k]
            sel = np.nonzero(idx >= 0)[0]
            if sel.size:
                x = inp.fin[idx[sel]].astype(np.float64)
                c[sel] += x @ w64[k]
                if with_bound:
                    s[sel] += np.abs(x) @ np.abs(w64[k])
                terms[sel] += case.cin
    b = inp.bias.astype(np.float64)[None, :]
    v = c + b
    e = (terms + 2)[:, None] * U32 * (s + np.abs(b))

    def rounded(value, err):                  # one more float32 rounding of a result known to `err`
        return err + U32 * (np.abs(value) + err)

    if inp.film is not None:
        f = inp.film[rows].astype(np.float64)
        v, e = v * f[:, :cout], e * np.abs(f[:, :cout])
        e = rounded(v, e)
        v = v + f[:, cout:]
        e = rounded(v, e)
    act = act_code(case.epi)
    if act == 1:
        v = np.maximum(v, 0.0)
    elif act == 2:
        v = np.where(v > 0, v, float(np.float32(0.01)) * v)       # the kernel's constant is 0.01f
        e = rounded(v, e)
    if inp.res is not None:
        v = v + inp.res[rows].astype(np.float64)
        e = rounded(v, e)
    return v, (e if with_bound else None)


def sample_rows(case, inp, count=3000):
    rng = np.random.default_rng([case.n_out, case.cin, 5])
    rows = rng.integers(0, case.n_out, size=min(count, case.n_out))
    if case.cout > 4096:                                          # (the very wide tiny launches: every row anyway)
        rows = np.arange(case.n_out)
    if inp.map is not None:
        rows = np.concatenate([rows, inp.map.corners])
    return np.unique(rows)


# ---- the launches ----------------------------------------------------------------------------------------------------
SENTINEL = -12345.0
FRONT, BACK = 64, 4096       # guard floats in front of row 0 (256 bytes: the output stays 16-byte aligned) and after the last row
FORMS = ("null", "natural_masks", "permutation", "library")


def describe_mismatch(case, form, got, want, order):
    """which rows differ, where they sit in the execution order and in their tile"""
    bad = np.nonzero((got != want).any(axis=1))[0]
    pos = bad if order is None else np.argsort(order, kind="stable")[bad]
    bm = tile_rows(case.kernel)
    cols = np.nonzero((got != want).any(axis=0))[0]
    with np.errstate(invalid="ignore"):
        worst = float(np.nanmax(np.abs(got.astype(np.float64) - want)))
    return (f"{case.id}: {case.kernel}, order form '{form}': {bad.size} of {case.n_out} rows differ (first rows {bad[:6].tolist()}, "
            f"execution positions {np.sort(pos)[:6].tolist()} .. {int(pos.max())}, positions in their {bm}-row tile "
            f"{sorted(set((pos % bm).tolist()))[:12]}), columns {int(cols.min())} .. {int(cols.max())} ({cols.size} of {case.cout}), "
            f"max |diff| {worst:.3g}")


class Launcher:
    """one case on the device: operands uploaded once, then any number of launches under the row-order forms"""

    def __init__(self, pcc, case, inp, dev="cuda:0"):
        import torch
        from pcc_amd import _lib
        self.torch, self._lib, self.L, self.case, self.inp, self.dev = torch, _lib, pcc.lib(), case, inp, dev
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        K = case.K if case.K else 1
        L, ptr, check = self.L, _lib.ptr, _lib.check
        self.x32 = t(inp.fin)
        self.x = self.x32.to(torch.bfloat16) if case.mode == MODE_BF16 else self.x32
        self.w = t(inp.w)
        self.bias, self.nbr, self.film, self.res = t(inp.bias), t(inp.nbr), t(inp.film), t(inp.res)
        self.wp = {}
        for mode in {case.mode, MODE_F32} if case.mode == MODE_X3 else {case.mode}:
            if mode == MODE_F32:
                wp = torch.empty(L.pcc_conv_packed_elems(K, case.cin, case.cout), dtype=torch.float32, device=dev)
                check(L.pcc_conv_pack_weights(ptr(self.w), K, case.cin, case.cout, ptr(wp), _lib.stream()))
            elif mode == MODE_BF16:
                wp = torch.empty(L.pcc_conv_packed_elems_bf16(K, case.cin, case.cout), dtype=torch.bfloat16, device=dev)
                check(L.pcc_conv_pack_weights_bf16(ptr(self.w), K, case.cin, case.cout, ptr(wp), _lib.stream()))
            else:
                wp = torch.empty(L.pcc_conv_packed_elems_x3(K, case.cin, case.cout), dtype=torch.bfloat16, device=dev)
                check(L.pcc_conv_pack_weights_x3(ptr(self.w), K, case.cin, case.cout, ptr(wp), _lib.stream()))
            self.wp[mode] = wp
        self._orders = {}

    def order_form(self, form):
        """(order, group masks) on the device and the order on the host (None = natural)"""
        if form in self._orders:
            return self._orders[form]
        torch, case = self.torch, self.case
        if form == "null" or self.inp.nbr is None:
            val = (None, None, None)
        else:
            rm = row_masks(self.inp.nbr)
            if form == "natural_masks":
                val = (None, torch.from_numpy(group_masks(rm).view(np.int32)).to(self.dev), None)
            elif form == "permutation":
                order = planted_permutation(case.n_out, self.inp.map.planted)
                val = (torch.from_numpy(order).to(self.dev), torch.from_numpy(group_masks(rm, order).view(np.int32)).to(self.dev), order)
            else:
                # the library sorts rows without a neighbour last, so under this form the ragged last tile holds only such rows;
                # ragged tiles WITH data are the other three forms' (build_map keeps the natural tail populated)
                L, ptr = self.L, self._lib.ptr
                d_rm = torch.from_numpy(rm.view(np.int32)).to(self.dev)
                order = torch.empty(case.n_out, dtype=torch.int32, device=self.dev)
                gm = torch.empty((case.n_out + 31) // 32, dtype=torch.int32, device=self.dev)
                nbytes = L.pcc_order_scratch_bytes(case.n_out)
                scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
                self._lib.check(L.pcc_order_rows_by_mask(ptr(d_rm), None, case.n_out, -1, 1, ptr(order), ptr(gm), ptr(scratch), nbytes,
                                                         self._lib.stream()))
                host = order.cpu().numpy()
                assert np.array_equal(np.sort(host), np.arange(case.n_out)), "pcc_order_rows_by_mask: not a permutation"
                assert np.array_equal(gm.cpu().numpy().view(np.uint32), group_masks(rm, host)), "pcc_order_rows_by_mask: group masks"
                val = (order, gm, host)
        self._orders[form] = val
        return val

    def launch(self, form="null", mode=None, rows=None):
        """one launch into a guarded buffer pre-filled with the sentinel -> output [rows, cout] on the device"""
        torch, case, L, ptr = self.torch, self.case, self.L, self._lib.ptr
        mode = case.mode if mode is None else mode
        n_out = case.n_out if rows is None else rows
        n_in = case.n_in if case.K else n_out
        K = case.K if case.K else 1
        order, gmask, _ = self.order_form(form) if rows is None else (None, None, None)
        whole = torch.full((FRONT + n_out * case.cout + BACK,), SENTINEL, dtype=torch.float32, device=self.dev)
        out = whole[FRONT:FRONT + n_out * case.cout].view(n_out, case.cout)
        assert out.data_ptr() % 16 == 0 and out.data_ptr() != whole.data_ptr()
        x = self.x32 if mode == MODE_F32 else self.x
        common = (ptr(self.bias), ptr(self.nbr), ptr(order), ptr(gmask), K, ptr(out), n_out, case.cout, act_code(case.epi), ptr(self.film),
                  ptr(self.res), self._lib.stream())
        if mode == MODE_F32:
            rc = L.pcc_conv_fwd(ptr(x), n_in, case.cin, ptr(self.w), ptr(self.wp[mode]), *common)
        elif mode == MODE_BF16:
            rc = L.pcc_conv_fwd_bf16(ptr(x), n_in, case.cin, ptr(self.wp[mode]), *common)
        else:
            rc = L.pcc_conv_fwd_x3(ptr(x), n_in, case.cin, ptr(self.wp[mode]), *common)
        self._lib.check(rc)
        torch.cuda.synchronize()
        assert bool((whole[:FRONT] == SENTINEL).all()), f"{case.id}: {case.kernel} wrote in front of row 0 (form '{form}')"
        assert bool((whole[FRONT + n_out * case.cout:] == SENTINEL).all()), f"{case.id}: {case.kernel} wrote past the last row (form '{form}')"
        return out


def run_case(pcc, case, forms=FORMS, with_float64=True, with_sub_rows=True):
    """every check of one table row; raises AssertionError naming the case, the kernel and where the values differ"""
    import torch
    L = pcc.lib()
    inp = make_inputs(case)
    with small_threshold(L, case.small), torch.no_grad():
        got_name = case_name(L, case)
        assert got_name == case.kernel, f"{case.id}: the plan runs {got_name}, the table says {case.kernel}"
        run = Launcher(pcc, case, inp)
        if case.mode == MODE_F32:
            want = reference_f32(case, inp)
        elif case.mode == MODE_BF16:
            want = reference_f32(case, inp, fin=bf16_round(inp.fin), w=bf16_round(inp.w))
        else:
            want = None
        d_want = None if want is None else torch.from_numpy(want).to(run.dev)
        base = run.launch("null")
        assert torch.equal(base, run.launch("null")), f"{case.id}: {case.kernel}: two launches differ"
        if case.mode == MODE_F32:
            assert torch.equal(base, d_want), describe_mismatch(case, "null", base.cpu().numpy(), want, None)
        elif case.mode == MODE_BF16:
            # tests/test_bf16_conv.py: rtol 1e-4, atol 2e-5 * max |want|
            assert torch.allclose(base, d_want, rtol=1e-4, atol=2e-5 * float(np.abs(want).max())), \
                (case.id, case.kernel, float((base - d_want).abs().max()))
        # every row-order form the header allows: the same values
        for form in forms[1:] if inp.nbr is not None else ():
            out = run.launch(form)
            if not torch.equal(out, base):
                raise AssertionError(describe_mismatch(case, form, out.cpu().numpy(), base.cpu().numpy(), run.order_form(form)[2]))
        stats = {}
        if with_float64 and case.mode == MODE_F32:
            rows = sample_rows(case, inp)
            ref, bound = ref64_rows(case, inp, rows)
            got = base[torch.from_numpy(rows).to(run.dev)].cpu().numpy().astype(np.float64)
            err = np.abs(got - ref)
            stats["e32"] = float(err.max()) / float(np.abs(ref).max())
            stats["bound_used"] = float((err / np.maximum(bound, 1e-300)).max())
            worst = np.unravel_index(np.argmax(err - bound), err.shape)
            assert (err <= bound).all(), (f"{case.id}: {case.kernel}: row {int(rows[worst[0]])} column {int(worst[1])} is "
                                          f"{err[worst]:.3g} from float64, bound {bound[worst]:.3g}")
        elif with_float64 and case.mode == MODE_X3:
            # no other reference holds an x3 launch, so float64 is evaluated on EVERY row.  tests/test_x3_conv.py: relative to
            # the maximum, e3 < 4e-6 and e3 < 4 * e32 + 1e-6 (e32: the fp32 kernel's error on the same input)
            ref, _ = ref64_rows(case, inp, np.arange(case.n_out), with_bound=False)
            scale = float(np.abs(ref).max())
            err3 = np.abs(base.cpu().numpy().astype(np.float64) - ref)
            e32 = float(np.abs(run.launch("null", mode=MODE_F32).cpu().numpy().astype(np.float64) - ref).max()) / scale
            e3 = float(err3.max()) / scale
            stats["e3"], stats["e32"] = e3, e32
            worst = np.unravel_index(np.argmax(err3), err3.shape)
            assert e3 < 4e-6 and e3 < 4 * e32 + 1e-6, (f"{case.id}: {case.kernel}: e3 {e3:.3g}, e32 {e32:.3g}; worst at row {int(worst[0])} "
                                                        f"(position {int(worst[0]) % tile_rows(case.kernel)} of its {tile_rows(case.kernel)}-row "
                                                        f"tile) column {int(worst[1])}")
        # tile invariance: the first rows on their own are planned onto another kernel and give the same values
        if with_sub_rows and case.sub_rows:
            other = case_name(L, case, case.sub_rows)
            assert other != case.kernel and not isinstance(other, int), (case.id, other)
            sub = run.launch(rows=case.sub_rows)
            if not torch.equal(sub, base[:case.sub_rows]):
                raise AssertionError(f"{other} on the first {case.sub_rows} rows differs from: " + describe_mismatch(
                    case, "null", base[:case.sub_rows].cpu().numpy(), sub.cpu().numpy(), None))
    return stats
