"""Every forward convolution kernel and tile `plan_conv` (csrc/conv.hip) can pick, per launch, against a reference of the
same operation: the small-launch kernel, the five MFMA tiles at one to eight channel chunks, with a map and without, their
64-bit-addressed twins, and the bf16 / split-bf16 ("x3") modes on the tiles they plan.

The case table (tests/_conv_plan_cases.py) names the kernel each row expects; every GPU case first asserts that the
planner returns that name, and a CPU test sweeps `pcc_conv_kernel_name` over a grid of shapes and fails when the planner
can emit a name no row reaches.  Inputs are synthetic (seeded numpy): ~25 % neighbour density with planted corners — rows
and whole 32-position groups without a neighbour (the first, a middle one, the last full one; the ragged tail keeps its
data), rows whose only neighbour is the first / last offset, an offset present in a single row, repeated input rows, n_in of
1 / far below / above n_out — run under every row-order form the header allows (no order, natural groups' masks, a random
permutation with its masks, the library's own order), into an output buffer with guard bands, twice.

Checks and where their numbers come from
  fp32       np.array_equal with oracle/chain.c + the epilogue in numpy float32                      (an equality)
  fp32       float64 on sampled rows incl. the planted ones, bound (L + 2) 2^-24 (sum |x w| + |b|) pushed through the
             epilogue's roundings (_conv_plan_cases.ref64_rows)                                      (derived)
  x3         float64 on every row, e3 < 4e-6 and e3 < 4 e32 + 1e-6 relative to the maximum           (tests/test_x3_conv.py)
  bf16       fp32 reference on bf16-rounded operands, rtol 1e-4, atol 2e-5 max |want|                (tests/test_bf16_conv.py)
  all modes  order forms agree bit for bit; the first 5,000 rows launched alone take another kernel and agree bit for bit

Measured on an MI355X box (16 host cores): the GPU tests of this module 28.6 s of wall time (226 tests: 223 table cases, two
shells, the child process), of which 17.7 CPU-seconds in the chain oracle; the child process 4.6 s.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _conv_plan_cases as cp
from _conv_plan_cases import CASES, GLOBAL_CASES, MODE_BF16, MODE_F32, MODE_X3

DEV = "cuda:0"

# Measured wall time of the child process of test_64bit_addressed_kernel_on_every_tile; its timeout is three times that,
# because load on a shared box varies.
CHILD_WALL_S = 4.6
CHILD_TIMEOUT_S = math.ceil(3 * CHILD_WALL_S)


# ---- the table itself (host only) ------------------------------------------------------------------------------------
def test_row_counts_sit_on_the_plan_boundaries():
    assert (cp.last_rows_64x64(256), cp.last_rows_32x128(256)) == (24512, 95936)
    assert (cp.last_rows_64x64(128), cp.last_rows_32x128(128)) == (49088, 191936)
    assert [cp.last_rows_small(c) for c in (128, 256, 64, 32, 96)] == [5120, 2560, 20480, 40960, 13632]
    rows = {(c.cout, c.n_out) for c in CASES if c.mode == MODE_F32}
    for cout, n in ((256, 24512), (256, 95936), (128, 49088), (128, 191936), (128, 5120), (256, 2560), (64, 20480), (32, 40960), (96, 13632)):
        assert (cout, n) in rows and (cout, n + 1) in rows, (cout, n)


def test_case_table_names_what_the_planner_picks(pcc):
    """every row's kernel string is the planner's answer for that row (so a wrong table fails here, without a GPU), ids are
    unique, big launches are ragged in their tile, and the first `sub_rows` rows are planned onto another kernel"""
    L = pcc.lib()
    assert len({c.id for c in CASES}) == len(CASES)
    for c in CASES:
        with cp.small_threshold(L, c.small):
            assert cp.case_name(L, c) == c.kernel, c.id
            if c.sub_rows:
                other = cp.case_name(L, c, c.sub_rows)
                assert isinstance(other, str) and other != c.kernel, c.id
    on_boundary = set()                     # the row counts that sit on a plan boundary by construction, and the row after
    for cout in {c.cout for c in CASES}:
        for last in (cp.last_rows_small(cout), cp.last_rows_64x64(max(cout, 128)), cp.last_rows_32x128(max(cout, 128))):
            on_boundary |= {last, last + 1}
    sweep = [c for c in CASES if c.n_out > 6000 and c.n_out not in on_boundary]
    assert len(sweep) > 100 and all(c.n_out % cp.tile_rows(c.kernel) != 0 for c in sweep)
    for tile in cp.FP32_TILES:
        mine = [c for c in CASES if c.mode == MODE_F32 and c.kernel.startswith("conv_mfma_buf_kernel<%d, %d," % tile)]
        assert {c.cin for c in mine if c.K} == set(range(32, 257, 32)) and {c.cin for c in mine if not c.K} >= {64, 96}
        assert {c.epi for c in mine} == set(cp.EPILOGUES)
        assert {c.n_out for c in mine if c.n_out <= tile[0] + 1} == {1, tile[0] - 1, tile[0], tile[0] + 1}
    assert {c.cout for c in CASES if c.mode == MODE_F32} >= {100, 33, 5, 31, 160, 192}
    assert {c.n_in for c in CASES if c.K} >= {1, 97} and any(c.n_in > c.n_out for c in CASES) and any(1 < c.n_in < c.n_out for c in CASES)
    assert len(GLOBAL_CASES) == 20 and all(c.kernel.startswith("conv_mfma_kernel<") and c.epi == "bias" for c in GLOBAL_CASES)


def _planner_sweep(L):
    """every kernel name the planner emits on a grid of shapes: cin 32 .. 256, the output widths of the model and ragged
    ones, row counts on both sides of every threshold, map / no map, three modes, small threshold off and default"""
    couts = (32, 64, 96, 128, 160, 192, 256, 5, 31, 33, 100, 250)
    rows = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 1_300_000, 5_160_000}
    for cout in couts:
        for last in (cp.last_rows_small4(cout), cp.last_rows_small(cout), cp.last_rows_64x64(max(cout, 128)), cp.last_rows_32x128(max(cout, 128))):
            rows |= {last, last + 1}
    names = set()
    for small in (0, cp.SMALL_MAX):
        with cp.small_threshold(L, small):
            for mode in (MODE_F32, MODE_BF16, MODE_X3):
                for cin in range(32, 257, 32):
                    for cout in couts:
                        for n_out in rows:
                            for K in (27, 0):
                                name = cp.planner_name(L, mode, n_out, cin, cout, n_out, K)
                                if isinstance(name, str):                  # (an error code: the mode does not run the shape)
                                    names.add(name)
    return names


def test_table_reaches_every_kernel_the_planner_can_emit(pcc):
    """fails, naming the kernels, when plan_conv can emit a name no table row launches — until the table follows a changed
    plan.  conv_thin_kernel is not in the grid (cin % 32 == 0): CONV_SHAPES and test_thin_im2col... cover that family."""
    emitted = _planner_sweep(pcc.lib())
    assert emitted, "the sweep found no kernel name"
    reached = {c.kernel for c in CASES} | {c.kernel for c in GLOBAL_CASES}
    assert not emitted - reached, sorted(emitted - reached)
    # and the 64-bit-addressed twin of every fp32 tile launch (one name per tile and map form: it has no chunk parameter)
    twins = {cp.global_twin(n) for n in emitted} - {None}
    assert len(twins) == 2 * len(cp.FP32_TILES) and not twins - {c.kernel for c in GLOBAL_CASES}, sorted(twins - {c.kernel for c in GLOBAL_CASES})


@pytest.mark.parametrize("K", [1, 8, 27])
def test_backward_data_pads_dy_to_the_widths_the_thin_plan_takes(pcc, K):
    """The training path's backward-data convolution reads dY [n_out, cout] as its input and zero-pads a narrow one to the
    first width the fp32 plan takes (autograd._taken_width asks the planner).  That used to be a hand copy of thin_cin()
    (csrc/conv.hip), the tuple below: wherever the plan takes the tuple's width — every shape that ran — the planner's answer
    is that width; where it does not (no width of the tuple fits, or the thin kernel's weights would pass its 160 KB of LDS:
    the launch was an error), it is the next multiple of 32, the MFMA kernel."""
    from pcc_amd import autograd, sparse as sp
    old_tuple = (1, 2, 3, 4, 6, 8, 12, 16, 24)
    cin, n = 64, 9500
    ran = []
    for cout in range(1, 32):
        old = next((c for c in old_tuple if c >= cout), None)
        got = autograd._taken_width(n, cout, cin, n, K, K > 1)
        if old is not None and sp._plan_takes(sp.MODE_F32, n, old, cin, n, K, K > 1):
            ran.append(cout)
            assert got == old, (cout, got, old)
        else:
            assert got == 32, (cout, got)
    # 27 x 24 x 64 floats are 162 KB: with 27 offsets the widest thin width that ran is 16
    assert ran == list(range(1, 17 if K == 27 else 25))
    assert [autograd._taken_width(n, c, cin, n, K, K > 1) for c in (32, 64, 128, 256)] == [32, 64, 128, 256]


@pytest.mark.parametrize("n_out,n_in,K", [(50003, 25008, 27), (6001, 1, 27), (96007, 97008, 27), (33, 36, 3), (1, 5, 27)])
def test_synthetic_map_has_the_planted_corners(n_out, n_in, K):
    m = cp.build_map(n_out, n_in, K)
    nbr = m.nbr
    assert nbr.shape == (n_out, K) and nbr.min() >= -1 and nbr.max() < n_in
    rm = cp.row_masks(nbr)
    assert all(int(rm[j]) == sum(1 << k for k in range(K) if nbr[j, k] >= 0) for j in list(m.corners) + [0, n_out - 1])
    if n_out < 256:
        return
    assert 0.2 < float((nbr >= 0).mean()) < 0.3
    groups = (n_out + 31) // 32
    for order in (None, cp.planted_permutation(n_out, m.planted)):
        gm = cp.group_masks(rm, order)
        mid = groups // 2 if order is None else 1 + (n_out // 32 - 3) // 2
        last = n_out // 32 - 1                                                                   # the last full group
        assert gm.shape[0] == groups and gm[0] == 0 and gm[mid] == 0 and gm[last] == 0            # whole groups without a neighbour
        if n_out % 32:                                                                           # rows with neighbours in the ragged tail
            tail = np.arange(32 * (groups - 1), n_out) if order is None else order[32 * (groups - 1):]
            assert gm[-1] != 0 and (rm[tail] != 0).sum() * 2 > tail.shape[0]
        if order is not None:
            assert np.array_equal(np.sort(order), np.arange(n_out)) and not np.array_equal(order, np.arange(n_out))
            assert all(int(gm[g]) == int(np.bitwise_or.reduce(rm[order[32 * g:32 * g + 32]])) for g in (1, groups // 3, groups - 2))
    assert int((rm == 0).sum()) >= 32 + 32 + 1 + 3
    assert int((rm == 1).sum()) >= 3 and int((rm == np.uint32(1 << (K - 1))).sum()) >= 3     # only the first / only the last offset
    row, k = m.lone
    assert int((nbr[:, k] >= 0).sum()) == 1 and nbr[row, k] >= 0                               # an offset one row has
    others = np.arange(K) != k
    assert any((nbr[j, others] == nbr[j, 0]).all() and nbr[j, 0] >= 0 for j in m.corners)      # one input row under every other offset
    if n_in > 1:
        flat = nbr[nbr >= 0]
        assert np.unique(flat).shape[0] < flat.shape[0]                                         # repeated input rows


@pytest.mark.parametrize("pick", ["f32-128x128-n50003-in25008-K27-small640-bias-t32x128c4m",
                                  "f32-96x128-n6001-in3007-K27-small640-lrelu_film_res-t64x64c3m"])
def test_chain_oracle_is_within_the_float64_bound(pick):
    """the reference itself, on this machine: chain oracle + numpy epilogue against the float64 evaluation and its bound"""
    case = {c.id: c for c in CASES}[pick]
    inp = cp.make_inputs(case)
    want = cp.reference_f32(case, inp)
    rows = cp.sample_rows(case, inp)
    assert set(inp.map.corners.tolist()) <= set(rows.tolist()) and rows.shape[0] > 2000
    ref, bound = cp.ref64_rows(case, inp, rows)
    err = np.abs(want[rows].astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / bound).max())
    assert float(err.max()) < 1e-5 * float(np.abs(ref).max())
    # the bound is not vacuous: a dropped term is outside it: the same rows without their last present offset
    nbr2 = inp.nbr.copy()
    j = int(rows[np.argmax((inp.nbr[rows] >= 0).sum(axis=1))])
    nbr2[j, np.nonzero(nbr2[j] >= 0)[0][-1]] = -1
    bad = cp.reference_f32(case, inp._replace(nbr=nbr2))
    i = int(np.nonzero(rows == j)[0][0])
    assert (np.abs(bad[j].astype(np.float64) - ref[i]) > bound[i]).any()


# ---- on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_planned_kernel_matches_its_reference(pcc, case):
    stats = cp.run_case(pcc, case)
    print(case.id, case.kernel, {k: float("%.3g" % v) for k, v in stats.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("grid,radius,cin,cout,tile", [(128, 50.0, 96, 128, cp.T32x128), (160, 62.0, 64, 256, cp.T64x128)])
def test_library_map_and_order_on_a_shell(pcc, grid, radius, cin, cout, tile):
    """a real geometry through the Python layer (the library's own kernel map and mask order, 63 k and 98 k rows) on the two
    large tiles, against the chain oracle over oracle.coords.kernel_map"""
    import torch
    from oracle import chain
    from oracle import coords as oc
    L = pcc.lib()
    p = pcc.synthetic.sphere_shell(grid, radius, 1.0)[:, :3]
    c = np.concatenate([np.zeros((p.shape[0], 1)), p], axis=1).astype(np.int32)
    c = c[np.random.default_rng(grid).permutation(c.shape[0])]
    n = c.shape[0]
    rng = np.random.default_rng([grid, cin, cout])
    F = rng.standard_normal((n, cin), dtype=np.float32)
    W = (rng.standard_normal((27, cin, cout), dtype=np.float32) * np.float32(1.0 / np.sqrt(cin * 10.0))).astype(np.float32)
    b = (rng.standard_normal(cout, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    layer = pcc.MinkowskiConvolution(cin, cout, kernel_size=3, stride=1, bias=True, dimension=3)
    with torch.no_grad(), cp.small_threshold(L, cp.SMALL_MAX):
        assert cp.planner_name(L, MODE_F32, n, cin, cout, n, 27) == cp.tile_name(MODE_F32, tile, cin // 32, True), n
        layer.kernel.copy_(torch.from_numpy(W).reshape(layer.kernel.shape))
        layer.bias.copy_(torch.from_numpy(b).reshape(layer.bias.shape))
        layer = layer.to(DEV)
        x = pcc.SparseTensor(torch.from_numpy(F).to(DEV), coordinate_map=pcc.CoordMap(torch.from_numpy(c).to(DEV), 1))
        got = layer(x).F.cpu().numpy()
    nbr = oc.kernel_map(c, c, 3, 1)
    want = cp.epilogue_f32(chain.conv_chain(F, W, nbr, n, mfma_order=True), b, None, None, 0)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (cp.tile_name(MODE_F32, tile, cin // 32, True), bad.size, bad[:8].tolist(), float(np.abs(got - want).max()))


@pytest.mark.gpu
def test_64bit_addressed_kernel_on_every_tile(pcc):
    """conv_mfma_kernel (operands of 4 GiB and more; forced by PCC_CONV_PATH=global, which is read once per process) on all
    five tiles, an even and an odd chunk count, with a map and without, against the chain oracle — in one child process"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_conv_plan_child.py")
    try:
        r = subprocess.run([sys.executable, child], env=dict(os.environ, PCC_CONV_PATH="global"), capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"the child ran past {CHILD_TIMEOUT_S} s; its last lines:\n" + "\n".join(out.splitlines()[-10:]))
    tail = "\n".join((r.stdout + "\n" + r.stderr).splitlines()[-25:])
    print(tail)
    assert r.returncode == 0, tail
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("OK ")]
    assert len(ok) == len(GLOBAL_CASES) and any(ln.startswith(f"RAN {len(GLOBAL_CASES)} ") for ln in r.stdout.splitlines()), tail
    assert all(" conv_mfma_kernel<" in ln for ln in ok)

