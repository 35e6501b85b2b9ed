"""The layer backward of the sparse convolutions, held to EQUALITY with float64 references (tests/_conv_grad_cases.py).

The per-launch suites pin each kernel (test_conv_plans.py, test_wgrad_plans.py, test_coord_paths.py); this module pins the code
that joins them into a gradient: `SparseConvFn.backward` (autograd.py) — dY padded to the width backward-data takes, the padded
W^T, the bf16 copy shared by the weight gradient and backward-data, the pad unit of 64, the adjoint shape's own mode, db through
pcc_cast_colsum or the fallback sum, `out_channels` slicing, `needs_input_grad` combinations, kernel size 1 —,
`CoordMap.transposed_ordered_map` / `conv_map(adjoint=True)` (sparse.py) and `pcc_kernel_map_transpose` (csrc/conv_bwd.hip).

  1. pcc_kernel_map_transpose against a numpy transposition, into guarded buffers, on the oracle's maps and on sizes around the
     one-thread-per-entry grid; the composition in transposed_ordered_map (order, group masks).
  2. the public layers (MinkowskiConvolution stride 1 / 2, kernel 1 / 3; MinkowskiGenerativeConvolutionTranspose kernel 2 / 3)
     forward + backward on real coordinate sets, per map kind, mode (fp32, set_bf16, set_x3) and geometry; product rows are
     matched to oracle rows by coordinate lookup.  Operands lie on grids for which every sum is exact in any order, so out, dX,
     dW, db are compared with np.array_equal; bf16 launches are expected to compute the float64 value of bf16-rounded operands,
     for exactly the launches the documented rule sends to bf16 — which also proves that the mode ran.
  3. host-only: the references equal torch float64 autograd through the oracle, the exactness assertion rejects an oversized
     case, the restated launch rule agrees with the library, and the table reaches every kernel family forward, adjoint and in
     the weight gradient.

Measured on an MI355X box (16 host cores): the module 15.3 s of wall time (241 tests: 43 host-only, 44 transposition cases, 63
integer and 18 wide-mantissa layer tests of 4 to 15 layer shapes each, 18 variant and epilogue tests; the slowest, the generative
kernel-3 layer over the 9 k-row shell, 1.2 s) — tests/test_train_ops.py takes 4.7 s there.  Ignoring the bf16 switch, running only
the adjoint in fp32, or W instead of W^T on square layers each fail it; the first two pass every integer case and fail on the wide
mantissas.
"""
import ctypes

import numpy as np
import pytest
import torch

import _conv_grad_cases as gc
from _conv_grad_cases import MODE_BF16, MODE_F32, MODE_X3
from oracle import coords as oc
from oracle import nn as on

DEV = "cuda:0"
SENTINEL = 12345
GUARD = 64


# ---- helpers -----------------------------------------------------------------------------------------------------------------
class arithmetic:
    """the training path's mode switches for the length of a block"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from pcc_amd import autograd
        self.was = (autograd.BF16, autograd.X3)
        autograd.set_bf16(self.mode == "bf16")
        autograd.set_x3(self.mode == "x3")

    def __exit__(self, *exc):
        from pcc_amd import autograd
        autograd.set_bf16(self.was[0])
        autograd.set_x3(self.was[1])


def wgrad_name(L, bf16, K, cin, cout, n_out):
    buf = ctypes.create_string_buffer(96)
    rc = L.pcc_conv_wgrad_kernel_name(int(bf16), K, cin, cout, n_out, buf, len(buf), None, None)
    assert rc == 0, (bf16, K, cin, cout, n_out, rc)
    return buf.value.decode()


def library_launches(mode, s, cin, cout):
    """(forward mode, adjoint mode, dY width) with the arguments autograd.py passes, under the switches of `mode`"""
    from pcc_amd import autograd
    n_in, n_out, K, has_nbr = s.coords.shape[0], s.out.shape[0], s.ksize ** 3, s.ksize > 1
    with arithmetic(mode):
        fwd = autograd._mode(n_in, cin, cout, n_out, K, has_nbr)
        width = autograd._taken_width(n_out, cout, cin, n_in, K, has_nbr)
        adj = autograd._mode(n_out, width, cin, n_in, K, has_nbr)
    return fwd, adj, width


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ---- 3. host-only: the references and the table ---------------------------------------------------------------------------------
SELF_CHECK_SHAPES = ((4, 8), (32, 3), (2, 2))


@pytest.mark.parametrize("size", gc.TINY)
@pytest.mark.parametrize("kind", gc.KINDS)
def test_references_equal_float64_autograd_through_the_oracle(kind, size):
    """out, dX, dW, db of the numpy references = torch autograd in float64 through oracle.nn._apply_conv, on every family"""
    s = gc.sets_of(kind, size)
    nbr = gc.table_of(s)
    n_in, n_out = s.coords.shape[0], s.out.shape[0]
    for cin, cout in SELF_CHECK_SHAPES:
        for family in gc.FAMILIES:
            ops = gc.operands(s, cin, cout, family)
            gc.assert_exact(s, ops)
            want = gc.expected(s, ops, "f32", cin, cout)
            X, W, b = (t64(a).requires_grad_(True) for a in (ops.X, ops.W, ops.b))
            out = on._apply_conv(X, W, b, nbr, n_out)
            assert out.dtype == torch.float64
            out.backward(t64(ops.dY))
            for name, got in (("out", out.detach()), ("dX", X.grad), ("dW", W.grad), ("db", b.grad)):
                assert np.array_equal(got.numpy(), want[name]), gc.describe_mismatch((kind, size, cin, cout, family), name, got.numpy(), want[name])


@pytest.mark.parametrize("size", gc.TINY)
@pytest.mark.parametrize("kind", ["same3", "k1", "down", "up2", "up3", "batch"])
def test_references_equal_the_oracle_layers(kind, size):
    """the same through the oracle's own layers (oracle.nn.conv, conv_transpose_generative), which build their coordinate sets
    and maps themselves and compute in float32 — exact here, by the asserted condition"""
    s = gc.sets_of(kind, size)
    for cin, cout in SELF_CHECK_SHAPES:
        for family in gc.FAMILIES:
            ops = gc.operands(s, cin, cout, family)
            gc.assert_exact(s, ops)
            want = gc.expected(s, ops, "f32", cin, cout)
            X, W, b = (torch.from_numpy(a.copy()).requires_grad_(True) for a in (ops.X, ops.W if s.ksize > 1 else ops.W[0], ops.b))
            x = on.SparseTensor(s.coords, X, s.stride)
            y = on.conv_transpose_generative(x, W, b, s.ksize) if s.layer == "up" else on.conv(x, W, b, s.ksize, s.lstride)
            assert np.array_equal(y.C, s.out)
            y.F.backward(torch.from_numpy(ops.dY))
            for name, got in (("out", y.F.detach()), ("dX", X.grad), ("dW", W.grad.reshape(ops.W.shape)), ("db", b.grad)):
                assert np.array_equal(got.numpy().astype(np.float64), want[name]), (kind, size, cin, cout, family, name)


def test_bf16_rounding_is_torchs_and_keeps_the_grid():
    rng = np.random.default_rng(3)
    a = np.concatenate([(rng.integers(-2047, 2048, size=4096) / 256.0), [0.0, 1.00390625, 1.01171875, -7.99609375, 3.0]]).astype(np.float32)
    r = gc.bf16_round(a)
    assert np.array_equal(r, torch.from_numpy(a).to(torch.bfloat16).float().numpy())
    assert np.array_equal(r * 256, np.round(r * 256)) and float(np.abs(r).max()) <= 8.0 and (r != a).any()
    assert r[-4] == 1.0 and r[-3] == 1.015625                  # halfway cases go to the even neighbour


def test_exactness_assertion_rejects_an_oversized_case():
    """db of a generative layer over the 9 k-row shell sums 110 k rows of up to 2,047 grid units: not a case of the table"""
    s = gc.sets_of("up3", "shell9k")
    with pytest.raises(AssertionError, match="db is not exact"):
        gc.assert_exact(s, gc.operands(s, 4, 4, "wideG"))
    with pytest.raises(AssertionError, match="out is not exact"):       # 18 neighbours x 1,024 channels x about 1.5 x 1,024 units
        gc.assert_exact(gc.sets_of("same3", "patch70"), gc.operands(gc.sets_of("same3", "patch70"), 1024, 2, "wideX"))
    gc.assert_exact(s, gc.operands(s, 128, 128, "int"))


# (mode, cin, cout, K) -> (forward, adjoint, dY width, bf16 weight gradient, padded cin, padded cout), written out by hand from the
# documented rule (the module docstring of _conv_grad_cases.py)
RULE = [
    ("f32", 128, 128, 27, (MODE_F32, MODE_F32, 128, False, 128, 128)),
    ("f32", 64, 100, 27, (MODE_F32, MODE_F32, 128, False, 64, 128)),
    ("f32", 2, 2, 27, (MODE_F32, MODE_F32, 2, False, 32, 32)),
    ("bf16", 128, 128, 27, (MODE_BF16, MODE_BF16, 128, True, 128, 128)),
    ("bf16", 128, 128, 1, (MODE_BF16, MODE_BF16, 128, True, 128, 128)),
    ("bf16", 192, 64, 8, (MODE_BF16, MODE_BF16, 64, True, 192, 64)),
    ("bf16", 96, 160, 27, (MODE_F32, MODE_F32, 160, False, 96, 160)),
    ("bf16", 64, 100, 27, (MODE_BF16, MODE_BF16, 128, True, 64, 128)),
    ("bf16", 64, 3, 27, (MODE_BF16, MODE_F32, 3, True, 64, 64)),
    ("bf16", 64, 4, 27, (MODE_BF16, MODE_F32, 4, True, 64, 64)),
    ("bf16", 128, 2, 27, (MODE_BF16, MODE_F32, 2, True, 128, 64)),
    ("bf16", 4, 64, 27, (MODE_F32, MODE_BF16, 64, False, 32, 64)),
    ("bf16", 2, 128, 27, (MODE_F32, MODE_BF16, 128, False, 32, 128)),
    ("bf16", 32, 3, 27, (MODE_F32, MODE_F32, 3, False, 32, 32)),
    ("x3", 128, 128, 27, (MODE_X3, MODE_X3, 128, False, 128, 128)),
    ("x3", 192, 64, 27, (MODE_X3, MODE_X3, 64, False, 192, 64)),
    ("x3", 96, 160, 27, (MODE_F32, MODE_F32, 160, False, 96, 160)),
    ("x3", 64, 100, 27, (MODE_X3, MODE_X3, 128, False, 64, 128)),
    ("x3", 64, 3, 27, (MODE_F32, MODE_F32, 3, False, 64, 32)),
    ("x3", 64, 4, 8, (MODE_F32, MODE_F32, 4, False, 64, 32)),
    ("x3", 4, 64, 27, (MODE_F32, MODE_F32, 64, False, 32, 64)),
    ("x3", 2, 128, 27, (MODE_F32, MODE_F32, 128, False, 32, 128)),
    ("x3", 32, 64, 27, (MODE_X3, MODE_F32, 64, False, 32, 64)),
    ("x3", 64, 128, 1, (MODE_X3, MODE_X3, 128, False, 64, 128)),
]
# (cout, cin, K) -> the width dY is padded to
WIDTHS = [(5, 64, 27, 6), (7, 64, 27, 8), (9, 64, 27, 12), (25, 64, 27, 32), (100, 64, 27, 128), (3, 192, 27, 3), (24, 256, 27, 32),
          (24, 64, 27, 32), (24, 32, 27, 24), (24, 64, 8, 24), (1, 64, 1, 1), (160, 96, 27, 160)]      # (27 x 24 x 64 floats: 162 KB of weights)


def test_restated_rule_agrees_with_the_documented_one(pcc):
    from pcc_amd import autograd
    for mode, cin, cout, K, want in RULE:
        ln = gc.launches(mode, cin, cout, K)
        assert (ln.fwd, ln.adj, ln.width, ln.wgrad_bf16, ln.cin_p, ln.cout_p) == want, (mode, cin, cout, K, ln)
        with arithmetic(mode):
            for rows in (1, 70, 1088, 9224, 110346):
                n_out = rows + 5 if K > 1 else rows               # (no map: every row reads itself)
                assert autograd._mode(rows, cin, cout, n_out, K, K > 1) == ln.fwd, (mode, cin, cout, K, rows)
                assert autograd._taken_width(n_out, cout, cin, rows, K, K > 1) == ln.width, (mode, cin, cout, K, rows)
                assert autograd._mode(n_out, ln.width, cin, rows, K, K > 1) == ln.adj, (mode, cin, cout, K, rows)
    for cout, cin, K, want in WIDTHS:
        assert gc.taken_width(cout, cin, K) == want == autograd._taken_width(1000, cout, cin, 1000, K, K > 1), (cout, cin, K)
    assert not autograd.BF16 and not autograd.X3


def test_table_reaches_every_kernel_family(pcc):
    """the kernels the table's forward, adjoint and weight-gradient launches take (the library's plan queries, with the arguments
    autograd.py passes): every family named below, adjoint launches counted on their own; the restated rule agrees with the
    library on every row; row counts on both sides of the one-launch small-map limit"""
    from pcc_amd import sparse as sp
    L = pcc.lib()
    small_map = int(L.pcc_small_map_max())
    fwd, adj, wgrad, map_rows, missing = set(), set(), set(), set(), []
    cases = list(gc.all_layer_cases())
    assert len(cases) == len(set(cases))
    for kind, size, mode, cin, cout, family in cases:
        s = gc.sets_of(kind, size)
        n_in, n_out, K, has_nbr = s.coords.shape[0], s.out.shape[0], s.ksize ** 3, s.ksize > 1
        ln = gc.launches(mode, cin, cout, K)
        assert library_launches(mode, s, cin, cout) == (ln.fwd, ln.adj, ln.width), (kind, size, mode, cin, cout)
        fwd.add(sp.conv_kernel_name(ln.fwd, n_in, cin, cout, n_out, K, has_nbr))
        adj.add(sp.conv_kernel_name(ln.adj, n_out, ln.width, cin, n_in, K, has_nbr))
        wgrad.add(wgrad_name(L, ln.wgrad_bf16, K, ln.cin_p, ln.cout_p, n_out))
        if has_nbr:
            map_rows.add(n_out)
    table = set(cases)
    for kind in gc.KINDS:                                     # every shape class for every map kind at the 1.1 k shell, in all three modes
        for mode in gc.MODES:
            for cin, cout in gc.SHAPES:
                assert (kind, "shell1k", mode, cin, cout, "int") in table
    for which, names in (("forward", fwd), ("adjoint", adj)):
        for family in ("conv_small_kernel<", "conv_mfma_buf_kernel<", "conv_mfma_buf_kernel[bf16]<", "conv_mfma_buf_kernel[x3]<", "conv_thin_kernel<"):
            if not any(n.startswith(family) for n in names):
                missing.append((which, family))
    for family in ("conv_wgrad_kernel", "conv_wgrad_slice_kernel<", "conv_wgrad_bf16_kernel", "conv_wgrad_bf16_slice_kernel<"):
        if not any(n == family or (family.endswith("<") and n.startswith(family)) for n in wgrad):
            missing.append(("wgrad", family))
    assert not missing, (missing, sorted(fwd), sorted(adj), sorted(wgrad))
    # db through pcc_cast_colsum and through the fallback sum; dY padded to a wider taken width; both pad units
    plans = {(cout, gc.launches(mode, cin, cout, 27)) for _, _, mode, cin, cout, _ in cases}
    assert {p.db_kernel for _, p in plans} == {True, False} and any(p.width > cout for cout, p in plans)
    assert any(p.wgrad_bf16 and p.cout_p > cout for cout, p in plans) and any(not p.wgrad_bf16 and p.cout_p > cout for cout, p in plans)
    assert small_map > 0 and any(1 < n <= small_map for n in map_rows) and any(n > small_map for n in map_rows), sorted(map_rows)


# ---- 1. pcc_kernel_map_transpose ----------------------------------------------------------------------------------------------
def guarded_transpose(pcc, nbr, n_in):
    """pcc_kernel_map_transpose into sentinel-filled outputs that lie inside larger sentinel buffers -> (nbr_t, mask_t); asserts
    that the guards in front and behind are untouched"""
    from pcc_amd import _lib
    L, ptr = pcc.lib(), _lib.ptr
    n_out, K = nbr.shape
    d_nbr = torch.from_numpy(np.ascontiguousarray(nbr, dtype=np.int32)).to(DEV)
    t_whole = torch.full((GUARD + n_in * K + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    m_whole = torch.full((GUARD + n_in + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = L.pcc_kernel_map_transpose(ptr(d_nbr), n_out, K, n_in, ptr(t_whole[GUARD:]), ptr(m_whole[GUARD:]), _lib.stream())
    assert rc == 0, (rc, L.pcc_last_error())
    t, m = t_whole.cpu().numpy(), m_whole.cpu().numpy()
    for name, whole, used in (("nbr_t", t, n_in * K), ("mask_t", m, n_in)):
        assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + used:] == SENTINEL).all(), f"{name}: a guard was written ({n_out} x {K} onto {n_in} rows)"
    return t[GUARD:GUARD + n_in * K].reshape(n_in, K), m[GUARD:GUARD + n_in].view(np.uint32)


def assert_transposed(pcc, nbr, n_in, who):
    want_t, want_m = gc.transpose_reference(nbr, n_in)
    got_t, got_m = guarded_transpose(pcc, nbr, n_in)
    assert np.array_equal(got_t, want_t), gc.describe_mismatch(who, "nbr_t", got_t, want_t)
    assert np.array_equal(got_m, want_m), gc.describe_mismatch(who, "mask_t", got_m, want_m)
    return want_t, want_m


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["one", "five", "patch70", "shell1k"])
@pytest.mark.parametrize("kind", ["same3", "down", "up2", "up3", "pruned"])
def test_map_transpose_of_the_oracles_maps(pcc, kind, size):
    s = gc.sets_of(kind, size)
    assert_transposed(pcc, s.nbr.astype(np.int32), s.coords.shape[0], (kind, size))


# (n_out, n_in, K, input rows nobody reads): around the grid of one thread per entry, 256 to a block
TRANSPOSE_SIZES = [(255, 255, 1, 0), (256, 256, 1, 0), (257, 257, 1, 0), (256, 300, 1, 44), (32, 32, 8, 0), (33, 33, 8, 0), (33, 40, 8, 7),
                   (9, 9, 27, 0), (10, 10, 27, 0), (10, 12, 27, 2), (1, 1, 1, 0), (1, 1, 8, 0), (1, 1, 27, 0), (300, 200, 27, 37), (200, 300, 27, 120)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_out,n_in,K,unread", TRANSPOSE_SIZES)
def test_map_transpose_around_the_block_size(pcc, n_out, n_in, K, unread):
    nbr = gc.injective_map(n_out, n_in, K, unread)
    assert (nbr >= 0).any() and int(nbr.max()) < n_in - unread
    want_t, want_m = assert_transposed(pcc, nbr, n_in, (n_out, n_in, K))
    if unread:                                               # rows that nobody reads stay -1 with mask 0
        assert (want_t[n_in - unread:] == -1).all() and (want_m[n_in - unread:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_out,n_in,K", [(0, 33, 27), (33, 0, 27), (0, 0, 8), (0, 257, 1)])
def test_map_transpose_of_empty_sets(pcc, n_out, n_in, K):
    """n_in = 0 or n_out = 0: OK, and nothing is written past the memsets (every input row -1 / 0, the guards untouched)"""
    nbr = np.full((n_out, K), -1, dtype=np.int32)
    got_t, got_m = guarded_transpose(pcc, nbr, n_in)
    assert (got_t == -1).all() and (got_m == 0).all()


def device_maps(pcc, s):
    """the input CoordMap, the output CoordMap as the layer would pick it, and the oracle row of every product output row"""
    in_map = pcc.CoordMap(torch.from_numpy(s.coords).to(DEV), s.stride)
    if s.own_out:
        out_map = pcc.CoordMap(torch.from_numpy(s.out).to(DEV), s.stride)
    elif s.layer == "up":
        out_map = in_map.up(s.ksize)
    else:
        out_map = in_map if s.lstride == 1 else in_map.down()
    idx = oc.lookup(s.out, out_map.coords.cpu().numpy())
    assert out_map.n == s.out.shape[0] and np.array_equal(np.sort(idx), np.arange(s.out.shape[0])), (s.kind, s.size, "the output set differs from the oracle's")
    return in_map, out_map, idx


def assert_transposed_ordered_map(s, got, idx, who):
    """(nbr_t, order, gmask) of CoordMap.transposed_ordered_map against numpy on the oracle's map; idx: oracle row of a product row"""
    n_in = s.coords.shape[0]
    want_t, want_m = gc.transpose_reference(s.nbr, n_in)
    nbr_t, order, gmask = (t.cpu().numpy() for t in got)
    assert nbr_t.shape == want_t.shape and int(nbr_t.max(initial=-1)) < s.out.shape[0] and int(nbr_t.min(initial=-1)) >= -1
    in_oracle_rows = np.where(nbr_t >= 0, idx[np.maximum(nbr_t, 0)], -1)
    assert np.array_equal(in_oracle_rows, want_t), gc.describe_mismatch(who, "nbr_t", in_oracle_rows, want_t)
    assert np.array_equal(np.sort(order), np.arange(n_in)), f"{who}: order is no permutation of the input rows"
    want_g = gc.group_or(want_m, order)
    assert np.array_equal(gmask.view(np.uint32), want_g), gc.describe_mismatch(who, "gmask", gmask.view(np.uint32), want_g)


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["five", "patch70", "shell1k"])
@pytest.mark.parametrize("kind", ["same3", "down", "up2", "up3", "pruned", "batch"])
def test_transposed_ordered_map_against_numpy(pcc, kind, size):
    s = gc.sets_of(kind, size)
    in_map, out_map, idx = device_maps(pcc, s)
    got = in_map.transposed_ordered_map(out_map, s.ksize, s.layer == "up")
    assert_transposed_ordered_map(s, got, idx, (kind, size))
    nbr_t, order, gmask, pairs = in_map.conv_map(out_map, s.ksize, s.layer == "up", 64, adjoint=True)
    assert nbr_t is got[0] and order is got[1] and gmask is got[2] and pairs is None
    thin = in_map.conv_map(out_map, s.ksize, s.layer == "up", 3, adjoint=True)                                   # thin dY: the plain table
    assert thin[0] is got[0] and thin[1:] == (None, None, None)
    assert in_map.conv_map(out_map, 1, False, 64, adjoint=True) == (None, None, None, None)


# ---- 2. the layers ------------------------------------------------------------------------------------------------------------
def make_layer(pcc, s, cin, cout, ops, w_grad=True):
    if s.layer == "up":
        layer = pcc.MinkowskiGenerativeConvolutionTranspose(cin, cout, kernel_size=s.ksize, stride=2, bias=ops.b is not None, dimension=3)
    else:
        layer = pcc.MinkowskiConvolution(cin, cout, kernel_size=s.ksize, stride=s.lstride, bias=ops.b is not None, dimension=3)
    layer = layer.to(DEV)
    with torch.no_grad():
        layer.kernel.copy_(torch.from_numpy(ops.W if s.ksize > 1 else ops.W[0]))
        if ops.b is not None:
            layer.bias.copy_(torch.from_numpy(ops.b).reshape(1, -1))
    for p in layer.parameters():
        p.requires_grad_(w_grad)
    return layer


def run_layer(pcc, s, maps, cin, cout, ops, x_grad=True, w_grad=True, out_channels=None, sum_backward=False, **epilogue):
    """forward + backward of the public layer -> {out, dX, dW, db} as numpy (None where no gradient was asked for); rows of
    `out` in the product's order, dY given in the oracle's"""
    in_map, out_map, idx = maps
    layer = make_layer(pcc, s, cin, cout, ops, w_grad)
    x = torch.from_numpy(ops.X).to(DEV).requires_grad_(x_grad)
    got = layer(pcc.SparseTensor(x, coordinate_map=in_map), out_map=out_map if s.own_out else None, out_channels=out_channels, **epilogue)
    assert got.map is out_map or torch.equal(got.C, out_map.coords)
    assert got.F.grad_fn is not None, "the layer did not take the training path"
    if sum_backward:
        got.F.sum().backward()                                # dY arrives as a stride-0 expansion of one element
    else:
        got.F.backward(torch.from_numpy(ops.dY[idx]).to(DEV))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    dW = host(layer.kernel.grad)
    return {"out": host(got.F), "dX": host(x.grad), "dW": None if dW is None else dW.reshape((s.ksize ** 3, cin, -1)),
            "db": None if layer.bias is None or layer.bias.grad is None else host(layer.bias.grad).reshape(-1)}


def compare(who, got, want, idx, names=("out", "dX", "dW", "db")):
    for name in names:
        w = want[name][idx] if name == "out" else want[name]
        assert got[name] is not None, f"{who}: no {name}"
        assert got[name].dtype == np.float32 and np.array_equal(got[name], w), gc.describe_mismatch(who, name + (" (product row order)" if name == "out" else ""), got[name], w)


_REFS = {}


def shared_expected(s, ops, mode, cin, cout, family):
    """the references of one (kind, size), computed once and shared among the modes that expect the same values"""
    ln = gc.launches(mode, cin, cout, s.ksize ** 3)
    rounds = (False,) * 3 if family == "int" else (ln.fwd == MODE_BF16, ln.adj == MODE_BF16, ln.wgrad_bf16)      # (integers are bf16 numbers)
    if _REFS.get("group") != (s.kind, s.size):
        _REFS.clear()
        _REFS["group"] = (s.kind, s.size)
    key = (cin, cout, family, rounds)
    if key not in _REFS:
        _REFS[key] = gc.expected(s, ops, mode, cin, cout)
    return _REFS[key]


def check_exact(s, ops, mode, who):
    gc.assert_exact(s, ops, who)
    if mode == "bf16":                                       # (rounding can move the largest operand up to the next power of two)
        gc.assert_exact(s, ops._replace(X=gc.bf16_round(ops.X), W=gc.bf16_round(ops.W), dY=gc.bf16_round(ops.dY)), who)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode,size", gc.int_cases())
def test_layer_gradients_are_exact_on_integers(pcc, kind, mode, size):
    s = gc.sets_of(kind, size)
    maps = device_maps(pcc, s)
    with arithmetic(mode):
        for cin, cout in gc.shapes_of(size):
            who = (kind, mode, size, (cin, cout), "int")
            ops = gc.operands(s, cin, cout, "int")
            check_exact(s, ops, "f32", who)
            want = shared_expected(s, ops, mode, cin, cout, "int")
            compare(who, run_layer(pcc, s, maps, cin, cout, ops), want, maps[2])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode,size", gc.wide_cases())
def test_layer_gradients_are_exact_on_wide_mantissas(pcc, kind, mode, size):
    """fp32 and x3 keep every operand bit; a bf16 launch computes the value of its rounded operands — which differs from the
    unrounded one on the family whose wide operand it reads, so an expected bf16 launch that did not run in bf16 fails"""
    s = gc.sets_of(kind, size)
    maps = device_maps(pcc, s)
    with arithmetic(mode):
        for cin, cout in gc.WIDE_SHAPES:
            ln = gc.launches(mode, cin, cout, s.ksize ** 3)
            for family in gc.WIDE:
                who = (kind, mode, size, (cin, cout), family)
                ops = gc.operands(s, cin, cout, family)
                check_exact(s, ops, mode, who)
                want = shared_expected(s, ops, mode, cin, cout, family)
                plain = want if mode != "bf16" else shared_expected(s, ops, "f32", cin, cout, family)
                for name, rounded, reads in (("out", ln.fwd == MODE_BF16, ("wideX", "wideW")), ("dX", ln.adj == MODE_BF16, ("wideG", "wideW")),
                                             ("dW", ln.wgrad_bf16, ("wideX", "wideG"))):
                    if mode == "bf16" and family in reads:
                        assert rounded == (not np.array_equal(want[name], plain[name])), (who, name, "rounding the operands must change exactly the bf16 launches")
                assert mode != "bf16" or np.array_equal(want["db"], plain["db"])
                compare(who, run_layer(pcc, s, maps, cin, cout, ops), want, maps[2])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("kind", gc.VARIANT_KINDS)
def test_layer_gradient_variants(pcc, kind, mode):
    """no bias; x without gradient (dW must still be right); kernel and bias frozen (dX alone: in bf16 the branch without the weight
    gradient's bf16 copy); out_channels = 1 (columns >= 1 of dW and db exactly zero); a stride-0 dY (out.sum().backward())"""
    s = gc.sets_of(kind, "shell1k")
    maps = device_maps(pcc, s)
    idx = maps[2]
    with arithmetic(mode):
        for cin, cout in gc.VARIANT_SHAPES:
            ops = gc.operands(s, cin, cout, "int")
            check_exact(s, ops, "f32", (kind, mode, cin, cout))
            want = gc.expected(s, ops, mode, cin, cout)
            who = lambda v: (kind, mode, "shell1k", (cin, cout), v)
            # no bias
            nb = ops._replace(b=None)
            got = run_layer(pcc, s, maps, cin, cout, nb)
            compare(who("no_bias"), got, dict(want, out=gc.expected(s, nb, mode, cin, cout)["out"]), idx, ("out", "dX", "dW"))
            assert got["db"] is None
            # x without gradient
            got = run_layer(pcc, s, maps, cin, cout, ops, x_grad=False)
            compare(who("x_frozen"), got, want, idx, ("out", "dW", "db"))
            assert got["dX"] is None
            # kernel and bias frozen
            got = run_layer(pcc, s, maps, cin, cout, ops, w_grad=False)
            compare(who("w_frozen"), got, want, idx, ("out", "dX"))
            assert got["dW"] is None and got["db"] is None
            # a stride-0 dY
            ones = ops._replace(dY=np.ones_like(ops.dY))
            gc.assert_exact(s, ones)
            compare(who("sum_backward"), run_layer(pcc, s, maps, cin, cout, ones, sum_backward=True), gc.expected(s, ones, mode, cin, cout), idx)
        # out_channels = 1 on a 64 -> 64 layer: one output column of W, bias, dY
        ops = gc.operands(s, 64, 64, "int")
        one = ops._replace(W=np.ascontiguousarray(ops.W[:, :, :1]), b=ops.b[:1], dY=np.ascontiguousarray(ops.dY[:, :1]))
        gc.assert_exact(s, one)
        want = gc.expected(s, one, mode, 64, 1)
        got = run_layer(pcc, s, maps, 64, 64, ops._replace(dY=one.dY), out_channels=1)
        assert got["out"].shape == (s.out.shape[0], 1) and got["dW"].shape == ops.W.shape and got["db"].shape == (64,)
        full = {"out": want["out"], "dX": want["dX"], "dW": np.zeros(ops.W.shape), "db": np.zeros(64)}
        full["dW"][:, :, :1], full["db"][:1] = want["dW"], want["db"]
        assert np.abs(want["dW"]).max() > 0 and np.abs(want["db"]).max() > 0
        compare((kind, mode, "shell1k", (64, 64), "out_channels_1"), got, full, idx)


def epilogue_reference(act, c, beta, gamma, res, G):
    """out = act(c beta + gamma) + res (beta, gamma or res None: that term is absent) and the gradients of its inputs, in numpy
    float32 in the kernel's operation order.  On integers every step is exact except leaky ReLU's single multiplication by 0.01f
    (and what is computed from its result)."""
    f = np.float32
    c, G = c.astype(f), G.astype(f)
    u = c if beta is None else c * beta + gamma
    slope = f(0.0) if act == 1 else f(0.01)
    v = u if act == 0 else np.where(u > 0, u, slope * u)
    du = G if act == 0 else G * np.where(u > 0, f(1.0), slope)
    return {"out": v if res is None else v + res, "dc": du if beta is None else du * beta, "dbeta": du * c, "dgamma": du}


EPILOGUE_FORMS = ((True, True), (True, False), (False, True))          # (FiLM, residual)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("kind", gc.VARIANT_KINDS)
def test_layer_with_the_training_epilogue(pcc, kind, mode):
    """act(c beta + gamma) + residual on top of the convolution (act x FiLM x residual), integer beta, gamma, residual: identity
    and ReLU through the layer call, everything exact (the convolution's gradients are those of dY = dc); leaky ReLU as
    convolution + epilogue_train with the convolution's output kept: out, dc, dfilm equal the float32 restatement"""
    from pcc_amd import autograd
    s = gc.sets_of(kind, "shell1k")
    in_map, out_map, idx = device_maps(pcc, s)
    n_out = s.out.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a[idx])).to(DEV)
    with arithmetic(mode):
        for cin, cout in gc.VARIANT_SHAPES:
            ops = gc.operands(s, cin, cout, "int")
            rng = np.random.default_rng([cin, cout, n_out, 41])
            beta, gamma, res = (rng.integers(-3, 4, size=(n_out, cout)).astype(np.float32) for _ in range(3))
            c = gc.expected(s, ops, mode, cin, cout)["out"]
            assert np.abs(c).max() * 3 + 3 < gc.EXACT_LIMIT
            for act in gc.EPILOGUE_ACTS:
                for with_film, with_res in EPILOGUE_FORMS:
                    who = (kind, mode, "shell1k", (cin, cout), f"epilogue act {act} film {with_film} residual {with_res}")
                    e = epilogue_reference(act, c, beta if with_film else None, gamma, res if with_res else None, ops.dY)
                    fm = dev(np.concatenate([beta, gamma], axis=1)).requires_grad_(True) if with_film else None
                    rs = dev(res).requires_grad_(True) if with_res else None
                    layer = make_layer(pcc, s, cin, cout, ops)
                    x = torch.from_numpy(ops.X).to(DEV).requires_grad_(True)
                    if act != 2:
                        through = ops._replace(dY=e["dc"])
                        gc.assert_exact(s, through, who)
                        want = gc.expected(s, through, mode, cin, cout)
                        out = layer(pcc.SparseTensor(x, coordinate_map=in_map), act=act, film=fm, residual=rs).F
                        out.backward(dev(ops.dY))
                        dc = None
                        grads = {"dX": x.grad.cpu().numpy(), "dW": layer.kernel.grad.cpu().numpy().reshape(ops.W.shape),
                                 "db": layer.bias.grad.cpu().numpy().reshape(-1)}
                        compare(who, grads, want, idx, ("dX", "dW", "db"))
                    else:
                        conv = layer(pcc.SparseTensor(x, coordinate_map=in_map)).F
                        conv.retain_grad()
                        out = autograd.epilogue_train(conv, fm, rs, act)
                        out.backward(dev(ops.dY))
                        assert np.array_equal(conv.detach().cpu().numpy(), c[idx])
                        dc = conv.grad.cpu().numpy()
                        assert (e["dc"] != np.round(e["dc"])).any()                    # (the slope was applied somewhere)
                    checks = [("out", out.detach().cpu().numpy(), e["out"]), ("dc", dc, e["dc"])]
                    if with_film:
                        checks += [("dbeta", fm.grad.cpu().numpy()[:, :cout], e["dbeta"]), ("dgamma", fm.grad.cpu().numpy()[:, cout:], e["dgamma"])]
                    if with_res:
                        checks.append(("dresidual", rs.grad.cpu().numpy(), ops.dY))
                    for name, got_a, want_a in checks:
                        if got_a is not None:
                            assert got_a.dtype == np.float32 and np.array_equal(got_a, want_a[idx]), gc.describe_mismatch(who, name + " (product row order)", got_a, want_a[idx])
