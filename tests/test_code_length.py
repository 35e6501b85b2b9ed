"""The code-length kernels (csrc/code_length.hip) against the numpy restatement (tests/_code_length_reference.py): equality per
channel and in the operation, escape and flag words, for the Gaussian conditional (pcc_gc_code_length), the factorized model
(pcc_eb_code_length) and planes that exist already (pcc_code_length_planes).

Shapes: n in {1, 63, 64, 65, 257, 4099} x c in {1, 3, 8, 128} (3 = the q-map hyperprior's width), plus 8209 x 128, the one
that fills the capped grid.  A workgroup of 256 threads takes 1,024 elements in four steps, so every shape above 1,024
elements loops, and n * c is a multiple of the grid's element stride for 64 x 128 alone.  The stride is a multiple of c for
c in {1, 8, 128} (a thread keeps its channel) and is not for c = 3 (a thread's channel moves on every step).  The symbols
and indexes the fused kernels derive are restated in numpy as well (float32 subtraction and rint, a count of table entries),
and must equal what pcc_gc_encode_prep / pcc_eb_quantize write."""
import numpy as np
import pytest
import torch

import _code_length_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = [1, 63, 64, 65, 257, 4099]
CS = [1, 3, 8, 128]
SHAPES = [(n, c) for c in CS for n in NS] + [(8209, 128)]


@pytest.fixture(scope="module")
def gaussian(pcc):
    from pcc_amd import entropy as E
    gc = E.GaussianConditional(None).to(DEV)
    gc.update_scale_table(E.get_scale_table())
    cdf, sizes, off = gc.tables()
    return gc, ref.cost_table(cdf, sizes), sizes, off


@pytest.fixture(scope="module")
def factorized(pcc):
    """c -> (EntropyBottleneck(c) with seeded density parameters, cost, cdf_sizes, offsets)"""
    from pcc_amd import entropy as E
    made = {}

    def get(c):
        if c not in made:
            torch.manual_seed(100 + c)
            eb = E.EntropyBottleneck(c)
            eb.update()
            eb = eb.to(DEV)
            cdf, sizes, off = eb.tables()
            made[c] = (eb, ref.cost_table(cdf, sizes), sizes, off)
        return made[c]

    return get


def _gaussian_inputs(gc, n, c, seed):
    """y, params with every scale level present (n * c >= 64), scales below the 0.11 bound (and below zero), and values that
    leave their table on either side by one to eight nibbles"""
    rng = np.random.default_rng(seed)
    table = gc.scale_table.cpu().numpy()
    levels = table.size
    e = n * c
    pick = np.arange(e) % levels if e >= levels else rng.integers(0, levels, e)
    scales = (table[pick] * rng.uniform(0.93, 1.0, e)).astype(np.float32)          # at or just under the level's own entry
    low = rng.random(e)
    low[:levels] = 1.0                                                             # (the first of every level stays)
    scales[low < 0.05] = np.float32(0.05)                                          # below the bound
    scales[low < 0.02] = np.float32(-3.0)
    means = rng.normal(0.0, 2.0, e).astype(np.float32)
    y = (means + rng.normal(0.0, 1.0, e) * np.maximum(scales, 0.11)).astype(np.float32)
    far = rng.random(e) < 0.04
    y[far] += (rng.choice([-1.0, 1.0], far.sum()) * 16.0 ** rng.integers(0, 7, far.sum()) * 9).astype(np.float32)      # |v| up to 1.5e8: 8 nibbles
    params = np.concatenate([scales.reshape(n, c), means.reshape(n, c)], axis=1)
    return y.reshape(n, c), np.ascontiguousarray(params), table


def _gaussian_planes(y, params, table):
    """numpy: what pcc_gc_encode_prep writes, [c, n]"""
    n, c = y.shape
    scale = np.maximum(params[:, :c], np.float32(0.11))
    idx = (table.size - 1) - (scale[:, :, None] <= table[None, None, :-1]).sum(axis=2)
    sym = np.rint(y - params[:, c:]).astype(np.int64)
    return sym.T.astype(np.int32), idx.T.astype(np.int32)


def _host(cl):
    return cl.raw.cpu().numpy()


@pytest.mark.parametrize("n,c", SHAPES)
def test_gaussian_code_length_equals_the_restatement(pcc, gaussian, n, c):
    gc, cost, sizes, off = gaussian
    y, params, table = _gaussian_inputs(gc, n, c, seed=n * 1000 + c)
    sym, idx = _gaussian_planes(y, params, table)
    want = ref.code_length(sym, idx, cost, sizes, off)
    assert want[c + 2] == 0
    if n * c >= 64:
        assert np.unique(idx).size == 64                                            # every scale level is hit
    if n * c >= 4096:
        q16, ops, esc, _ = ref.symbol_costs(sym, idx, cost, sizes, off)
        v = sym.reshape(-1) - off[idx.reshape(-1)]
        assert (esc & (v < 0)).any() and (esc & (v > 0)).any() and ops.max() >= 6   # escapes on both sides, several nibbles
    yd, pd = torch.from_numpy(y).to(DEV), torch.from_numpy(params).to(DEV)
    got = gc.code_length(yd, pd)
    assert got.q16_bits_per_channel.shape == (c,) and got.q16_bits_per_channel.dtype == torch.int64 and got.symbols == n * c
    assert got.raw.is_cuda and got.ops.is_cuda and got.escapes.is_cuda and got.flags.is_cuda
    assert np.array_equal(_host(got), want), (n, c)
    # the planes pcc_gc_encode_prep writes are the restated ones, and cost the same through pcc_code_length_planes
    sym_d, idx_d = gc.encode_prep(yd, pd)
    assert np.array_equal(sym_d.cpu().numpy(), sym) and np.array_equal(idx_d.cpu().numpy(), idx)
    assert np.array_equal(_host(gc.code_length_planes(sym_d, idx_d)), want)
    # integer sums: a second run agrees bit for bit
    assert torch.equal(gc.code_length(yd, pd).raw, got.raw)


@pytest.mark.parametrize("n,c", SHAPES)
def test_factorized_code_length_equals_the_restatement(pcc, factorized, n, c):
    eb, cost, sizes, off = factorized(c)
    rng = np.random.default_rng(n * 1000 + c + 7)
    med = eb.medians().cpu().numpy()
    z = (med[None, :] + rng.normal(0.0, 6.0, (n, c))).astype(np.float32)
    far = rng.random((n, c)) < 0.04
    z[far] += (rng.choice([-1.0, 1.0], far.sum()) * 16.0 ** rng.integers(1, 7, far.sum())).astype(np.float32)
    sym = np.rint(z - med[None, :].astype(np.float32)).astype(np.int64).T.astype(np.int32)
    idx = np.repeat(np.arange(c, dtype=np.int32), n).reshape(c, n)
    want = ref.code_length(sym, idx, cost, sizes, off)
    assert want[c + 2] == 0 and (n * c < 4096 or want[c + 1] > 0)
    zd = torch.from_numpy(z).to(DEV)
    got = eb.code_length(zd)
    assert np.array_equal(_host(got), want), (n, c)
    sym_d, _ = eb.quantize_features(zd, want_zhat=False)
    assert np.array_equal(sym_d.cpu().numpy(), sym)
    assert np.array_equal(_host(eb.code_length_planes(sym_d, torch.from_numpy(idx).to(DEV))), want)
    assert torch.equal(eb.code_length(zd).raw, got.raw)


def test_cost_tables_on_the_device_are_the_host_builders(pcc, gaussian, factorized):
    gc, cost, _, _ = gaussian
    dev_cost = gc.cost_tables(DEV)
    assert dev_cost.dtype == torch.int32 and dev_cost.is_cuda and np.array_equal(dev_cost.cpu().numpy(), cost)
    assert gc.cost_tables(DEV) is dev_cost                                          # uploaded once
    eb, cost, _, _ = factorized(8)
    assert np.array_equal(eb.cost_tables(DEV).cpu().numpy(), cost)
    eb.update(force=True)                                                           # new tables: the matrix is rebuilt
    assert "cuda" not in {d.type for d in eb.__dict__["_cost_tables"]}


def test_error_flags_are_raised_on_valid_memory(pcc, gaussian):
    """an index outside the tables and a slot of frequency 0 set their flag bits (the lane coder's meanings); the launch reads
    nothing it was not given and returns normally"""
    from pcc_amd.entropy import check, ptr
    gc, cost, sizes, off = gaussian
    n, c = 300, 3
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 64, (c, n)).astype(np.int32)
    sym = rng.integers(-2, 3, (c, n)).astype(np.int32)
    clean = ref.code_length(sym, idx, cost, sizes, off)
    assert clean[c + 2] == 0
    for bad in (64, -1, 2 ** 31 - 1):
        idx2 = idx.copy()
        idx2[1, 17] = bad
        got = _host(gc.code_length_planes(torch.from_numpy(sym).to(DEV), torch.from_numpy(idx2).to(DEV)))
        assert got[c + 2] == ref.FLAG_INDEX and np.array_equal(got, ref.code_length(sym, idx2, cost, sizes, off))
    # a planted table set with a slot of frequency 0 (table 1, slot 1), through the C entry point
    L = pcc.lib()
    cdf = np.zeros((2, 6), dtype=np.int32)
    cdf[0, :6] = [0, 1, 2, 40000, 65535, 65536]
    cdf[1, :5] = [0, 30000, 30000, 65000, 65536]
    tsizes, toff = np.array([6, 5], dtype=np.int32), np.array([-2, -1], dtype=np.int32)
    tcost = np.empty_like(cdf)
    check(L.pcc_code_length_tables_build(ptr(cdf), 6, ptr(tsizes), 2, ptr(tcost)))
    assert np.array_equal(tcost, ref.cost_table(cdf, tsizes))
    sym = np.array([[-2, -1, 0, 1, 5, -9], [-1, 1, 1, 1, 7, -1]], dtype=np.int32)
    idx = np.array([[0] * 6, [1] * 6], dtype=np.int32)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    d_cost, d_sizes, d_off = dev(tcost), dev(tsizes), dev(toff)

    def run(sym, idx):
        out = torch.full((2 + 3,), -1, dtype=torch.int64, device=DEV)
        d_sym, d_idx = dev(sym), dev(idx)                                           # (held until the result has been read)
        check(L.pcc_code_length_planes(ptr(d_sym), ptr(d_idx), sym.shape[1], 2, ptr(d_cost), 6, ptr(d_sizes), ptr(d_off), 2, ptr(out),
                                       pcc._lib.stream()))
        return out.cpu().numpy()

    want = ref.code_length(sym, idx, tcost, tsizes, toff)
    assert want[4] == 0 and np.array_equal(run(sym, idx), want)
    hit = sym.copy()
    hit[1, 2] = 0                                                                   # v = 1 of table 1: frequency 0
    want = ref.code_length(hit, idx, tcost, tsizes, toff)
    assert want[4] == ref.FLAG_FREQ0 and np.array_equal(run(hit, idx), want)
    # arguments the entry points refuse
    out = torch.full((5,), -1, dtype=torch.int64, device=DEV)
    d_sym, d_idx = dev(sym), dev(idx)
    assert L.pcc_code_length_planes(ptr(d_sym), ptr(d_idx), 6, 0, ptr(d_cost), 6, ptr(d_sizes), ptr(d_off), 2, ptr(out), pcc._lib.stream()) < 0
    assert L.pcc_code_length_planes(ptr(d_sym), ptr(d_idx), 0, 2, ptr(d_cost), 6, ptr(d_sizes), ptr(d_off), 2, ptr(out), pcc._lib.stream()) == 0
    assert out.cpu().tolist() == [0] * 5                                            # no symbols: the sums are still cleared
