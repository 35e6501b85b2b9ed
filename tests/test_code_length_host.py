"""Code length on the host (no GPU): the cost-table builder against its numpy restatement, and the derived interval of
entropy.stream_bytes_interval against the stream lengths of the real host coders (the reference-format coder and the host twin
of the lane-parallel one), on the model's own 64 Gaussian tables and on a seeded factorized table set.

The interval is derived (entropy.stream_bytes_interval's docstring), not fitted: per stream the word count W obeys
S - 32 - E < 32 W <= S + E with S the exact table cost in bits and E = ops * (-log2(1 - 2^-15) + 2^-17), carried as
E16 = ceil(ops * 3386 / 1000) in 1/65536 bit.  Its width is therefore 4 bytes per stream plus 4 bytes per full word in 2 E:
the tests assert that width, so a looser interval does not pass."""
import math

import numpy as np
import pytest
import torch

import _code_length_reference as ref

WORD = 32 << 16                       # one 32-bit word in Q16 bits
NUM, DEN = 3386, 1000                 # the derived per-operation slack in Q16 bits


@pytest.fixture(scope="module")
def gaussian_tables(pcc):
    from pcc_amd import entropy as E
    gc = E.GaussianConditional(None)
    gc.update_scale_table(E.get_scale_table())
    return gc.tables()


@pytest.fixture(scope="module")
def factorized_tables(pcc):
    from pcc_amd import entropy as E
    torch.manual_seed(5)
    eb = E.EntropyBottleneck(8)
    eb.update()
    return eb.tables()


def _build(pcc, cdf, sizes):
    from pcc_amd.entropy import check, ptr
    out = np.empty_like(cdf)
    check(pcc.lib().pcc_code_length_tables_build(ptr(cdf), cdf.shape[1], ptr(sizes), sizes.size, ptr(out)))
    return out


def test_slack_constant_is_the_derived_one(pcc):
    from pcc_amd import entropy as E
    exact = 65536.0 * -math.log2(1.0 - 2.0 ** -15) + 0.5          # one put's state error + one table cost's Q16 rounding
    assert (E.OP_SLACK_NUM, E.OP_SLACK_DEN) == (NUM, DEN)
    assert exact <= NUM / DEN < exact + 1e-3
    assert -math.log2(1.0 - 2.0 ** -15) <= 2.0 ** -15 * math.log2(math.e) * (1 + 2.0 ** -15)


def test_cost_tables_equal_the_restatement(pcc, gaussian_tables, factorized_tables):
    for cdf, sizes, _ in (gaussian_tables, factorized_tables):
        got = _build(pcc, cdf, sizes)
        assert got.dtype == np.int32 and np.array_equal(got, ref.cost_table(cdf, sizes))
        assert (got[np.arange(sizes.size), sizes - 2] > 0).all()          # every escape slot is codable
    # planted rows: a frequency-1 slot, a frequency-0 slot, a table of one symbol and the escape, a table whose one slot takes
    # the whole range (65536 reads as frequency 0 in the coder's 16 bits: it cannot code that slot, so the cost is -1 too)
    cdf = np.zeros((4, 6), dtype=np.int32)
    sizes = np.array([6, 5, 3, 2], dtype=np.int32)
    cdf[0, :6] = [0, 1, 2, 40000, 65535, 65536]
    cdf[1, :5] = [0, 30000, 30000, 65000, 65536]
    cdf[2, :3] = [0, 65535, 65536]
    cdf[3, :2] = [0, 65536]
    got = _build(pcc, cdf, sizes)
    assert np.array_equal(got, ref.cost_table(cdf, sizes))
    assert got[0, 0] == got[0, 1] == 16 << 16 and got[0, 4] == 16 << 16 and got[0, 5] == -1
    assert got[1, 1] == -1 and got[1, 0] > 0 and got[1, 4] == -1
    assert got[2, 0] == round(65536 * (16 - math.log2(65535))) and got[2, 1] == 16 << 16 and got[2, 2] == -1
    assert got[3, 0] == -1
    L = pcc.lib()
    assert L.pcc_code_length_tables_build(cdf.ctypes.data, 6, np.array([7, 5, 3, 2], dtype=np.int32).ctypes.data, 4, got.ctypes.data) < 0


def _check(pcc, tables, symbols, indexes, lanes, tag):
    """the real coder's length lies in the interval of the restated cost, and the interval is as narrow as derived"""
    from pcc_amd import entropy as E
    cdf, sizes, off = tables
    cost = ref.cost_table(cdf, sizes)
    q16, ops, esc, flags = ref.symbol_costs(symbols, indexes, cost, sizes, off)
    assert not flags.any()
    S, O, n = int(q16.sum()), int(ops.sum()), int(np.asarray(symbols).size)
    if lanes:
        actual = len(E._rans_lanes_encode_host(symbols, indexes, lanes, cdf, sizes, off))
    else:
        actual = len(E._rans_encode(symbols, indexes, cdf, sizes, off))
    lo, hi = E.stream_bytes_interval(S, O, lanes, symbols=n)
    assert lo <= actual <= hi, (tag, lo, actual, hi)
    streams = min(lanes, n) if lanes else 1
    e16 = -(-O * NUM // DEN)
    words_in_2e = 2 * e16 // WORD
    assert hi - lo <= 4 * streams + 4 * words_in_2e, (tag, lo, hi, streams, e16)
    if streams and (S - e16) // WORD - (streams - 1) >= 0:           # (the lower end is not clamped at "no word at all")
        assert hi - lo >= 4 * (streams - 1) + 4 * words_in_2e, (tag, lo, hi, streams, e16)
    if lanes:                                                        # without the symbol count: every possible number of lanes in use
        lo2, hi2 = E.stream_bytes_interval(S, O, lanes)
        assert lo2 <= lo and hi <= hi2
    return actual, lo, hi, int(esc.sum())


def _gaussian_sequence(rng, tables, n, spread=1.0):
    _, sizes, off = tables
    idx = rng.integers(0, sizes.size, n).astype(np.int32)
    half = (sizes[idx] - 3) // 2                                     # the table's centre .. its last regular symbol
    sym = np.rint(rng.normal(0.0, 1.0, n) * (half * spread / 3.0 + 0.4)).astype(np.int32)
    return sym, idx


@pytest.mark.parametrize("lanes", [0, 1, 3, 64])
@pytest.mark.parametrize("n", [0, 1, 2, 1000, 200000])
def test_gaussian_streams_lie_in_the_interval(pcc, gaussian_tables, n, lanes):
    rng = np.random.default_rng(1000 * lanes + n)
    sym, idx = _gaussian_sequence(rng, gaussian_tables, n)
    actual, lo, hi, _ = _check(pcc, gaussian_tables, sym, idx, lanes, ("gaussian", n, lanes))
    if n == 0:
        assert actual == lo == hi == (8 + 4 * lanes if lanes else 8)
    # wide draws: a few percent of the symbols leave their table on either side
    sym, idx = _gaussian_sequence(rng, gaussian_tables, n, spread=2.0)
    _, _, _, escapes = _check(pcc, gaussian_tables, sym, idx, lanes, ("gaussian wide", n, lanes))
    assert escapes > 0 or n < 1000


@pytest.mark.parametrize("lanes", [0, 1, 3, 64])
@pytest.mark.parametrize("n", [0, 1, 2, 1000, 200000])
def test_factorized_streams_lie_in_the_interval(pcc, factorized_tables, n, lanes):
    _, sizes, off = factorized_tables
    c = sizes.size
    rng = np.random.default_rng(77 + 1000 * lanes + n)
    rows = -(-n // c)
    idx = np.repeat(np.arange(c, dtype=np.int32), rows)[:n]          # channel-major, as the z stream
    sym = (np.rint(rng.normal(0.0, 4.0, n)) + (off[idx] + (sizes[idx] - 2) // 2)).astype(np.int32)
    _check(pcc, factorized_tables, sym, idx, lanes, ("factorized", n, lanes))


def _escape_symbol(tables, ix, nb, negative):
    """a symbol of table ix whose escaped value has exactly nb nibbles"""
    _, sizes, off = tables
    maxv = int(sizes[ix]) - 2
    raw = 16 ** (nb - 1) + (1 if negative else 0) if nb > 1 else (1 if negative else 2)
    raw += (raw % 2 == 0) if negative else (raw % 2)
    v = -(raw + 1) // 2 if negative else maxv + raw // 2
    return v + int(off[ix])


@pytest.mark.parametrize("lanes", [0, 1, 3, 64])
def test_escapes_of_both_signs_and_every_length(pcc, gaussian_tables, lanes):
    _, sizes, off = gaussian_tables
    cost = ref.cost_table(*gaussian_tables[:2])
    rng = np.random.default_rng(9)
    sym, idx, want_nb = [], [], []
    for nb in range(1, 9):
        for negative in (False, True):
            for ix in (0, 17, 63):
                sym.append(_escape_symbol(gaussian_tables, ix, nb, negative))
                idx.append(ix)
                want_nb.append(nb)
    sym, idx = np.array(sym, dtype=np.int32), np.array(idx, dtype=np.int32)
    q16, ops, esc, flags = ref.symbol_costs(sym, idx, cost, sizes, off)
    assert esc.all() and np.array_equal(ops, np.array(want_nb) + 2)          # the symbol, the count nibble, nb value nibbles
    assert np.array_equal(q16, cost[idx, sizes[idx] - 2] + (np.array(want_nb) + 1) * ref.BYPASS_Q16)
    _check(pcc, gaussian_tables, sym, idx, lanes, ("every escape", lanes))
    # the value just past either end of a table (v = maxv: an escape with no value nibble, v = -1: one nibble)
    edge = np.array([int(off[5]) + int(sizes[5]) - 2, int(off[5]) - 1], dtype=np.int32)
    q16, ops, esc, _ = ref.symbol_costs(edge, np.array([5, 5]), cost, sizes, off)
    assert esc.all() and list(ops) == [2, 3]
    _check(pcc, gaussian_tables, edge, np.array([5, 5], dtype=np.int32), lanes, ("edges", lanes))
    # sequences that are all escapes, short and long
    for n in (1, 2, 1000, 20000):
        pick = rng.integers(0, sym.size, n)
        _, _, _, escapes = _check(pcc, gaussian_tables, sym[pick], idx[pick], lanes, ("all escapes", n, lanes))
        assert escapes == n


def test_interval_arguments():
    from pcc_amd import entropy as E
    assert E.stream_bytes_interval(0, 0) == (8, 8) and E.stream_bytes_interval(0, 0, lanes=64) == (8 + 256, 8 + 256)
    assert E.stream_bytes_interval(0, 0, lanes=3, symbols=0) == (20, 20)
    lo, hi = E.stream_bytes_interval(10 * WORD + WORD // 2, 100)
    assert (lo, hi) == (8 + 40, 8 + 40)                                # S - E and S + E share their word
    lo, hi = E.stream_bytes_interval(10 * WORD + 5, 1000)
    assert (lo, hi) == (8 + 36, 8 + 40)                                # E16 = 3386 > 5: the word below comes in
    with pytest.raises(ValueError):
        E.stream_bytes_interval(-1, 0)
