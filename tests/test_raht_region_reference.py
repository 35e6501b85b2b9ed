"""The properties the PCR2 stream rests on, on the CPU (tests/_raht_region_reference.py): the blocks of the Morton keys are the
blocks the plan's steps give, the range minimum over the rows a coefficient summarises equals the walk over the transform's
steps, and every row of a block of the finest level decodes bitwise as under uniform coding at that level.  Also the host side of
pcc_amd.raht: the level tables, the table choice under the level shift against its symbol-by-symbol restatement, and the header
checks of the PCR2 parser, which run before anything touches a GPU."""
import struct

import numpy as np
import pytest

import _raht_reference as ref
import _raht_region_reference as reg

CASES = sorted(ref.cases())


def _plan(name):
    coords, origin, depth = ref.cases()[name]
    return coords, ref.plan(coords, origin, depth)


@pytest.mark.parametrize("name", CASES)
def test_blocks_and_coefficient_levels_two_ways(name):
    coords, p = _plan(name)
    for b in reg.block_sizes(p["depth"], with_17=False):
        by_keys, n_keys = reg.blocks_from_keys(p, b)
        by_steps, n_steps = reg.blocks_from_steps(p, b)
        assert n_keys == n_steps and np.array_equal(by_keys, by_steps), b
        if b >= p["depth"]:
            assert n_keys == 1
        if b == 0:
            assert n_keys == coords.shape[0]
        for key, levels in reg.level_maps(coords).items():
            bl = reg.block_levels(p, levels, by_keys, n_keys)
            want = reg.coeff_levels_range_min(p, bl, by_keys)
            assert np.array_equal(reg.coeff_levels_walk(p, bl, by_keys), want), (b, key)
            assert want[0] == levels.min() and (want <= bl[by_keys]).all()


@pytest.mark.parametrize("b", (0, 1, 3))
@pytest.mark.parametrize("name", ("shell32", "random92", "random4000", "dense514", "deep300"))
def test_rows_of_the_finest_blocks_are_exact(name, b):
    """a block whose level is the cloud's smallest decodes bitwise as under uniform coding at that level: every coefficient
    above it carries the minimum"""
    coords, p = _plan(name)
    steps = reg.level_steps(4 / 255)
    a = ref.attributes(coords.shape[0], 3, seed=13)
    co = ref.forward(p, a)
    block_of_row, n_blocks = reg.blocks_from_keys(p, b)
    for key in ("halves", "random"):
        levels = reg.level_maps(coords)[key]
        bl = reg.block_levels(p, levels, block_of_row, n_blocks)
        cl = reg.coeff_levels_range_min(p, bl, block_of_row)
        finest = int(bl.min())
        rec = ref.inverse(p, reg.dequantize(reg.quantize(co, cl, steps), cl, steps))
        flat = np.full(coords.shape[0], finest, dtype=np.uint8)
        uniform = ref.inverse(p, reg.dequantize(reg.quantize(co, flat, steps), flat, steps))
        rows = bl[block_of_row] == finest
        assert rows.any() and np.array_equal(rec[rows].view(np.uint64), uniform[rows].view(np.uint64)), key
        if name in ("shell32", "random4000"):
            assert not rows.all() and not np.array_equal(rec[~rows], uniform[~rows]), key


def test_level_steps_and_quality_levels(pcc):
    from pcc_amd import raht
    for q in (4 / 255, 0.25 / 255, 1.0, 0.1):
        steps = raht.level_steps(q)
        assert steps.dtype == np.float64 and steps.shape == (64,) and steps[0] == q
        assert np.array_equal(steps, reg.level_steps(q)) and (np.diff(steps) > 0).all()
        assert abs(steps[63] / q - 256.0 / 0.11) <= 1e-9 * 256.0 / 0.11
    # one level is one spacing of the Gaussian scale table
    table = raht.get_scale_table().double().numpy()
    assert np.allclose(table[1:] / table[:-1], raht.level_steps(1.0)[1], rtol=1e-5)
    with pytest.raises(ValueError):
        raht.level_steps(0.0)
    # ties to even: (1 - q) * 2 = 0.5, 1.5 and (1 - q) * 4 = 2.5
    assert raht.quality_levels(np.array([0.75, 0.25]), span=2).tolist() == [0, 2]
    assert raht.quality_levels(np.array([0.375]), span=4).tolist() == [2]
    got = raht.quality_levels(np.array([[1.0, 0.0, 0.5, -3.0, 7.0]]))
    assert got.dtype == np.uint8 and got.tolist() == [[0, 24, 12, 24, 0]]
    assert raht.quality_levels(np.array([0.0]), span=63).tolist() == [63] and raht.quality_levels(np.array([0.2]), span=0).tolist() == [0]
    import torch
    t = raht.quality_levels(torch.tensor([0.75, 0.25, 1.0]), span=2)
    assert t.dtype == torch.uint8 and t.tolist() == [0, 2, 0]
    for span in (64, -1):
        with pytest.raises(ValueError):
            raht.quality_levels(np.array([0.5]), span=span)


def _symbols(seed=7):
    rng = np.random.default_rng(seed)
    sym = np.concatenate([np.rint(rng.normal(0, s, 60)).astype(np.int64) for s in (0.05, 0.4, 3.0, 40.0, 900.0)] + [np.array([70000, -3])])
    ctx = np.concatenate([np.full(60, k) for k in (0, 1, 2, 3, 5)] + [np.array([6, 6])])
    return sym, ctx, rng


def test_shifted_table_choice_equals_its_restatement(pcc):
    from pcc_amd import raht
    tables = raht.gaussian_tables()
    sym, ctx, rng = _symbols()
    for shift in (rng.integers(0, 4, sym.size), rng.integers(0, 64, sym.size), np.full(sym.size, 63), np.zeros(sym.size, dtype=np.int64),
                  np.where(np.arange(sym.size) % 2, 12, 0)):
        got = raht.choose_tables(sym, ctx, 8, shift=shift)
        assert got.dtype == np.uint8 and np.array_equal(got, reg.choose_tables_shifted(sym, ctx, 8, shift, *tables))
        assert got[4] == 0 and got[7] == 0                   # empty contexts
    # no shift at all is the rule without one, and shift=None is that code path
    plain = raht.choose_tables(sym, ctx, 8)
    assert np.array_equal(raht.choose_tables(sym, ctx, 8, shift=None), plain)
    assert np.array_equal(plain, ref.choose_tables(sym, ctx, 8, *tables))
    assert np.array_equal(raht.choose_tables(sym, ctx, 8, shift=np.zeros(sym.size, dtype=np.int64)), plain)
    # symbols divided by two table spacings are served by the table two below, named two above: the shifted choice of the
    # whole is the plain choice of the undivided half
    wide = np.rint(rng.normal(0, 40.0, 4000)).astype(np.int64)
    ratio = raht.level_steps(1.0)[6]
    both = np.concatenate([wide, np.rint(wide / ratio).astype(np.int64)])
    shift = np.concatenate([np.zeros(4000, dtype=np.int64), np.full(4000, 6)])
    t_wide = int(raht.choose_tables(wide, np.zeros(4000, dtype=np.int64), 1)[0])
    assert abs(int(raht.choose_tables(both, np.zeros(8000, dtype=np.int64), 1, shift=shift)[0]) - t_wide) <= 1
    for bad in (np.zeros(3), -np.ones(sym.size)):
        with pytest.raises(ValueError):
            raht.choose_tables(sym, ctx, 8, shift=bad)


class _FakePlan:
    """what the PCR2 parser reads of a plan before it decodes anything"""
    def __init__(self, n, depth):
        self.n, self.depth = n, depth


def _pcr2(pcc, levels=(3, 5, 0, 0, 63), n=9, depth=2, c=3, block_log2=1, qstep=0.25, magic=b"PCR2", zero=0, n_blocks=None, level_table=None,
          table_value=0, payload=b"\x00" * 8):
    """a well-formed PCR2 stream of ``len(levels)`` blocks (the payload is never decoded by the parser)"""
    from pcc_amd import raht
    from pcc_amd.entropy import _rans_encode
    deltas = np.diff(np.asarray(levels, dtype=np.int64), prepend=0)
    t = int(raht.choose_tables(deltas, np.zeros(deltas.size, dtype=np.int64), 1)[0]) if level_table is None else level_table
    coded = _rans_encode(deltas.astype(np.int32), np.full(deltas.size, min(t, 63), dtype=np.int32), *raht.gaussian_tables())
    return (reg.HEAD.pack(magic, depth, c, block_log2, zero, qstep, n, len(levels) if n_blocks is None else n_blocks, t, len(coded)) + coded
            + struct.pack("<%dq" % c, *range(c)) + bytes([table_value]) * (3 * depth * c) + struct.pack("<I", len(payload)) + payload)


def test_pcr2_header_checks(pcc):
    from pcc_amd import raht
    plan = _FakePlan(9, 2)
    five = lambda b: 5
    good = _pcr2(pcc)
    c, block_log2, qstep, levels, dc, table, payload = raht.parse_region(plan, good, five)
    assert (c, block_log2, qstep, levels.tolist(), dc.tolist(), payload) == (3, 1, 0.25, [3, 5, 0, 0, 63], [0, 1, 2], b"\x00" * 8)
    assert table.shape == (18,) and reg.parse(good)["n_blocks"] == 5
    # a cut at every field boundary, and inside the last field
    bounds = reg.field_boundaries(good)
    assert bounds[-1] == len(good) and bounds[10] == 29 and len(bounds) == 16
    for cut in bounds[:-1] + [len(good) - 3]:
        with pytest.raises(ValueError):
            raht.parse_region(plan, good[:cut], five)
    for bad in (_pcr2(pcc, magic=b"PCR1"), _pcr2(pcc, n=10), _pcr2(pcc, depth=3), _pcr2(pcc, c=0), _pcr2(pcc, c=17), _pcr2(pcc, qstep=0.0),
                _pcr2(pcc, qstep=float("inf")), _pcr2(pcc, block_log2=18), _pcr2(pcc, zero=1), _pcr2(pcc, level_table=64),
                _pcr2(pcc, n_blocks=4), _pcr2(pcc, n_blocks=6),                              # n_blocks off by one, either way
                _pcr2(pcc, levels=(3, 5, 0, -1, 63)), _pcr2(pcc, levels=(3, 64, 0, 0, 63)),    # a delta that leaves 0 .. 63
                _pcr2(pcc, levels=(60, 61, 62, 63, 64)), _pcr2(pcc, levels=(-1, 0, 0, 0, 0)),
                _pcr2(pcc, table_value=64),                                                    # a table index that names no table
                b""):
        with pytest.raises(ValueError):
            raht.parse_region(plan, bad, five)
    # the block count is compared with the geometry's before the levels are decoded
    with pytest.raises(ValueError):
        raht.parse_region(plan, good, lambda b: 6)
    with pytest.raises(ValueError):
        raht.parse_region(_FakePlan(4, 2), _pcr2(pcc, n=4), five)          # more blocks than rows
    # and decode_attributes sends a PCR2 magic to this parser, decode_symbols keeps refusing it
    with pytest.raises(ValueError):
        raht.decode_symbols(plan, good)
