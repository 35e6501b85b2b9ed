"""The numpy restatement of RAHT (tests/_raht_reference.py: the closed-form plan and the step-by-step transform the GPU is compared
with) against the recursive definition, on the CPU: equal coefficients, energy preserved, the inverse returns the input; the
table choice of pcc_amd.raht against its symbol-by-symbol restatement; and the header checks of the PCR1 / PCA1 parsers, which
run before anything touches a GPU."""
import struct

import numpy as np
import pytest

import _raht_reference as ref

CASES = sorted(ref.cases())


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_recursive_definition(name):
    coords, origin, depth = ref.cases()[name]
    p = ref.plan(coords, origin, depth)
    assert p["status"].tolist() == [0, 0]
    for c in (1, 3):
        a = ref.attributes(coords.shape[0], c, seed=11)
        co = ref.forward(p, a)
        assert np.array_equal(co, ref.forward_recursive(p, a))
        # orthonormal: energy is preserved, and the inverse returns the input (in Morton order)
        assert abs((co ** 2).sum() - (a ** 2).sum()) <= 1e-12 * (a ** 2).sum()
        assert np.abs(ref.inverse(p, co) - a[p["perm"]]).max() <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_plan_invariants(name):
    coords, origin, depth = ref.cases()[name]
    p = ref.plan(coords, origin, depth)
    n = coords.shape[0]
    assert p["step"][0] == -1 and (p["step"][1:] >= 0).all() and (p["step"] < 3 * p["depth"]).all()
    assert np.array_equal(np.sort(p["perm"]), np.arange(n)) and np.array_equal(np.sort(p["step_rows"]), np.arange(n))
    assert p["step_offsets"][0] == 0 and p["step_offsets"][-1] == n - 1 and p["step_rows"][-1] == 0
    assert ((p["left"] < np.arange(n)) | (np.arange(n) == 0)).all()
    # every row is the first row of a right node exactly once, and the last merge spans the cloud
    top = p["step_rows"][p["step_offsets"][-1] - 1] if n > 1 else 0
    assert n == 1 or p["w0"][top] + p["w1"][top] == n


def test_plan_reports_duplicates_and_rows_outside():
    coords = np.array([[1, 1, 1], [2, 3, 1], [1, 1, 1], [9, 0, 0], [0, -1, 0]])
    p = ref.plan(coords, (0, 0, 0), 3)
    assert p["status"].tolist() == [2, 2]           # two rows outside (both get key 0: one of them a duplicate), one repeated voxel
    assert ref.plan(coords[:2], (0, 0, 0), 3)["status"].tolist() == [0, 0]


def test_default_origin_and_depth_follow_the_octree_coder():
    coords = np.array([[5, -3, 7], [12, 0, 7], [5, 4, 8]])
    o, d = ref.default_origin_depth(coords)
    assert o.tolist() == [5, -3, 7] and d == 3      # extents 7, 7, 1 -> 3 bits


def test_quantiser_rounds_half_to_even():
    assert ref.quantize(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49, 7.3]), 1.0).tolist() == [0, 2, 2, 0, -2, 0, 7]
    assert ref.near_rounding_boundary(np.array([0.5, 1.0, 1.4999999]), 1.0, 1e-6).tolist() == [True, False, True]


def test_table_choice_equals_its_restatement(pcc):
    from pcc_amd import raht
    cdf, cdf_len, off = raht.gaussian_tables()
    assert cdf.shape[0] == 64
    rng = np.random.default_rng(7)
    sym = np.concatenate([np.rint(rng.normal(0, s, 40)).astype(np.int64) for s in (0.05, 0.4, 3.0, 40.0, 900.0)] + [np.array([70000, -3])])
    ctx = np.concatenate([np.full(40, k) for k in (0, 1, 2, 3, 5)] + [np.array([6, 6])])
    got = raht.choose_tables(sym, ctx, 8)
    want = ref.choose_tables(sym, ctx, 8, cdf, cdf_len, off)
    assert np.array_equal(got, want)
    assert got[4] == 0 and got[7] == 0                       # empty contexts
    assert got[0] < got[1] < got[2] < got[3]                 # wider symbols, wider table
    # the escape's price, as the coder spends it: tail bin + 4 bits per nibble + 4 per group of 15 nibbles
    assert ref.bypass_bits(0) == 4 and ref.bypass_bits(15) == 8 and ref.bypass_bits(16) == 12
    costs = raht.symbol_costs(np.array([0, 100000]))
    maxv = int(cdf_len[0]) - 2
    tail = int(np.rint((16 - np.log2(float(cdf[0, maxv + 1] - cdf[0, maxv]))) * 2 ** 20))
    assert costs[0, 1] == tail + ref.bypass_bits(2 * (100000 - int(off[0]) - maxv)) * 2 ** 20


class _FakePlan:
    """what the PCR1 parser reads of a plan before it decodes anything"""
    def __init__(self, n, depth):
        self.n, self.depth = n, depth


def _pcr1(n=5, depth=2, c=3, qstep=0.25, magic=b"PCR1", payload=b"\x00" * 8):
    return (struct.pack("<4sBBHdI", magic, depth, c, 0, qstep, n) + struct.pack("<%dq" % c, *range(c)) + bytes(3 * depth * c)
            + struct.pack("<I", len(payload)) + payload)


def test_pcr1_header_checks(pcc):
    from pcc_amd import raht
    plan = _FakePlan(5, 2)
    for bad in (_pcr1(magic=b"PCR2"), _pcr1()[:10], _pcr1()[:30], _pcr1()[:-3], _pcr1(n=6), _pcr1(depth=3), _pcr1(c=0), _pcr1(c=17),
                _pcr1(qstep=0.0), _pcr1(qstep=float("nan")), b""):
        with pytest.raises(ValueError):
            raht.decode_symbols(plan, bad)
    data = bytearray(_pcr1())
    data[20 + 24] = 64                                       # a table index that names no table
    with pytest.raises(ValueError):
        raht.decode_symbols(plan, bytes(data))


def test_pca1_header_checks(pcc):
    from pcc_amd import anchor
    good = b"PCA1" + struct.pack("<B3xI", 1, 28) + b"PCO1" + bytes(24)
    for bad in (b"PCA2" + good[4:], good[:8], good[:20], b"PCA1" + struct.pack("<B3xI", 7, 28) + good[12:], b"",
                b"PCA1" + struct.pack("<B3xI", 1, 28) + b"PCO2" + bytes(24), good):       # the last: a cloud of no points
        with pytest.raises(ValueError):
            anchor.decompress(bad, "cpu")
    with pytest.raises(ValueError):
        anchor.to_coded(np.zeros((1, 3)), "xyz")


@pytest.mark.parametrize("name", sorted(ref.anchor_cases()))
def test_anchor_cases_have_no_coefficient_near_a_rounding_boundary(name):
    """tests/test_anchor.py compares the encoder's symbols with numpy's rint and excludes coefficients that a GPU value within the
    coefficient tolerance could round to the other side: the cases are chosen so that there is none to exclude"""
    x, qstep, _ = ref.anchor_cases()[name]
    _, _, co, tol, _ = ref.anchor_reference(name)
    assert int(ref.near_rounding_boundary(co, qstep, tol).sum()) == 0
