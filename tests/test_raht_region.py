"""Region-wise quantisation of the RAHT coefficients on the GPU (csrc/raht.hip: pcc_raht_blocks, pcc_raht_block_levels,
pcc_raht_coeff_levels, pcc_raht_quantize, pcc_raht_dequantize; the PCR2 stream of pcc_amd.raht) against the numpy restatement
tests/_raht_region_reference.py, which finds the blocks from the keys and the coefficient levels as range minima.  Everything
here is integer work or a single correctly rounded float64 operation, so every comparison is for EQUALITY: the symbols are held
against np.rint of the kernel's OWN coefficients, which leaves no rounding boundary to allow for.  Clouds: those of
tests/_raht_reference.py without the second one-point cloud (dense512 / dense514 put a first folded step of exactly 256 and of 257
rows under the level walk); block sizes 0, 1, 3, the depth and 17; level maps flat 0, flat 63, random and two halves."""
import functools
import struct

import numpy as np
import pytest
import torch

import _raht_reference as ref
import _raht_region_reference as reg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7
CASES = ["one", "siblings", "meet_at_top", "cube", "random92", "shell32", "random4000", "deep300", "dense512", "dense514"]
QSTEP = 4 / 255


@functools.lru_cache(maxsize=None)
def setup(name):
    """-> (coords, the restatement's plan, the package's plan)"""
    from pcc_amd import raht
    coords, origin, depth = ref.cases()[name]
    want = ref.plan(coords, origin, depth)
    p = raht.plan(torch.from_numpy(coords).to(DEV), origin=origin, depth=depth)
    for k in ("perm", "step", "left", "w1"):
        assert np.array_equal(getattr(p, k).cpu().numpy(), want[k]), k
    return coords, want, p


@functools.lru_cache(maxsize=None)
def reference_levels(name, b, key):
    """-> (block_of_row, n_blocks, block levels, coefficient levels) of the restatement"""
    coords, want, _ = setup(name)
    block_of_row, n_blocks = reg.blocks_from_keys(want, b)
    bl = reg.block_levels(want, reg.level_maps(coords)[key], block_of_row, n_blocks)
    return block_of_row, n_blocks, bl, reg.coeff_levels_range_min(want, bl, block_of_row)


def run_levels(p, levels, b):
    """the three level entry points through the C ABI, every output pre-filled with a sentinel and longer than needed ->
    (block_of_row, n_blocks, block_level, coeff_level) as numpy arrays"""
    from pcc_amd._lib import check, lib, ptr, stream
    L, n = lib(), p.n
    block_of_row = torch.full((n + 3,), SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
    nbytes = L.pcc_raht_scratch_bytes(n)
    scratch = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    check(L.pcc_raht_blocks(ptr(p.step), n, b, ptr(block_of_row), ptr(count), ptr(scratch), nbytes, stream()))
    n_blocks = int(count[0])
    assert bool((block_of_row[n:] == SENTINEL).all()) and bool((count[1:] == SENTINEL).all())
    block_level = torch.full((n_blocks + 3,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
    lv = torch.from_numpy(levels).to(DEV)
    check(L.pcc_raht_block_levels(ptr(lv), ptr(p.perm), ptr(block_of_row), n, n_blocks, ptr(block_level), ptr(status), stream()))
    assert status.tolist() == [0] + [SENTINEL] * 3 and bool((block_level[n_blocks:] == SENTINEL).all())
    coeff_level = torch.full((n + 5,), 200, dtype=torch.uint8, device=DEV)
    lev = torch.full((n + 3,), SENTINEL, dtype=torch.int32, device=DEV)
    check(L.pcc_raht_coeff_levels(ptr(block_level), ptr(block_of_row), n, n_blocks, ptr(p.left), ptr(p.step_rows), ptr(p.step_offsets), p.depth,
                                  ptr(coeff_level), ptr(lev), stream()))
    torch.cuda.synchronize()
    assert bool((coeff_level[n:] == 200).all()) and bool((lev[n:] == SENTINEL).all())
    return block_of_row[:n].cpu().numpy(), n_blocks, block_level[:n_blocks].cpu().numpy(), coeff_level[:n].cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_blocks_and_levels_equal_numpy(pcc, name):
    coords, want, p = setup(name)
    for b in reg.block_sizes(want["depth"]):
        for key, levels in reg.level_maps(coords).items():
            w_rows, w_n, w_bl, w_cl = reference_levels(name, b, key)
            rows, n_blocks, bl, cl = run_levels(p, levels, b)
            assert n_blocks == w_n and rows.dtype == np.int32 and np.array_equal(rows, w_rows), (b, key)
            assert bl.dtype == np.int32 and np.array_equal(bl, w_bl), (b, key)
            assert cl.dtype == np.uint8 and np.array_equal(cl, w_cl), (b, key)
    # a coefficient-level output that starts at an odd address takes the byte stores: the same levels
    from pcc_amd._lib import check, ptr, stream
    from pcc_amd import raht
    block_of_row, n_blocks = raht.blocks(p, 1)
    bl = raht.block_levels(p, reg.level_maps(coords)["random"], block_of_row, n_blocks)
    odd = torch.full((p.n + 9,), 200, dtype=torch.uint8, device=DEV)
    lev = torch.empty(p.n, dtype=torch.int32, device=DEV)
    check(pcc.lib().pcc_raht_coeff_levels(ptr(bl), ptr(block_of_row), p.n, n_blocks, ptr(p.left), ptr(p.step_rows), ptr(p.step_offsets), p.depth,
                                          ptr(odd[1:]), ptr(lev), stream()))
    assert np.array_equal(odd[1:p.n + 1].cpu().numpy(), reference_levels(name, 1, "random")[3])
    assert int(odd[0]) == 200 and bool((odd[p.n + 1:] == 200).all())
    assert np.array_equal(raht.coeff_levels(p, bl, block_of_row).cpu().numpy(), reference_levels(name, 1, "random")[3])


@pytest.mark.parametrize("c", (1, 3, 16))
@pytest.mark.parametrize("name", CASES)
def test_quantiser_equals_numpy_on_the_kernels_own_coefficients(pcc, name, c):
    from pcc_amd import raht
    from pcc_amd._lib import check, ptr, stream
    coords, want, p = setup(name)
    n = p.n
    a = ref.attributes(n, c, seed=40 + c) * 2.0 - 0.5
    co = raht.forward(p, a)
    co_host = co.cpu().numpy()
    for qstep, key, b in ((QSTEP, "random", 1), (0.25 / 255, "halves", 3)):
        steps = raht.level_steps(qstep)
        cl = reference_levels(name, min(b, 17), key)[3]
        CL = torch.from_numpy(cl).to(DEV)
        sym = torch.full((n + 2, c), SENTINEL, dtype=torch.int32, device=DEV)
        status = torch.full((3,), SENTINEL, dtype=torch.int32, device=DEV)
        check(pcc.lib().pcc_raht_quantize(ptr(co), n, c, ptr(CL), ptr(steps), ptr(sym), ptr(status), stream()))
        assert status.tolist() == [0, SENTINEL, SENTINEL] and bool((sym[n:] == SENTINEL).all())
        got = sym[:n].cpu().numpy()
        assert np.array_equal(got, reg.quantize(co_host, cl, steps)), (key, b)
        out = torch.full((n + 2, c), float(SENTINEL), dtype=torch.float64, device=DEV)
        check(pcc.lib().pcc_raht_dequantize(ptr(sym), n, c, ptr(CL), ptr(steps), ptr(out), stream()))
        assert bool((out[n:] == float(SENTINEL)).all())
        assert np.array_equal(out[:n].cpu().numpy().view(np.uint64), reg.dequantize(got, cl, steps).view(np.uint64)), (key, b)
        # the Python layer: the same symbols and values
        assert np.array_equal(raht.quantize_levels(co, CL, steps).cpu().numpy(), got)
        assert torch.equal(raht.dequantize_levels(sym[:n], CL, steps), out[:n])
    # ties go to even: coefficients at k + 1/2 steps of their level (steps[0] = 1 exactly, halves of it are exact)
    ties = torch.tensor([[0.5], [1.5], [2.5], [-0.5], [-1.5], [-2.5], [0.49999], [7.3]], dtype=torch.float64, device=DEV)
    zero = torch.zeros(8, dtype=torch.uint8, device=DEV)
    assert raht.quantize_levels(ties, zero, raht.level_steps(1.0)).reshape(-1).tolist() == [0, 2, 2, 0, -2, -2, 0, 7]


@pytest.mark.parametrize("name", CASES)
def test_flat_level_zero_is_pcr1(pcc, name):
    """all points at level 0: the symbols, the payload bytes and the decoded attributes of PCR1 (level 0 is qstep itself and a
    shift of zero chooses the same tables)"""
    from pcc_amd import raht
    coords, want, p = setup(name)
    a = ref.smooth_colours(coords)
    for b in (0, 3):
        data1, sym1 = raht.encode_attributes(p, a, QSTEP, return_symbols=True)
        data2, sym2 = raht.encode_attributes(p, a, QSTEP, return_symbols=True, levels=np.zeros(p.n, dtype=np.uint8), block_log2=b)
        assert data1[:4] == b"PCR1" and data2[:4] == b"PCR2"
        assert sym2.dtype == np.int64 and np.array_equal(sym1, sym2)
        f = reg.parse(data2)
        nt = 9 * want["depth"]                               # PCR1: 20 bytes of head | dc | tables | payload_len | payload
        dc1, tables1, payload1 = data1[20:44], data1[44:44 + nt], data1[48 + nt:]
        assert struct.unpack("<I", data1[44 + nt:48 + nt])[0] == len(payload1)
        assert f["payload"] == payload1 and f["table"].tobytes() == tables1 and f["dc"].tolist() == list(struct.unpack("<3q", dc1))
        assert f["n_blocks"] == reg.blocks_from_keys(want, b)[1] and f["block_log2"] == b and f["qstep"] == QSTEP
        rec1, rec2 = raht.decode_attributes(p, data1), raht.decode_attributes(p, data2)
        assert torch.equal(rec1, rec2)


@pytest.mark.parametrize("key", ("random", "halves", "flat63"))
@pytest.mark.parametrize("name", CASES)
def test_stream_round_trip(pcc, name, key):
    from pcc_amd import raht
    from pcc_amd.entropy import _rans_encode
    coords, want, p = setup(name)
    n = p.n
    a = ref.smooth_colours(coords)
    levels = reg.level_maps(coords)[key]
    b = 1
    _, n_blocks, bl, cl = reference_levels(name, b, key)
    data, sym = raht.encode_attributes(p, a, QSTEP, return_symbols=True, levels=levels, block_log2=b)
    # two runs: the same bytes (and a tensor of levels is an array of levels)
    assert raht.encode_attributes(p, a, QSTEP, levels=torch.from_numpy(levels).to(DEV), block_log2=b) == data
    steps = reg.level_steps(QSTEP)
    assert np.array_equal(sym, reg.quantize(raht.forward(p, a).cpu().numpy(), cl, steps))
    back, qstep, region = raht.decode_region(p, data)
    assert qstep == QSTEP and back.dtype == np.int64 and np.array_equal(back, sym)
    # the decoder's levels, rebuilt from the plan and the stream, are the encoder's
    assert region.n_blocks == n_blocks and region.block_log2 == b
    assert np.array_equal(region.block_level.cpu().numpy(), bl) and np.array_equal(region.coeff_level.cpu().numpy(), cl)
    enc = raht.region(p, levels, b)
    assert torch.equal(enc.coeff_level, region.coeff_level) and torch.equal(enc.block_of_row, region.block_of_row)
    # the reconstruction against the numpy inverse of symbols x steps, within the transform's bound
    rec = raht.decode_attributes(p, data, channels=3).cpu().numpy()
    coeffs = reg.dequantize(sym, cl, steps)
    tol = 1e-12 * np.abs(a).max() * np.sqrt(n)
    err = np.abs(rec - ref.inverse(want, coeffs)).max()
    print(f"{name} {key}: {len(data)} bytes, {n_blocks} blocks, inverse max error {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    with pytest.raises(ValueError):
        raht.decode_attributes(p, data, channels=1)
    # the whole stream is the restatement's assembly (symbol-by-symbol table choice): on the clouds small enough for it
    if n <= 100:
        assert data == reg.assemble(want, sym, QSTEP, b, bl, cl, raht.gaussian_tables(), _rans_encode)
    # a stream cut inside its payload, and one whose block count is not the geometry's
    if n > 1:
        with pytest.raises(ValueError):
            raht.decode_attributes(p, data[:-1])
        wrong = bytearray(data)
        wrong[20:24] = struct.pack("<I", n_blocks + 1)
        with pytest.raises(ValueError):
            raht.decode_attributes(p, bytes(wrong))


@pytest.mark.parametrize("b", (0, 1, 3))
@pytest.mark.parametrize("name", ("shell32", "random4000", "dense514", "deep300", "random92"))
def test_rows_of_the_finest_blocks_decode_as_uniform(pcc, name, b):
    from pcc_amd import raht
    coords, want, p = setup(name)
    a = ref.attributes(p.n, 3, seed=13)
    for key in ("halves", "random"):
        levels = reg.level_maps(coords)[key]
        block_of_row, _, bl, _ = reference_levels(name, b, key)
        finest = int(bl.min())
        rec = raht.decode_attributes(p, raht.encode_attributes(p, a, QSTEP, levels=levels, block_log2=b)).cpu().numpy()
        flat = np.full(p.n, finest, dtype=np.uint8)
        uniform = raht.decode_attributes(p, raht.encode_attributes(p, a, QSTEP, levels=flat, block_log2=b)).cpu().numpy()
        rows = bl[block_of_row] == finest
        assert rows.any() and np.array_equal(rec[rows].view(np.uint64), uniform[rows].view(np.uint64)), key
        if name in ("shell32", "random4000"):
            assert not rows.all() and not np.array_equal(rec[~rows], uniform[~rows]), key


def test_argument_errors(pcc):
    from pcc_amd import raht
    from pcc_amd._lib import PCC, ptr, stream
    L = pcc.lib()
    coords, want, p = setup("cube")
    n = 8
    block_of_row, n_blocks = raht.blocks(p, 0)
    rows = torch.zeros(n, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbytes = L.pcc_raht_scratch_bytes(n)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    for b in (-1, 18):
        assert L.pcc_raht_blocks(ptr(p.step), n, b, ptr(rows), ptr(count), ptr(scratch), nbytes, stream()) == PCC.ERR_ARG
        assert b"block_log2" in L.pcc_last_error()
    assert L.pcc_raht_blocks(ptr(p.step), 0, 1, ptr(rows), ptr(count), ptr(scratch), nbytes, stream()) == PCC.ERR_ARG
    assert L.pcc_raht_blocks(None, n, 1, ptr(rows), ptr(count), ptr(scratch), nbytes, stream()) == PCC.ERR_ARG
    assert L.pcc_raht_blocks(ptr(p.step), n, 1, ptr(rows), None, ptr(scratch), nbytes, stream()) == PCC.ERR_ARG
    assert L.pcc_raht_blocks(ptr(p.step), n, 1, ptr(rows), ptr(count), ptr(scratch), nbytes - 1, stream()) == PCC.ERR_ARG
    assert bool((rows == 0).all()) and int(count) == 0
    levels = torch.zeros(n, dtype=torch.uint8, device=DEV)
    bl = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    args = lambda lv=levels, nb=n_blocks, out=bl, rows_n=n: (ptr(lv) if lv is not None else None, ptr(p.perm), ptr(block_of_row), rows_n, nb,
                                                            ptr(out) if out is not None else None, ptr(status), stream())
    for bad in (args(lv=None), args(out=None), args(nb=0), args(nb=n + 1), args(rows_n=0)):
        assert L.pcc_raht_block_levels(*bad) == PCC.ERR_ARG
    assert bool((bl == SENTINEL).all()) and int(status) == SENTINEL
    cl = torch.full((n,), 200, dtype=torch.uint8, device=DEV)
    lev = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    good_bl = raht.block_levels(p, levels, block_of_row, n_blocks)
    walk = lambda offsets=p.step_offsets, depth=p.depth, nb=n_blocks, out=cl: (ptr(good_bl), ptr(block_of_row), n, nb, ptr(p.left), ptr(p.step_rows),
                                                                             ptr(offsets), depth, ptr(out) if out is not None else None, ptr(lev), stream())
    for bad in (walk(offsets=np.array([0, 4, 3, 7], dtype=np.int32)), walk(offsets=np.array([0, 4, 6, 9], dtype=np.int32)),
                walk(offsets=np.array([1, 4, 6, 7], dtype=np.int32)), walk(depth=18), walk(depth=-1), walk(nb=0), walk(nb=n + 1), walk(out=None)):
        assert L.pcc_raht_coeff_levels(*bad) == PCC.ERR_ARG
    assert bool((cl == 200).all()) and bool((lev == SENTINEL).all())
    co = torch.zeros((n, 17), dtype=torch.float64, device=DEV)
    sym = torch.full((n, 17), SENTINEL, dtype=torch.int32, device=DEV)
    steps = raht.level_steps(1.0)
    zero = torch.zeros(n, dtype=torch.uint8, device=DEV)
    for c in (0, 17):
        assert L.pcc_raht_quantize(ptr(co), n, c, ptr(zero), ptr(steps), ptr(sym), ptr(status), stream()) == PCC.ERR_ARG
        assert b"channels" in L.pcc_last_error()
        assert L.pcc_raht_dequantize(ptr(sym), n, c, ptr(zero), ptr(steps), ptr(co), stream()) == PCC.ERR_ARG
    for bad_steps in (None, np.where(np.arange(64) == 9, 0.0, steps), np.where(np.arange(64) == 63, np.inf, steps)):
        assert L.pcc_raht_quantize(ptr(co), n, 3, ptr(zero), ptr(bad_steps), ptr(sym), ptr(status), stream()) == PCC.ERR_ARG
        assert L.pcc_raht_dequantize(ptr(sym), n, 3, ptr(zero), ptr(bad_steps), ptr(co), stream()) == PCC.ERR_ARG
    assert L.pcc_raht_quantize(ptr(co), n, 3, None, ptr(steps), ptr(sym), ptr(status), stream()) == PCC.ERR_ARG
    assert L.pcc_raht_dequantize(None, n, 3, ptr(zero), ptr(steps), ptr(co), stream()) == PCC.ERR_ARG
    torch.cuda.synchronize()
    assert bool((sym == SENTINEL).all()) and bool((co == 0).all()) and int(status) == SENTINEL


def test_python_layer_refuses_bad_levels_and_symbols(pcc):
    from pcc_amd import raht
    coords, want, p = setup("shell32")
    a = ref.smooth_colours(coords)
    levels = reg.level_maps(coords)["random"]
    for bad in (np.where(np.arange(p.n) == 77, 64, levels).astype(np.uint8), np.where(np.arange(p.n) == 5, 255, levels).astype(np.uint8),
                np.where(np.arange(p.n) == 5, -1, levels.astype(np.int64)), np.where(np.arange(p.n) == 5, 300, levels.astype(np.int64)),
                levels[:-1], levels.astype(np.float64)):
        with pytest.raises(ValueError):
            raht.encode_attributes(p, a, QSTEP, levels=bad)
    for b in (-1, 18):
        with pytest.raises(ValueError):
            raht.encode_attributes(p, a, QSTEP, levels=levels, block_log2=b)
    with pytest.raises(ValueError):
        raht.encode_attributes(p, a, 0.0, levels=levels)
    # the status word of the block levels counts every level above 63
    from pcc_amd._lib import check, ptr, stream
    block_of_row, n_blocks = raht.blocks(p, 3)
    lv = torch.from_numpy(np.where(np.arange(p.n) % 100 == 0, 64 + np.arange(p.n) % 190, levels).astype(np.uint8)).to(DEV)
    out = torch.empty(n_blocks, dtype=torch.int32, device=DEV)
    status = torch.empty(1, dtype=torch.int32, device=DEV)
    check(pcc.lib().pcc_raht_block_levels(ptr(lv), ptr(p.perm), ptr(block_of_row), p.n, n_blocks, ptr(out), ptr(status), stream()))
    assert int(status) == len(range(0, p.n, 100)) and int(out.max()) <= 63
    # symbols of 2^28 and more are counted, not written
    co = torch.tensor([[1.0, 2.0 ** 28, -(2.0 ** 28)], [2.0 ** 28 - 1, float("nan"), 3.0]], dtype=torch.float64, device=DEV)
    sym = torch.empty((2, 3), dtype=torch.int32, device=DEV)
    zero = torch.zeros(2, dtype=torch.uint8, device=DEV)
    check(pcc.lib().pcc_raht_quantize(ptr(co), 2, 3, ptr(zero), ptr(raht.level_steps(1.0)), ptr(sym), ptr(status), stream()))
    assert int(status) == 3 and sym.tolist() == [[1, 0, 0], [2 ** 28 - 1, 0, 3]]
    with pytest.raises(ValueError):
        raht.quantize_levels(co, zero, raht.level_steps(1.0))
    with pytest.raises(ValueError):
        raht.encode_attributes(p, a, 1e-12, levels=levels)
