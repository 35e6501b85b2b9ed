"""The lane-parallel y stream "PCL1" on the GPU: csrc/rans_lanes.hip against its host twin (which tests/test_rans_lanes_host.py
holds to the oracle's coder byte for byte), and the format through the model: same reconstruction, same z string, same
structure as the reference-format round trip of the same frame."""
import threading

import numpy as np
import pytest
import torch

from test_rans_lanes_host import CASES, case_sequence, tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gc(pcc):
    """a Gaussian conditional that codes with the tables of the host tests"""
    from pcc_amd import entropy as pe
    g = pe.GaussianConditional(None).to(DEV)
    g._set_tables(*tables())
    return g


def gpu_encode(gc, sym, idx, lanes):
    s = torch.from_numpy(sym).to(DEV).reshape(1, -1)
    i = torch.from_numpy(idx).to(DEV).reshape(1, -1)
    return gc._lanes_encode_begin(s, i, lanes)()[0]


def gpu_decode(gc, data, idx):
    sym, status = gc._lanes_decode(data, torch.from_numpy(idx).to(DEV))
    return sym.cpu().numpy(), int(status.item())


def both_ways(pcc, gc, sym, idx, lanes):
    from pcc_amd import entropy as pe
    cdf, cdf_length, offset = tables()
    host = pe._rans_lanes_encode_host(sym, idx, lanes, cdf, cdf_length, offset)
    ours = gpu_encode(gc, sym, idx, lanes)
    assert ours == host
    for data in (host, ours):
        back, status = gpu_decode(gc, data, idx)
        assert status == 0 and np.array_equal(back, sym)
    assert np.array_equal(pe._rans_lanes_decode_host(ours, idx, cdf, cdf_length, offset), sym)


@pytest.mark.parametrize("case", CASES + ["every"], ids=lambda c: c if isinstance(c, str) else "n%d-P%d-s%g" % c)
def test_kernels_equal_the_host_twin(pcc, gc, case):
    sym, idx, lanes = case_sequence(case)
    both_ways(pcc, gc, sym, idx, lanes)


@pytest.mark.parametrize("lanes", [1, 257, 4096])
def test_lane_counts_at_the_ends_of_the_range(pcc, gc, lanes):
    """one lane, a partial last wave in a second workgroup, and the largest count (16 workgroups, most lanes with 4 or 5 symbols)"""
    sym, idx, _ = case_sequence((20000, 256, .25))
    both_ways(pcc, gc, sym, idx, lanes)


def test_symbols_that_cost_more_than_a_word_take_the_capacity_retry(pcc, gc):
    from pcc_amd import entropy as pe
    sym, idx, lanes = case_sequence("huge")
    before = pe.LANES_RETRIES
    both_ways(pcc, gc, sym, idx, lanes)
    assert pe.LANES_RETRIES == before + 1


def test_a_symbol_beyond_int16_round_trips(pcc, gc):
    sym, idx, lanes = case_sequence((1000, 100, .3))
    sym = sym.copy()
    sym[sym.size // 2] = 40000
    both_ways(pcc, gc, sym, idx, lanes)


def test_header_faults_raise_before_a_launch(pcc, gc):
    """(only valid and header-invalid streams reach the GPU decoder: corrupt payloads are the host twin's tests)"""
    import struct
    from pcc_amd import entropy as pe
    cdf, cdf_length, offset = tables()
    sym, idx, lanes = case_sequence((1000, 100, .3))
    good = pe._rans_lanes_encode_host(sym, idx, lanes, cdf, cdf_length, offset)
    (len0,) = struct.unpack_from("<I", good, 8)
    bad_length = bytearray(good)
    struct.pack_into("<I", bad_length, 8, len0 + 2)
    idx_dev = torch.from_numpy(idx).to(DEV)
    torch.cuda.synchronize()
    for data in (b"PCL2" + good[4:], good[:4] + struct.pack("<H", 0) + good[6:], good[:4] + struct.pack("<H", 4097) + good[6:],
                 bytes(bad_length), good[:-4], good[:20], b""):
        with pytest.raises((ValueError, RuntimeError)):
            gc._lanes_decode(data, idx_dev)
    with pytest.raises(RuntimeError):                   # the right header for another symbol count
        gc._lanes_decode(good, idx_dev[:50])
    back, status = gpu_decode(gc, good, idx)
    assert status == 0 and np.array_equal(back, sym)


# ---- through the model ----------------------------------------------------------------------------------------------------

def _frame(pcc, cfg):
    pts = pcc.synthetic.sphere_shell(**cfg)
    qc, qf = pcc.synthetic.uniform_qmap(pts[:, :3], 0.5, 0.5)
    return pts, qc, qf


def _compress(pcc, model, pts, qc, qf, **kw):
    x = torch.from_numpy(pts).to(DEV)
    Q = pcc.SparseTensor(coordinates=torch.from_numpy(qc).to(DEV), features=torch.from_numpy(qf).to(DEV), device=DEV)
    return model.compress(x, Q, **kw)


def _canonical(rec):
    r = rec.cpu().numpy()
    return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]


@pytest.fixture(scope="module")
def model(pcc):
    m = pcc.synthetic.make_model(0, DEV)
    m.update()
    return m


@pytest.fixture(scope="module")
def two_hyperprior_model(pcc):
    m = pcc.synthetic.make_model(0, DEV, config=pcc.synthetic.TWO_HYPERPRIOR_CONFIG)
    m.update()
    return m



@pytest.mark.parametrize("name,lanes", [("config1", 64), ("shell128", 256)])
def test_model_round_trip_equals_the_reference_format_round_trip(pcc, model, tmp_path, monkeypatch, name, lanes):
    from pcc_amd import entropy as pe
    cfg = pcc.synthetic.CONFIG1 if name == "config1" else dict(grid=128, radius=50, half_width=0.5)
    pts, qc, qf = _frame(pcc, cfg)
    assert name != "config1" or pts.shape[0] == 4904
    assert pe.STREAM_LANES == 0
    r_strings, r_shape, r_k, r_coords = _compress(pcc, model, pts, qc, qf)
    r_rec = model.decompress(coordinates=r_coords, strings=r_strings, shape=r_shape, k=r_k)
    seen = {}
    inner = pe.GaussianConditional._lanes_encode_begin

    def spy(self, sym, idx, n_lanes):
        seen["idx"] = idx.reshape(-1).cpu().numpy()
        return inner(self, sym, idx, n_lanes)

    monkeypatch.setattr(pe.GaussianConditional, "_lanes_encode_begin", spy)
    pe.set_stream_lanes(lanes)
    try:
        strings, shape, k, coords = _compress(pcc, model, pts, qc, qf)
        rec = model.decompress(coordinates=coords, strings=strings, shape=shape, k=k)
        assert torch.equal(rec, r_rec)
        assert shape == r_shape and k == r_k and torch.equal(coords, r_coords)
        assert strings[1][0] == r_strings[1][0]                                       # the z string: the reference's format
        y = strings[0][0]
        assert y[:4] == b"PCL1" and int.from_bytes(y[4:6], "little") == lanes
        # the y string is the host twin's container of the symbols the reference-format y string holds
        cdf, cdf_length, offset = model.entropy_model.gaussian_conditional.tables()
        ref_symbols = pe._rans_decode(r_strings[0][0], seen["idx"], cdf, cdf_length, offset)
        assert y == pe._rans_lanes_encode_host(ref_symbols, seen["idx"], lanes, cdf, cdf_length, offset)
        # file mode
        path = str(tmp_path / "lanes.bin")
        assert _compress(pcc, model, pts, qc, qf, path=path) is None
        assert np.array_equal(_canonical(model.decompress(path=path)), _canonical(r_rec))
        # a reference-format y string in lanes mode
        with pytest.raises(ValueError, match="PCC_STREAM_LANES"):
            model.decompress(coordinates=r_coords, strings=r_strings, shape=r_shape, k=r_k)
    finally:
        pe.set_stream_lanes(0)
    again = model.decompress(coordinates=r_coords, strings=r_strings, shape=r_shape, k=r_k)          # the default is back
    assert torch.equal(again, r_rec)


def test_blocks_round_trip_in_lanes_mode(pcc, model):
    from pcc_amd import entropy as pe
    from pcc_amd import parallel as par
    pts, qc, qf = _frame(pcc, dict(grid=64, radius=27.0, half_width=0.6))
    x, q = torch.from_numpy(pts).to(DEV), torch.from_numpy(qf).to(DEV)
    _, _, r_units = par.compress_blocks(model, x, q, 32)
    r_rec = par.decompress_blocks(model, r_units)
    pe.set_stream_lanes(64)
    try:
        _, _, units = par.compress_blocks(model, x, q, 32)
        assert all(u[1][0][0][:4] == b"PCL1" and u[1][1][0] == r[1][1][0] for u, r in zip(units, r_units))
        rec = par.decompress_blocks(model, units)
    finally:
        pe.set_stream_lanes(0)
    assert torch.equal(rec, r_rec)


def test_two_hyperprior_model_in_lanes_mode(pcc, two_hyperprior_model):
    from pcc_amd import entropy as pe
    m = two_hyperprior_model
    pts, qc, qf = _frame(pcc, pcc.synthetic.CONFIG1)
    r_strings, r_shape, r_k, r_coords = _compress(pcc, m, pts, qc, qf)
    r_rec = m.decompress(coordinates=r_coords, strings=r_strings, shape=r_shape, k=r_k)
    pe.set_stream_lanes(64)
    try:
        strings, shape, k, coords = _compress(pcc, m, pts, qc, qf)
        rec = m.decompress(coordinates=coords, strings=strings, shape=shape, k=k)
    finally:
        pe.set_stream_lanes(0)
    assert torch.equal(rec, r_rec) and shape == r_shape and k == r_k and torch.equal(coords, r_coords)
    for pair, r_pair in zip(strings, r_strings):                  # two (y, z) pairs: both y strings in lanes, both z strings unchanged
        assert pair[0][0][:4] == b"PCL1" and r_pair[0][0][:4] != b"PCL1" and pair[1][0] == r_pair[1][0]


def test_two_coding_threads_produce_identical_frames(pcc, model):
    from pcc_amd import entropy as pe
    pts, qc, qf = _frame(pcc, pcc.synthetic.CONFIG1)
    out, errors = {}, []

    def code(i):
        try:
            torch.cuda.set_device(DEV)
            with torch.cuda.stream(torch.cuda.Stream(DEV)):
                for _ in range(3):
                    strings, shape, k, coords = _compress(pcc, model, pts, qc, qf)
                    rec = model.decompress(coordinates=coords, strings=strings, shape=shape, k=k)
                out[i] = (strings, rec.cpu())
        except BaseException as e:
            errors.append(e)

    pe.set_stream_lanes(64)
    try:
        want_strings, shape, k, coords = _compress(pcc, model, pts, qc, qf)
        want = model.decompress(coordinates=coords, strings=want_strings, shape=shape, k=k).cpu()
        threads = [threading.Thread(target=code, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        pe.set_stream_lanes(0)
    assert not errors, errors
    for i in range(2):
        assert out[i][0] == want_strings and torch.equal(out[i][1], want)
