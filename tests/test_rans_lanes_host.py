"""The lane-parallel y stream "PCL1" on the host (no GPU needed): the product's host twin of the GPU coder against a
container assembled HERE from the oracle's reference-format coder.

Format: the symbol sequence is dealt to P lanes, lane s owns positions s, s + P, ...; lane s's substream
is exactly what the reference-format coder writes for sym[s::P], idx[s::P] alone; a lane without symbols has length 0.
Container, little-endian: b"PCL1", P (uint16), 0 (uint16), P x uint32 byte lengths, the substreams in lane order."""
import struct

import numpy as np
import pytest

from oracle import rans as orans
from test_rans_host import _draw, _tables

_MEMO = {}


def tables():
    if "t" not in _MEMO:
        _MEMO["t"] = _tables()
    return _MEMO["t"]


def _oracle_encode_py(sym, idx, cdf, cdf_length, offset):
    """oracle/rans_py.py, the oracle coder's Python statement ("must agree with rans.c byte for byte"), on Python integers"""
    from oracle import rans_py
    return bytes(rans_py.encode_with_indexes(sym.tolist(), idx.tolist(), cdf.tolist(), cdf_length.tolist(), offset.tolist()))


def expected_container(sym, idx, lanes, cdf, cdf_length, offset, encode=orans.encode_with_indexes):
    """-> (container bytes, [substream per lane]) from the oracle's coder on each lane's subsequence"""
    subs = [encode(sym[s::lanes], idx[s::lanes], cdf, cdf_length, offset) if s < sym.size else b"" for s in range(lanes)]
    head = b"PCL1" + struct.pack("<HH", lanes, 0) + b"".join(struct.pack("<I", len(b)) for b in subs)
    return head + b"".join(subs), subs


def every_table_every_symbol(cdf_length, offset):
    """the sequence of tests/test_rans_host.py::test_every_table_every_symbol"""
    sym, idx = [], []
    for t in range(cdf_length.size):
        maxv = cdf_length[t] - 2
        vals = np.arange(-3, maxv + 3) + offset[t]
        sym.append(vals)
        idx.append(np.full(vals.size, t))
    return np.concatenate(sym).astype(np.int32), np.concatenate(idx).astype(np.int32)


def huge_symbols():
    """4096 symbols of value 2^30 on table 0: each costs more than one 32-bit word"""
    return np.full(4096, 1 << 30, dtype=np.int32), np.zeros(4096, dtype=np.int32)


CASES = [(1, 64, .3), (63, 64, .3), (64, 64, .3), (65, 64, .3), (1000, 100, .3), (4099, 1, .3), (20000, 256, .25), (20000, 256, 1.5)]


def case_sequence(case):
    """(n, P, spread) | "every" | "huge" -> (sym, idx, P)"""
    cdf, cdf_length, offset = tables()
    if case == "every":
        return (*every_table_every_symbol(cdf_length, offset), 128)
    if case == "huge":
        return (*huge_symbols(), 64)
    n, lanes, spread = case
    sym, idx = _draw(np.random.default_rng(n * 7 + lanes), n, cdf_length, offset, spread)
    return sym, idx, lanes


def check_against_oracle(pe, sym, idx, lanes, encode=orans.encode_with_indexes):
    cdf, cdf_length, offset = tables()
    want, subs = expected_container(sym, idx, lanes, cdf, cdf_length, offset, encode)
    ours = pe._rans_lanes_encode_host(sym, idx, lanes, cdf, cdf_length, offset)
    assert ours == want
    assert np.array_equal(pe._rans_lanes_decode_host(ours, idx, cdf, cdf_length, offset), sym)
    # the oracle's decoder on each sliced substream of OUR container
    at = 8 + 4 * lanes
    for s in range(lanes):
        (length,) = struct.unpack_from("<I", ours, 8 + 4 * s)
        assert length == len(subs[s])
        if length:
            back = np.asarray(orans.decode_with_indexes(ours[at:at + length], idx[s::lanes], cdf, cdf_length, offset))
            assert np.array_equal(back, sym[s::lanes])
        at += length
    assert at == len(ours)
    return ours


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-P%d-s%g" % c)
def test_host_twin_equals_the_oracle_per_lane(pcc, case):
    from pcc_amd import entropy as pe
    sym, idx, lanes = case_sequence(case)
    ours = check_against_oracle(pe, sym, idx, lanes)
    if lanes == 1:              # the 12-byte header plus the reference stream
        cdf, cdf_length, offset = tables()
        assert ours[12:] == orans.encode_with_indexes(sym, idx, cdf, cdf_length, offset) and len(ours[:12]) == 12


def test_every_table_every_symbol_in_lanes(pcc):
    from pcc_amd import entropy as pe
    sym, idx, lanes = case_sequence("every")
    check_against_oracle(pe, sym, idx, lanes)


def test_symbols_that_cost_more_than_a_word(pcc):
    """The expected substreams of THIS case come from the oracle's Python statement of the coder (oracle/rans_py.py), not from
    oracle/rans.c: the C oracle counts an escape's nibbles with a 32-bit shift, which is undefined from 8 nibbles on
    (raw >= 2^28, i.e. a symbol 2^27 past its table), and its build does not come back from this sequence.  The two files
    state the same coder, and every other case here uses the C one.  The oracle's C DECODER reads these streams."""
    from pcc_amd import entropy as pe
    sym, idx, lanes = case_sequence("huge")
    ours = check_against_oracle(pe, sym, idx, lanes, encode=_oracle_encode_py)
    assert len(ours) > 4 * sym.size


def test_malformed_containers_are_reported_not_crashed(pcc):
    from pcc_amd import entropy as pe
    cdf, cdf_length, offset = tables()
    sym, idx, lanes = case_sequence((1000, 100, .3))
    good = pe._rans_lanes_encode_host(sym, idx, lanes, cdf, cdf_length, offset)
    L = pcc.lib()

    def refused(data, indexes=idx):
        with pytest.raises(RuntimeError):
            pe._rans_lanes_decode_host(bytes(data), indexes, cdf, cdf_length, offset)
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        assert L.pcc_rans_lanes_header(buf.ctypes.data if buf.size else None, buf.size) < 0 or indexes is not idx

    def with_length(s, value):
        out = bytearray(good)
        struct.pack_into("<I", out, 8 + 4 * s, value)
        return out

    (len0,) = struct.unpack_from("<I", good, 8)
    refused(b"PCL2" + good[4:])                                                 # wrong magic
    refused(good[:4] + struct.pack("<H", 0) + good[6:])                         # P = 0
    refused(good[:4] + struct.pack("<H", 4097) + good[6:])                      # P = 4097
    refused(with_length(0, len0 + 2))                                           # a length that is no multiple of 4
    refused(with_length(0, 4) + b"")                                            # a length of 4
    refused(with_length(0, len0 + 4))                                           # lengths that do not add up to the buffer
    refused(good[:-4])                                                          # truncated
    refused(good[:20])                                                          # truncated inside the header
    refused(b"")
    # the right header for another symbol count: a lane with bytes and no symbols
    refused(good, indexes=idx[:50])
    assert L.pcc_rans_lanes_header(np.frombuffer(good, dtype=np.uint8).ctypes.data, len(good)) == lanes
    # one payload word flipped: reported through the end-state check, or decoded (to other symbols) with every read inside
    # the lane's substream — the call returns either way
    for at in (8 + 4 * lanes + 8, len(good) - 4, len(good) // 2 // 4 * 4):
        bad = bytearray(good)
        bad[at] ^= 0x5A
        bad[at + 3] ^= 0xC3
        try:
            pe._rans_lanes_decode_host(bytes(bad), idx, cdf, cdf_length, offset)
        except RuntimeError:
            pass


def test_setting_is_validated(pcc):
    from pcc_amd import entropy as pe
    assert pe.STREAM_LANES == 0 or "PCC_STREAM_LANES" in __import__("os").environ
    was = pe.STREAM_LANES
    try:
        pe.set_stream_lanes(64)
        assert pe.STREAM_LANES == 64
        for bad in (-1, 4097):
            with pytest.raises(ValueError):
                pe.set_stream_lanes(bad)
        assert pe.STREAM_LANES == 64
    finally:
        pe.set_stream_lanes(was)
