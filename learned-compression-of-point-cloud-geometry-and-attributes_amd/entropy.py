"""Factorized entropy bottleneck and Gaussian conditional on libpcc_hip.so.

Host-side mirror of ``compressai.entropy_models.EntropyBottleneck`` / ``GaussianConditional``
as the reference uses them (model/entropy_models.py:269-270,313,330,352-353,371-372,393,407-408):
same constructor arguments, parameter / buffer names (so reference state_dicts load), and the
``compress`` / ``decompress`` / ``forward`` / ``update`` / ``loss`` methods.  Quantisation, index
build and likelihoods run as HIP kernels on [N, C] feature matrices; CDF tables are built on the
host at ``update()`` (one-off) and the rANS coder is the host C++ one in the same library
(SURVEY.md N12-N14).  Training mode — additive U(-.5, .5) noise instead of rounding, likelihoods differentiable through torch
ops, compressai's LowerBound gradients — is ``forward(..., training=True)`` / ``module.train()``.
"""
import functools
import math
import os

import numpy as np
import scipy.stats
import torch
import torch.nn as nn

from . import _lib, _threads
from ._lib import check, ptr

SCALES_MIN, SCALES_MAX, SCALES_LEVELS = 0.11, 256.0, 64


def get_scale_table(minimum=SCALES_MIN, maximum=SCALES_MAX, levels=SCALES_LEVELS):
    return torch.exp(torch.linspace(math.log(minimum), math.log(maximum), levels))


class _LowerBoundFn(torch.autograd.Function):
    """max(x, bound) whose gradient also flows where x < bound if it pushes x up (compressai.ops.LowerBound)."""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x, bound)
        return torch.max(x, bound)

    @staticmethod
    def backward(ctx, grad):
        x, bound = ctx.saved_tensors
        keep = (x >= bound) | (grad < 0)
        return keep.to(grad.dtype) * grad, None


class _LowerBound(nn.Module):
    """compressai.ops.LowerBound (same state_dict entry)."""

    def __init__(self, bound):
        super().__init__()
        self.register_buffer("bound", torch.tensor([float(bound)]))

    def forward(self, x):
        return _LowerBoundFn.apply(x, self.bound.to(x.device))


# Training-mode quantisation adds U(-0.5, 0.5) noise (compressai EntropyModel.quantize, mode "noise").  Tests
# replace the source to feed the CPU oracle the same draws: a callable (shape, coords) -> CPU float tensor,
# where coords are the int32 [N, 4] coordinates of the tensor's points (NOISE_ROWS, set by the caller of the
# entropy model) — row order differs between implementations, coordinates do not.
NOISE_SOURCE = None
NOISE_ROWS = None


def _uniform_noise(like):
    if NOISE_SOURCE is not None:
        rows = None if NOISE_ROWS is None else NOISE_ROWS.detach().cpu().numpy()
        return NOISE_SOURCE(tuple(like.shape), rows).to(like.device, like.dtype)
    return torch.empty_like(like).uniform_(-0.5, 0.5)


def _pmf_to_cdf(pmf, tail, pmf_length, max_length):
    """compressai EntropyModel._pmf_to_cdf through the library's pmf_to_quantized_cdf."""
    L = _lib.lib()
    cdf = np.zeros((len(pmf_length), max_length + 2), dtype=np.int32)
    for i in range(len(pmf_length)):
        n = int(pmf_length[i])
        prob = np.ascontiguousarray(np.concatenate([pmf[i, :n], tail[i].reshape(-1)]).astype(np.float32))
        row = np.zeros(n + 2, dtype=np.int32)
        check(L.pcc_pmf_to_quantized_cdf(ptr(prob), n + 1, 16, ptr(row)))
        cdf[i, : n + 2] = row
    return cdf


def _pinned(key, numel, dtype):
    """The calling thread's pinned staging buffer ``key`` for the symbol / index planes (the only per-frame host traffic of the
    path): page-locked copies run at PCIe rate instead of through a pageable bounce buffer.  One staging set per coding thread
    (streamed sequences: one thread per frame in flight)."""
    st = _threads.current()
    ev = st.pin_busy.pop(key, None)
    if ev is not None:
        ev.synchronize()                       # the previous upload from this buffer (long done by now) before it is rewritten
    buf = st.pinned.get(key)
    if buf is None or buf.numel() < numel or buf.dtype != dtype:
        buf = st.pinned[key] = torch.empty(max(numel, 1), dtype=dtype, pin_memory=True)
    return buf[:numel]


def _to_host(t, key):
    """Device tensor -> numpy view of a pinned host buffer (valid until the next call with ``key``)."""
    t = t.contiguous()
    buf = _pinned(key, t.numel(), t.dtype)
    buf.copy_(t.reshape(-1), non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return buf.numpy().reshape(t.shape)


def _to_host_async(t, key):
    """Like _to_host without the wait: -> (numpy view, event); the view is valid after ``event.synchronize()``."""
    t = t.contiguous()
    buf = _pinned(key, t.numel(), t.dtype)
    buf.copy_(t.reshape(-1), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(t.device))
    return buf.numpy().reshape(t.shape), ev


def _upload_guard(key, device):
    """the staging buffer ``key`` of this thread has an upload in flight on the current stream: its next user waits for THAT (an event),
    not the uploader for the whole stream — a stream wait here stopped the coding thread until the GPU had drained everything queued
    (the kernel maps in front of h_s, the prefetched maps in front of g_s) and the chip then idled while the thread caught up"""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    _threads.current().pin_busy[key] = ev


def _to_device(arr, device, key):
    """numpy array -> device tensor through a pinned staging buffer."""
    src = torch.from_numpy(np.ascontiguousarray(arr))
    buf = _pinned(key, src.numel(), src.dtype)
    buf.copy_(src.reshape(-1))
    out = buf.to(device, non_blocking=True).reshape(src.shape)
    _upload_guard(key, out.device)
    return out


def _rans_thread():
    """The coding thread's job thread for the serial range-coder calls that run beside GPU work (the C calls release the interpreter
    lock).  Persistent: creating a thread per call cost the coding thread ~0.3 ms at the start of every decode (thread start + the new
    thread's Python prelude under the lock) — on the critical path, with the GPU idle."""
    return _threads.current().job_thread("pcc-rans")


@functools.lru_cache(maxsize=64)
def _channel_index_plane(c, n):
    """np.repeat(np.arange(c), n) as int32 (the factorized model's indexes: channel-major planes), cached: 150 k elements per decode.
    An eviction drops the cache's reference only: a decode in flight holds its own."""
    return np.repeat(np.arange(c, dtype=np.int32), n)


def _rans_encode(symbols, indexes, cdf, cdf_length, offset):
    """symbols / indexes: host int32 arrays (flattened channel-major)."""
    L = _lib.lib()
    symbols = np.ascontiguousarray(symbols, dtype=np.int32).reshape(-1)
    indexes = np.ascontiguousarray(indexes, dtype=np.int32).reshape(-1)
    n = symbols.size
    # typical streams need well under 1 byte per symbol; fall back to the worst-case bound if not
    for cap in (n + 4096, 4 * (3 * n + 4)):
        out = np.empty(cap, dtype=np.uint8)
        nbytes = L.pcc_rans_encode_with_indexes(ptr(symbols), ptr(indexes), n, ptr(cdf), cdf.shape[1],
                                                ptr(cdf_length), ptr(offset), ptr(out), cap)
        if nbytes >= 0:
            return out[:nbytes].tobytes()
    check(nbytes)


def _rans_encode_packed(symbols, indexes, cdf, cdf_length, offset):
    """symbols int16 / indexes uint8 host arrays (the planes pcc_gc_encode_prep_packed wrote): identical bytes"""
    L = _lib.lib()
    n = symbols.size
    for cap in (n + 4096, 4 * (3 * n + 4)):
        out = np.empty(cap, dtype=np.uint8)
        nbytes = L.pcc_rans_encode_with_indexes_i16u8(ptr(symbols), ptr(indexes), n, ptr(cdf), cdf.shape[1],
                                                      ptr(cdf_length), ptr(offset), ptr(out), cap)
        if nbytes >= 0:
            return out[:nbytes].tobytes()
    check(nbytes)


def _rans_decode_packed(data, indexes, cdf, cdf_length, offset, out):
    """indexes uint8 -> symbols into ``out`` (int16, pinned); returns False when a symbol did not fit int16"""
    L = _lib.lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    narrowed = np.zeros(1, dtype=np.int32)
    check(L.pcc_rans_decode_with_indexes_u8i16(ptr(buf), len(data), ptr(indexes), indexes.size, ptr(cdf), cdf.shape[1],
                                               ptr(cdf_length), ptr(offset), ptr(out), ptr(narrowed)))
    return int(narrowed[0]) == 0


def _rans_decode(data, indexes, cdf, cdf_length, offset):
    L = _lib.lib()
    indexes = np.ascontiguousarray(indexes, dtype=np.int32).reshape(-1)
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(indexes.size, dtype=np.int32)
    check(L.pcc_rans_decode_with_indexes(ptr(buf), len(data), ptr(indexes), indexes.size, ptr(cdf), cdf.shape[1],
                                         ptr(cdf_length), ptr(offset), ptr(out)))
    return out


# ---- the lane-parallel y stream ("PCL1") --------------------------------------------------------------
# Opt-in stream format of the y string: the symbol sequence dealt to STREAM_LANES lanes, each lane's substream what the
# reference-format coder writes for its symbols alone, coded and decoded by one GPU thread per lane (csrc/rans_lanes.hip) —
# only the stream bytes cross PCIe, and no host range coder sits between the GPU work of a frame.  0 (the default) is the
# reference's format, byte for byte.  The z string is in the reference's format in every mode.  The decoder takes the lane
# count from the stream, so any encoder's count decodes, but encoder and decoder must agree on the FORMAT: with lanes set, a
# y string without the magic is refused.  PCC_STREAM_LANES=n / set_stream_lanes(n).
LANES_MAGIC = b"PCL1"
LANES_MAX = 4096


def _lanes_setting(n):
    n = int(n)
    if not 0 <= n <= LANES_MAX:
        raise ValueError(f"PCC_STREAM_LANES / set_stream_lanes: {n} lanes (0 = the reference's format, or 1 .. {LANES_MAX})")
    return n


STREAM_LANES = _lanes_setting(os.environ.get("PCC_STREAM_LANES", "0") or 0)
LANES_RETRIES = 0          # encodes repeated with the worst-case scratch (a counter for tests and profiles)


def set_stream_lanes(n):
    global STREAM_LANES
    STREAM_LANES = _lanes_setting(n)


def _rans_lanes_encode_host(symbols, indexes, lanes, cdf, cdf_length, offset):
    """host twin of the GPU encoder: int32 host arrays -> PCL1 bytes"""
    L = _lib.lib()
    symbols = np.ascontiguousarray(symbols, dtype=np.int32).reshape(-1)
    indexes = np.ascontiguousarray(indexes, dtype=np.int32).reshape(-1)
    n = symbols.size
    head = 8 + 4 * int(lanes)
    for cap in (head + n + 4096 + 16 * int(lanes), head + 8 * n + 16 * int(lanes) + 16):
        out = np.empty(cap, dtype=np.uint8)
        nbytes = L.pcc_rans_lanes_encode_host(ptr(symbols), ptr(indexes), n, int(lanes), ptr(cdf), cdf.shape[1], ptr(cdf_length),
                                              ptr(offset), ptr(out), cap)
        if nbytes >= 0:
            return out[:nbytes].tobytes()
    check(nbytes)


def _rans_lanes_decode_host(data, indexes, cdf, cdf_length, offset):
    """host twin of the GPU decoder: PCL1 bytes -> int32 symbols; a malformed or corrupt stream raises"""
    L = _lib.lib()
    indexes = np.ascontiguousarray(indexes, dtype=np.int32).reshape(-1)
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty(indexes.size, dtype=np.int32)
    check(L.pcc_rans_lanes_decode_host(ptr(buf), len(data), ptr(indexes), indexes.size, ptr(cdf), cdf.shape[1], ptr(cdf_length),
                                       ptr(offset), ptr(out)))
    return out


def _lane_buffer(key, nbytes, device):
    """The calling thread's device buffer ``key`` of the lane coder (grown, never shrunk): two frames in flight on two coding
    threads do not share scratch; the frames of one thread follow each other on its stream."""
    bufs = _threads.current().lane_buffers
    buf = bufs.get((key, device))
    if buf is None or buf.numel() < nbytes:
        buf = bufs[(key, device)] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    return buf


_LANE_FLAGS = ((1, "a lane outgrew its scratch"), (2, "table index out of range"), (4, "symbol of frequency 0"),
               (8, "not a table blob"), (16, "a lane did not end at its initial state and the end of its substream"))


def _lane_flag_text(bits):
    return ", ".join(text for bit, text in _LANE_FLAGS if bits & bit) or "unknown"


def check_stream_status():
    """The status words of the calling thread's lane-parallel y decodes since the last call, read once (ColorModel.decompress
    calls this after g_s is enqueued: the decode itself never waits for the host).  A non-zero word raises ValueError."""
    st = _threads.current()
    pending, st.lane_status = st.lane_status, []
    bits = 0
    for word in pending:
        bits |= int(word.item())
    if bits:
        raise ValueError(f"lane-parallel y stream (PCC_STREAM_LANES): the decoder reports status {bits:#x} ({_lane_flag_text(bits)}): "
                         "the stream is corrupt or was coded with other tables")


# ---- code length without coding (DESIGN.md "Target-rate coding") ------------------------------------------------------
class CodeLength:
    """What a code-length launch (csrc/code_length.hip) returns: views of its one device int64 [C + 3] result, nothing read back.
    ``q16_bits_per_channel`` [C]: the exact table cost in 1/65536 bit; ``ops``: coder operations (symbols + bypass puts);
    ``escapes``: symbols coded through the escape slot; ``flags``: 0, or bit 1 = table index out of range, bit 2 = a slot of
    frequency 0 was hit (the sums are then unspecified).  ``symbols`` is the host-known number of symbols N * C."""
    __slots__ = ("raw", "q16_bits_per_channel", "ops", "escapes", "flags", "symbols")

    def __init__(self, raw, c, symbols):
        self.raw = raw
        self.q16_bits_per_channel, self.ops, self.escapes, self.flags = raw[:c], raw[c], raw[c + 1], raw[c + 2]
        self.symbols = int(symbols)


# E of stream_bytes_interval, per coder operation, in 1/65536 bit, as the fraction OP_SLACK_NUM / OP_SLACK_DEN:
#   2^16 * -log2(1 - 2^-15) = 2.885434...   (one put moves log2(x) off its ideal step by at most that: see the docstring)
# + 0.5                                      (the rounding of one table cost to Q16)
# = 3.385434... <= 3386 / 1000
OP_SLACK_NUM, OP_SLACK_DEN = 3386, 1000
_WORD_Q16 = 32 << 16


def stream_bytes_interval(q16_bits, ops, lanes=0, symbols=None):
    """The closed interval ``(lo, hi)`` of byte lengths that a range-coded stream can have, given its exact table cost
    ``q16_bits`` (the sum of a CodeLength's ``q16_bits_per_channel``, in 1/65536 bit) and its ``ops`` coder operations.  Pure
    integer arithmetic; derived from the coder (csrc/rans_host.cpp: put_sym, put_bits, rans_encode_run), not measured.

    One stream.  The state x starts at 2^31.  Each put first moves the low word of x out (x >>= 32) when it would overflow
    otherwise, which happens only while x >= 2^47 f, then maps x to floor(x / f) 2^16 + (x mod f) + start (a table put of
    frequency f; a bypass put is the case f = 2^12 with x 16 + value).  Against the ideal x 2^16 / f that is off by a relative
    error of at most f / x' <= 2^-15 in either direction, x' >= max(2^31, 2^15 f) being the state the put divides.  So with W
    words moved out, L = 32 W + log2(x) grows by 16 - log2(f) per put up to +-d, d = -log2(1 - 2^-15) <= 2^-15 log2(e)
    (1 + 2^-15).  It starts at 31 and the final x lies in [2^31, 2^63); the stream is W words and the two of the final state:

        bytes = 8 + 4 W,     S - 32 - E  <  32 W  <=  S + E,     E = ops * (d + 2^-17),

    S being ``q16_bits / 65536``; the 2^-17 per operation covers the rounding of a table cost to Q16 (bypass costs are exact).
    In integers: E16 = ceil(ops * 3386 / 1000) (2^16 d + 0.5 = 3.385434... per operation), W in
    [max(0, floor((q16_bits - E16) / 2^21)), floor((q16_bits + E16) / 2^21)].  The width is at most 4 bytes plus
    2 E / 8 = ops * 3386 / (1000 * 2^18) bytes: 4 bytes + 1 byte per 77,418 operations.  ops = 0 gives (8, 8).

    ``lanes`` > 0: the lane-parallel container (PCL1) of 8 + 4 lanes header bytes and one such stream per lane that holds a
    symbol; an empty lane has 0 bytes.  Summed over the m non-empty lanes: total words in [floor((q16 - E16) / 2^21) - (m - 1),
    floor((q16 + E16) / 2^21)] and 8 m bytes of final states.  m = min(lanes, symbols); when ``symbols`` is not given, the
    interval covers every m from 1 (0 if ops is 0) to min(lanes, ops).
    """
    q16_bits, ops, lanes = int(q16_bits), int(ops), int(lanes)
    if q16_bits < 0 or ops < 0 or lanes < 0:
        raise ValueError("stream_bytes_interval: negative argument")
    e16 = (ops * OP_SLACK_NUM + OP_SLACK_DEN - 1) // OP_SLACK_DEN
    w_hi = (q16_bits + e16) // _WORD_Q16
    w_lo = (q16_bits - e16) // _WORD_Q16           # = floor((S - 32 - E) / 32) + 1, the least integer above the open end
    if lanes == 0:
        return 8 + 4 * max(w_lo, 0), 8 + 4 * w_hi
    head = 8 + 4 * lanes
    if symbols is None:
        m_lo, m_hi = min(1, ops), min(lanes, ops)
    else:
        m_lo = m_hi = min(lanes, int(symbols))
    if m_hi == 0:
        return head, head
    return head + 8 * m_lo + 4 * max(w_lo - (m_lo - 1), 0), head + 8 * m_hi + 4 * w_hi


class _EntropyModelBase(nn.Module):
    def __init__(self, likelihood_bound=1e-9, entropy_coder_precision=16):
        super().__init__()
        self.entropy_coder_precision = int(entropy_coder_precision)
        self.likelihood_lower_bound = _LowerBound(likelihood_bound)
        self.register_buffer("_offset", torch.IntTensor())
        self.register_buffer("_quantized_cdf", torch.IntTensor())
        self.register_buffer("_cdf_length", torch.IntTensor())
        self._host_tables = None

    def _set_tables(self, cdf, cdf_length, offset):
        dev = self._offset.device
        self._quantized_cdf = torch.from_numpy(cdf).to(dev)
        self._cdf_length = torch.from_numpy(cdf_length).to(dev)
        self._offset = torch.from_numpy(offset).to(dev)
        self._host_tables = (np.ascontiguousarray(cdf), np.ascontiguousarray(cdf_length), np.ascontiguousarray(offset))
        self.__dict__["_lane_tables"] = {}
        self.__dict__["_cost_tables"] = {}

    def lane_tables(self, device):
        """The coding tables of the lane-parallel coder on ``device`` (pcc_rans_lanes_tables_build): built at the first use after
        update() / a checkpoint load and kept there."""
        cache = self.__dict__.setdefault("_lane_tables", {})
        device = torch.device(device)
        blob = cache.get(device)
        if blob is None:
            cdf, cdf_len, off = self.tables()
            L = _lib.lib()
            nbytes = check(L.pcc_rans_lanes_tables_bytes(ptr(cdf_len), cdf_len.size))
            host = np.empty(nbytes, dtype=np.uint8)
            check(L.pcc_rans_lanes_tables_build(ptr(cdf), cdf.shape[1], ptr(cdf_len), ptr(off), cdf_len.size, ptr(host), nbytes))
            blob = cache[device] = torch.from_numpy(host).to(device)
        return blob

    def cost_tables(self, device):
        """The Q16 cost of every slot of every coding table on ``device`` (pcc_code_length_tables_build): int32
        [n_tables, cdf_stride], ``cost[t][v] = round(65536 * (16 - log2(freq)))`` for the slots 0 .. cdf_length[t] - 2 (the last
        one is the escape symbol), -1 where the coder would refuse the slot (frequency 0) and in the unused tail of a row.
        Built at the first use after update() / a checkpoint load and kept there, like lane_tables."""
        return self._cost_tables_on(device)[0]

    def _cost_tables_on(self, device):
        """-> (cost, cdf_length, offset) on ``device``, int32: what the code-length kernels read"""
        cache = self.__dict__.setdefault("_cost_tables", {})
        device = torch.device(device)
        hit = cache.get(device)
        if hit is None:
            cdf, cdf_len, off = self.tables()
            cost = np.empty_like(cdf)
            check(_lib.lib().pcc_code_length_tables_build(ptr(cdf), cdf.shape[1], ptr(cdf_len), cdf_len.size, ptr(cost)))
            hit = cache[device] = tuple(torch.from_numpy(a).to(device) for a in (cost, cdf_len, off))
        return hit

    def code_length_planes(self, symbols, indexes):
        """The code length of int32 planes [C, N] that exist already (any column order) -> CodeLength."""
        c, n = symbols.shape
        cost, cdf_len, off = self._cost_tables_on(symbols.device)
        out = torch.empty(c + 3, dtype=torch.int64, device=symbols.device)
        check(_lib.lib().pcc_code_length_planes(ptr(symbols.contiguous()), ptr(indexes.contiguous()), n, c, ptr(cost), cost.shape[1],
                                                ptr(cdf_len), ptr(off), cost.shape[0], ptr(out), _lib.stream()))
        return CodeLength(out, c, n * c)

    def tables(self):
        if self._host_tables is None:
            if self._offset.numel() == 0:
                raise RuntimeError("entropy tables missing: call update() before compress/decompress "
                                   "(reference: evaluate.py:80-84)")
            self._host_tables = (np.ascontiguousarray(self._quantized_cdf.cpu().numpy().astype(np.int32)),
                                 np.ascontiguousarray(self._cdf_length.cpu().numpy().astype(np.int32)),
                                 np.ascontiguousarray(self._offset.cpu().numpy().astype(np.int32)))
        return self._host_tables

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # table buffers change size between a fresh module and an updated checkpoint
        for name in ("_offset", "_quantized_cdf", "_cdf_length", "scale_table"):
            key = prefix + name
            if key in state_dict and hasattr(self, name):
                setattr(self, name, state_dict[key].clone().to(getattr(self, name).device))
        self._host_tables = None
        self.__dict__["_lane_tables"] = {}
        self.__dict__["_cost_tables"] = {}
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class EntropyBottleneck(_EntropyModelBase):
    """compressai EntropyBottleneck(channels, tail_mass=1e-9, init_scale=10, filters=(3,3,3,3))."""

    def __init__(self, channels, tail_mass=1e-9, init_scale=10, filters=(3, 3, 3, 3)):
        super().__init__()
        self.channels = int(channels)
        self.filters = tuple(int(f) for f in filters)
        assert self.filters == (3, 3, 3, 3), "the HIP likelihood kernel is specialised for filters (3,3,3,3)"
        self.init_scale = float(init_scale)
        self.tail_mass = float(tail_mass)
        f = (1,) + self.filters + (1,)
        scale = self.init_scale ** (1 / (len(self.filters) + 1))
        for i in range(len(self.filters) + 1):
            init = np.log(np.expm1(1 / scale / f[i + 1]))
            self.register_parameter(f"_matrix{i}", nn.Parameter(torch.full((channels, f[i + 1], f[i]), float(init))))
            self.register_parameter(f"_bias{i}", nn.Parameter(torch.empty(channels, f[i + 1], 1).uniform_(-0.5, 0.5)))
            if i < len(self.filters):
                self.register_parameter(f"_factor{i}", nn.Parameter(torch.zeros(channels, f[i + 1], 1)))
        self.quantiles = nn.Parameter(torch.tensor([-self.init_scale, 0.0, self.init_scale]).repeat(channels, 1, 1))
        target = np.log(2 / self.tail_mass - 1)
        self.register_buffer("target", torch.tensor([-target, 0.0, target], dtype=torch.float32))

    # -- host math (used by update() and loss()) ---------------------------------------------
    def _density_params(self, device=None):
        get = lambda n: getattr(self, n) if device is None else getattr(self, n).detach().float().to(device)
        return ([get(f"_matrix{i}") for i in range(5)], [get(f"_bias{i}") for i in range(5)],
                [get(f"_factor{i}") for i in range(4)])

    @staticmethod
    def _logits_cumulative(params, v):
        mats, biases, factors = params
        for i in range(5):
            v = torch.matmul(torch.nn.functional.softplus(mats[i]), v) + biases[i]
            if i < 4:
                v = v + torch.tanh(factors[i]) * torch.tanh(v)
        return v

    def loss(self):
        """aux loss (reference: model/model.py:40-47, train.py:209)."""
        # compressai evaluates the density with stop_gradient=True here: only ``quantiles`` receive a gradient
        mats, biases, factors = self._density_params()
        frozen = ([m.detach() for m in mats], [b.detach() for b in biases], [f.detach() for f in factors])
        logits = self._logits_cumulative(frozen, self.quantiles)
        return torch.abs(logits - self.target).sum()

    def medians(self):
        q = self.quantiles
        key = (q._version, q.data_ptr())
        hit = self.__dict__.get("_medians_cache")
        if hit is None or hit[0] != key:
            hit = (key, q[:, 0, 1].detach().contiguous())          # (a strided slice: one small copy kernel per parameter version)
            self.__dict__["_medians_cache"] = hit
        return hit[1]

    @torch.no_grad()
    def update(self, force=False):
        if self._offset.numel() > 0 and not force:
            return False
        q = self.quantiles.detach().float().cpu()
        cpu = self._density_params("cpu")   # host copy of the density parameters
        med = q[:, 0, 1]
        minima = torch.clamp(torch.ceil(med - q[:, 0, 0]).int(), min=0)
        maxima = torch.clamp(torch.ceil(q[:, 0, 2] - med).int(), min=0)
        pmf_start = med - minima
        pmf_length = maxima + minima + 1
        max_length = int(pmf_length.max())
        samples = torch.arange(max_length)[None, :] + pmf_start[:, None, None]
        lo = self._logits_cumulative(cpu, samples - 0.5)
        up = self._logits_cumulative(cpu, samples + 0.5)
        s = -torch.sign(lo + up)
        pmf = torch.abs(torch.sigmoid(s * up) - torch.sigmoid(s * lo))[:, 0, :]
        tail = torch.sigmoid(lo[:, 0, :1]) + torch.sigmoid(-up[:, 0, -1:])
        cdf = _pmf_to_cdf(pmf.numpy(), tail.numpy(), pmf_length.numpy(), max_length)
        self._set_tables(cdf, (pmf_length + 2).numpy().astype(np.int32), (-minima).numpy().astype(np.int32))
        return True

    # -- device side -----------------------------------------------------------------------------
    def _kernel_params(self):
        """[C, 58] = softplus(matrix_i) | bias_i | tanh(factor_i) flattened (see pcc_eb_likelihood)."""
        parts = []
        C = self.channels
        for i in range(5):
            parts.append(torch.nn.functional.softplus(getattr(self, f"_matrix{i}").detach()).reshape(C, -1))
            parts.append(getattr(self, f"_bias{i}").detach().reshape(C, -1))
            if i < 4:
                parts.append(torch.tanh(getattr(self, f"_factor{i}").detach()).reshape(C, -1))
        out = torch.cat(parts, dim=1).contiguous().float()
        assert out.shape[1] == 58
        return out

    def quantize_features(self, z_feats, want_symbols=True, want_zhat=True):
        """z_feats [N, C] -> (symbols int32 [C, N] | None, z_hat [N, C] | None)."""
        n, c = z_feats.shape
        dev = z_feats.device
        sym = torch.empty((c, n), dtype=torch.int32, device=dev) if want_symbols else None
        zhat = torch.empty((n, c), dtype=torch.float32, device=dev) if want_zhat else None
        check(_lib.lib().pcc_eb_quantize(ptr(z_feats.contiguous()), n, c, ptr(self.medians()), ptr(sym), ptr(zhat),
                                         _lib.stream()))
        return sym, zhat

    def code_length(self, z_feats):
        """What compress_features would spend on z_feats [N, C], without coding it -> CodeLength (device tensors; nothing is
        read back, no plane written)."""
        n, c = z_feats.shape
        cost, cdf_len, off = self._cost_tables_on(z_feats.device)
        if cost.shape[0] != c:
            raise ValueError(f"code_length: {c} channels, but the model holds {cost.shape[0]} tables")
        out = torch.empty(c + 3, dtype=torch.int64, device=z_feats.device)
        check(_lib.lib().pcc_eb_code_length(ptr(z_feats.contiguous()), n, c, ptr(self.medians()), ptr(cost), cost.shape[1], ptr(cdf_len),
                                            ptr(off), ptr(out), _lib.stream()))
        return CodeLength(out, c, n * c)

    def likelihood_features(self, zhat_feats):
        """z_hat [N, C] -> likelihood plane [C, N]."""
        n, c = zhat_feats.shape
        lik = torch.empty((c, n), dtype=torch.float32, device=zhat_feats.device)
        check(_lib.lib().pcc_eb_likelihood(ptr(zhat_feats.contiguous()), n, c, ptr(self._kernel_params()), ptr(lik),
                                           _lib.stream()))
        return lik

    def _likelihood_train(self, v):
        """differentiable likelihood of v [C, 1, N] (compressai EntropyBottleneck._likelihood); elementwise
        torch ops: the training path needs gradients into the density parameters"""
        params = self._density_params()
        lower = self._logits_cumulative(params, v - 0.5)
        upper = self._logits_cumulative(params, v + 0.5)
        sign = -torch.sign(lower + upper).detach()
        return torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))

    def forward(self, x, training=None):
        """x: (1, C, N) as in the reference (``z.F.t().unsqueeze(0)``) -> (x_hat, likelihoods), both (1, C, N).
        Training mode: additive uniform noise instead of rounding, likelihoods with gradients."""
        if self.training if training is None else training:
            v = x.permute(1, 0, 2)                                   # [C, 1, N]
            v = v + _uniform_noise(v)
            lik = self.likelihood_lower_bound(self._likelihood_train(v))
            return v.permute(1, 0, 2), lik.permute(1, 0, 2)
        feats = x[0].t().contiguous()
        _, zhat = self.quantize_features(feats, want_symbols=False)
        lik = self.likelihood_features(zhat)
        return zhat.t().unsqueeze(0), lik.unsqueeze(0)

    def compress_features(self, z_feats, perm=None):
        """-> ([bytes], z_hat [N, C]); symbol order = channel-major over rows (optionally permuted)."""
        sym, zhat = self.quantize_features(z_feats)
        if perm is not None:
            sym = sym.index_select(1, perm.long())
        finish, _ = self._encode_begin(sym)
        return finish(), zhat

    def _encode_begin(self, sym):
        cdf, cdf_len, off = self.tables()
        c, n = sym.shape
        host, ev = _to_host_async(sym, "eb_sym")

        def finish():
            ev.synchronize()
            return [_rans_encode(host, np.repeat(np.arange(c, dtype=np.int32), n), cdf, cdf_len, off)]

        return finish, ev

    def compress_features_begin(self, z_feats, perm=None):
        """Two-phase form of compress_features: quantisation and the copy to the host are enqueued now; the returned
        function waits for the copy and runs the (serial, host) range coder — in between the caller can enqueue the
        GPU work that only needs z_hat (h_s, the preparation of the y symbols).  -> (finish() -> [bytes], z_hat)"""
        sym, zhat = self.quantize_features(z_feats)
        if perm is not None:
            sym = sym.index_select(1, perm.long())
        finish, _ = self._encode_begin(sym)
        return finish, zhat

    def compress(self, x):
        strings, _ = self.compress_features(x[0].t().contiguous())
        return strings

    def decompress_features(self, strings, n, device):
        """-> z_hat [N, C] on ``device``."""
        cdf, cdf_len, off = self.tables()
        c = self.channels
        idx = np.repeat(np.arange(c, dtype=np.int32), n)
        sym = torch.from_numpy(_rans_decode(strings[0], idx, cdf, cdf_len, off).reshape(c, n)).to(device)
        zhat = torch.empty((n, c), dtype=torch.float32, device=device)
        check(_lib.lib().pcc_eb_dequantize(ptr(sym), n, c, ptr(self.medians().to(device)), ptr(zhat), _lib.stream()))
        return zhat

    def decompress_features_async(self, strings, n, device):
        """Start the (host, serial) range decode of z on a worker thread — it needs nothing from the GPU — and return a
        function that joins it and dequantises: in between the caller builds the coordinate sets and kernel maps that
        depend on coordinates only."""
        cdf, cdf_len, off = self.tables()
        c = self.channels
        indexes = _channel_index_plane(c, n)
        # everything the call needs is prepared HERE: the worker's job is the C call alone (it releases the interpreter lock; Python
        # steps on the worker would each queue for the lock this thread holds while it builds the kernel maps)
        buf = np.frombuffer(strings[0], dtype=np.uint8)
        sym_host = _pinned("eb_sym32", c * n, torch.int32)          # decoded straight into the page-locked plane the upload reads
        out = sym_host.numpy()
        fn = _lib.lib().pcc_rans_decode_with_indexes
        args = (ptr(buf), len(strings[0]), ptr(indexes), indexes.size, ptr(cdf), cdf.shape[1], ptr(cdf_len), ptr(off), ptr(out))

        def work(_held=(buf, indexes, cdf, cdf_len, off, out)):      # the arrays behind the addresses live as long as the job
            return fn(*args)

        done = _rans_thread().submit(work)

        def finish():
            check(done.wait())
            sym = sym_host.to(device, non_blocking=True).reshape(c, n)
            _upload_guard("eb_sym32", device)
            zhat = torch.empty((n, c), dtype=torch.float32, device=device)
            check(_lib.lib().pcc_eb_dequantize(ptr(sym), n, c, ptr(self.medians().to(device)), ptr(zhat), _lib.stream()))
            return zhat

        return finish

    def decompress(self, strings, size):
        n = int(size[0])
        return self.decompress_features(strings, n, self.quantiles.device).t().unsqueeze(0)


class GaussianConditional(_EntropyModelBase):
    """compressai GaussianConditional(scale_table, scale_bound=0.11, tail_mass=1e-9)."""

    def __init__(self, scale_table=None, scale_bound=0.11, tail_mass=1e-9):
        super().__init__()
        self.tail_mass = float(tail_mass)
        self.lower_bound_scale = _LowerBound(scale_bound)
        self.register_buffer("scale_table",
                             torch.tensor([float(s) for s in scale_table]) if scale_table is not None else torch.Tensor())

    @torch.no_grad()
    def update_scale_table(self, scale_table, force=False):
        if self._offset.numel() > 0 and not force:
            return False
        self.scale_table = torch.tensor([float(s) for s in scale_table], device=self.scale_table.device)
        self.update()
        return True

    @torch.no_grad()
    def update(self):
        table = self.scale_table.detach().float().cpu()
        mult = -scipy.stats.norm.ppf(self.tail_mass / 2)
        center = torch.ceil(table * mult).int()
        pmf_length = 2 * center + 1
        max_length = int(pmf_length.max())
        samples = torch.abs(torch.arange(max_length).int() - center[:, None]).float()
        s = table[:, None]
        Phi = lambda v: 0.5 * torch.erfc(-(2 ** -0.5) * v)
        upper = Phi((0.5 - samples) / s)
        lower = Phi((-0.5 - samples) / s)
        pmf = upper - lower
        tail = 2 * lower[:, :1]
        cdf = _pmf_to_cdf(pmf.numpy(), tail.numpy(), pmf_length.numpy(), max_length)
        self._set_tables(cdf, (pmf_length + 2).numpy().astype(np.int32), (-center).numpy().astype(np.int32))

    # -- device side, [N, C] features; params [N, 2C] = (scales | means) aligned with y ------------
    def encode_prep(self, y_feats, params):
        n, c = y_feats.shape
        dev = y_feats.device
        sym = torch.empty((c, n), dtype=torch.int32, device=dev)
        idx = torch.empty((c, n), dtype=torch.int32, device=dev)
        table = self.scale_table.to(dev).contiguous()
        check(_lib.lib().pcc_gc_encode_prep(ptr(y_feats.contiguous()), ptr(params.contiguous()), n, c, ptr(table),
                                            table.numel(), ptr(sym), ptr(idx), _lib.stream()))
        return sym, idx

    def indexes_for(self, params, c):
        n = params.shape[0]
        dev = params.device
        idx = torch.empty((c, n), dtype=torch.int32, device=dev)
        table = self.scale_table.to(dev).contiguous()
        check(_lib.lib().pcc_gc_encode_prep(None, ptr(params.contiguous()), n, c, ptr(table), table.numel(), None,
                                            ptr(idx), _lib.stream()))
        return idx

    def code_length(self, y_feats, params):
        """What compress_features would spend on y_feats [N, C] under params [N, 2C], without coding it -> CodeLength (device
        tensors; nothing is read back, no plane written, no row order needed: a sum does not depend on it)."""
        n, c = y_feats.shape
        dev = y_feats.device
        table = self.scale_table.to(dev).contiguous()
        cost, cdf_len, off = self._cost_tables_on(dev)
        if cost.shape[0] != table.numel():
            raise ValueError(f"code_length: {table.numel()} scale levels, but the model holds {cost.shape[0]} tables")
        out = torch.empty(c + 3, dtype=torch.int64, device=dev)
        check(_lib.lib().pcc_gc_code_length(ptr(y_feats.contiguous()), ptr(params.contiguous()), n, c, ptr(table), table.numel(), ptr(cost),
                                            cost.shape[1], ptr(cdf_len), ptr(off), ptr(out), _lib.stream()))
        return CodeLength(out, c, n * c)

    def compress_features(self, y_feats, params, perm=None):
        sym, idx = self.encode_prep(y_feats, params)
        if perm is not None:
            p = perm.long()
            sym, idx = sym.index_select(1, p), idx.index_select(1, p)
        if STREAM_LANES:
            return self._lanes_encode_begin(sym, idx, STREAM_LANES)()
        return self._encode_begin(sym, idx)()

    def _lanes_encode_begin(self, sym, idx, lanes):
        """The lane-parallel form of _encode_begin: prep -> encode -> pack on the GPU (pcc_rans_lanes_encode); only the two result
        words and then the stream itself come to the host.  The first launch gives each lane scratch for 2 bytes per symbol;
        a lane that outgrows it raises a flag and the call is repeated with the format's worst case."""
        L = _lib.lib()
        sym, idx = sym.contiguous(), idx.contiguous()
        dev, n = sym.device, sym.numel()
        tables = self.lane_tables(dev)

        def launch(worst):
            sb = check(L.pcc_rans_lanes_encode_scratch_bytes(n, lanes, worst))
            ob = check(L.pcc_rans_lanes_encode_out_bytes(n, lanes, worst))
            scratch, out, result = _lane_buffer("enc_scratch", sb, dev), _lane_buffer("enc_out", ob, dev), _lane_buffer("enc_result", 8, dev)
            check(L.pcc_rans_lanes_encode(ptr(sym), ptr(idx), n, lanes, ptr(tables), worst, ptr(scratch), sb, ptr(out), ob, ptr(result),
                                          _lib.stream()))
            host, ev = _to_host_async(result[:8].view(torch.int32), "lanes_result")
            return out, host, ev

        first = launch(0)

        def finish():
            out, host, ev = first
            ev.synchronize()
            if int(host[1]) & 1:
                global LANES_RETRIES
                LANES_RETRIES += 1
                out, host, ev = launch(1)
                ev.synchronize()
            nbytes, flags = int(host[0]), int(host[1])
            if flags:
                raise ValueError(f"lane-parallel y stream: the encoder reports {flags:#x} ({_lane_flag_text(flags)})")
            return [_to_host(out[:nbytes], "lanes_stream").tobytes()]

        return finish

    def _encode_begin(self, sym, idx):
        cdf, cdf_len, off = self.tables()
        both, ev = _to_host_async(torch.stack([sym, idx]), "gc_sym_idx")

        def finish():
            ev.synchronize()
            return [_rans_encode(both[0], both[1], cdf, cdf_len, off)]

        return finish

    def compress_features_begin(self, y_feats, params, perm=None):
        """Two-phase form of compress_features (see EntropyBottleneck.compress_features_begin) -> finish() -> [bytes].
        One kernel writes the int16 symbol plane and the uint8 index plane in stream order (rows permuted on the way)
        into one buffer, one copy takes it to the host: 3 bytes per symbol instead of 8.  Symbols beyond int16 (legal,
        escape-coded, not seen with sane scales) fall back to the int32 planes."""
        if STREAM_LANES:
            # the lane-parallel stream: int32 planes in stream order stay on the device, the coder runs right behind them
            sym, idx = self.encode_prep(y_feats, params)
            if perm is not None:
                p = perm.long()
                sym, idx = sym.index_select(1, p), idx.index_select(1, p)
            return self._lanes_encode_begin(sym, idx, STREAM_LANES)
        n, c = y_feats.shape
        dev = y_feats.device
        cn = c * n
        flag_at = (3 * cn + 3) // 4 * 4
        packed = torch.empty(flag_at + 4, dtype=torch.uint8, device=dev)
        table = self.scale_table.to(dev).contiguous()
        base = packed.data_ptr()
        check(_lib.lib().pcc_gc_encode_prep_packed(ptr(y_feats.contiguous()), ptr(params.contiguous()), n, c, ptr(table), table.numel(),
                                                   ptr(None if perm is None else perm.contiguous()), base, base + 2 * cn, base + flag_at,
                                                   _lib.stream()))
        host, ev = _to_host_async(packed, "gc_packed")
        cdf, cdf_len, off = self.tables()

        def finish():
            ev.synchronize()
            if int(host[flag_at:flag_at + 4].view(np.int32)[0]):
                return self.compress_features(y_feats, params, perm)             # int32 planes
            return [_rans_encode_packed(host[:2 * cn].view(np.int16), host[2 * cn:3 * cn], cdf, cdf_len, off)]

        return finish

    def decompress_features(self, strings, params, c):
        """params rows must be in the bitstream's row order.  -> y_hat [N, C]."""
        return self.decompress_features_async(strings, params, c)()

    def decompress_features_async(self, strings, params, c):
        """Start decoding y: indexes are built on the GPU and copied to the host, then the serial rANS
        decode runs on a worker thread (the C call releases the GIL).  Returns a function that joins the
        thread, uploads the symbols and returns y_hat [N, C]; in between the caller can enqueue GPU
        work that does not depend on y (h_q, kernel maps of the first synthesis stage)."""
        if STREAM_LANES:
            return self._lanes_decode_begin(strings, params, c)
        n = params.shape[0]
        dev = params.device
        cn = c * n
        idx_dev = torch.empty(cn, dtype=torch.uint8, device=dev)
        table = self.scale_table.to(dev).contiguous()
        check(_lib.lib().pcc_gc_encode_prep_packed(None, ptr(params.contiguous()), n, c, ptr(table), table.numel(), None, None,
                                                   ptr(idx_dev), None, _lib.stream()))
        idx_host, idx_ev = _to_host_async(idx_dev, "gc_idx8")      # the worker waits for the copy; this thread goes on enqueueing h_q
        sym_host = _pinned("gc_sym16", cn, torch.int16)
        cdf, cdf_len, off = self.tables()

        # (arguments prepared here, the worker's job is the event wait and the C call: see the factorized model's decode)
        buf = np.frombuffer(strings[0], dtype=np.uint8)
        narrowed = np.zeros(1, dtype=np.int32)
        sym_np = sym_host.numpy()
        fn = _lib.lib().pcc_rans_decode_with_indexes_u8i16
        args = (ptr(buf), len(strings[0]), ptr(idx_host), idx_host.size, ptr(cdf), cdf.shape[1], ptr(cdf_len), ptr(off), ptr(sym_np), ptr(narrowed))

        def work(_held=(buf, idx_host, cdf, cdf_len, off, sym_np, narrowed)):     # (as in the factorized model's decode)
            idx_ev.synchronize()
            check(fn(*args))
            if int(narrowed[0]) == 0:
                return None
            return _rans_decode(strings[0], idx_host.astype(np.int32), cdf, cdf_len, off)      # a symbol beyond int16: int32 planes

        done = _rans_thread().submit(work)

        def finish():
            wide = done.wait()
            yhat = torch.empty((n, c), dtype=torch.float32, device=dev)
            if wide is None:
                sym = sym_host.to(dev, non_blocking=True)
                _upload_guard("gc_sym16", dev)                                   # the pinned plane is reused by the next frame
                check(_lib.lib().pcc_gc_dequantize_i16(ptr(sym), ptr(params.contiguous()), n, c, ptr(yhat), _lib.stream()))
            else:
                sym = _to_device(wide.reshape(c, n), dev, "gc_sym_up")
                check(_lib.lib().pcc_gc_dequantize(ptr(sym), ptr(params.contiguous()), n, c, ptr(yhat), _lib.stream()))
            return yhat

        return finish

    def _lanes_decode(self, data, idx):
        """PCL1 bytes + the device int32 index sequence -> (device int32 symbols like ``idx``, device status word); the header is
        checked on the host before anything is enqueued, nothing waits for the GPU"""
        if bytes(data[:4]) != LANES_MAGIC:
            raise ValueError("PCC_STREAM_LANES / set_stream_lanes is set, so the y string must be a lane-parallel (PCL1) stream, and "
                             "this one does not begin with its magic: it was coded in the reference's format (or is not a y "
                             "string).  Encoder and decoder must agree: decode with set_stream_lanes(0)")
        L = _lib.lib()
        dev = idx.device
        buf = np.frombuffer(data, dtype=np.uint8)
        check(L.pcc_rans_lanes_header(ptr(buf), len(data)))
        tables = self.lane_tables(dev)
        stage = _pinned("lanes_up", len(data), torch.uint8)
        stage.numpy()[:] = buf
        up = stage.to(dev, non_blocking=True)
        _upload_guard("lanes_up", dev)
        sym = torch.empty_like(idx)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        check(L.pcc_rans_lanes_decode(ptr(buf), ptr(up), len(data), ptr(idx), idx.numel(), ptr(tables), ptr(sym), ptr(status),
                                      _lib.stream()))
        return sym, status

    def _lanes_decode_begin(self, strings, params, c):
        """The lane-parallel form of decompress_features_async: the stream's bytes go up, the index plane is built and the decode
        (pcc_rans_lanes_decode) launched right behind what produced ``params``; nothing waits for the host and no job thread
        runs.  The returned function only dequantises.  The decoder's status word is left for check_stream_status()."""
        n = params.shape[0]
        params = params.contiguous()
        sym, status = self._lanes_decode(strings[0], self.indexes_for(params, c))
        _threads.current().lane_status.append(status)

        def finish():
            yhat = torch.empty((n, c), dtype=torch.float32, device=params.device)
            check(_lib.lib().pcc_gc_dequantize(ptr(sym), ptr(params), n, c, ptr(yhat), _lib.stream()))
            return yhat

        return finish

    def forward_features(self, y_feats, params):
        n, c = y_feats.shape
        dev = y_feats.device
        yhat = torch.empty((n, c), dtype=torch.float32, device=dev)
        lik = torch.empty((c, n), dtype=torch.float32, device=dev)
        check(_lib.lib().pcc_gc_forward(ptr(y_feats.contiguous()), ptr(params.contiguous()), n, c, ptr(yhat), ptr(lik),
                                        _lib.stream()))
        return yhat, lik

    # reference-shaped wrappers ((1, C, N) tensors) ------------------------------------------------
    def build_indexes(self, scales):
        c, n = scales.shape[1], scales.shape[2]
        params = torch.cat([scales[0].t(), torch.zeros((n, c), device=scales.device)], dim=1).contiguous()
        return self.indexes_for(params, c).unsqueeze(0)

    def forward(self, inputs, scales, means=None, training=None):
        if self.training if training is None else training:
            # compressai GaussianConditional.forward, mode "noise": y + U(-.5,.5); likelihood of the noisy value
            outputs = inputs + _uniform_noise(inputs)
            values = outputs if means is None else outputs - means
            s = self.lower_bound_scale(scales)
            values = torch.abs(values)
            Phi = lambda t: 0.5 * torch.erfc(-(2 ** -0.5) * t)
            lik = Phi((0.5 - values) / s) - Phi((-0.5 - values) / s)
            return outputs, self.likelihood_lower_bound(lik)
        means = torch.zeros_like(inputs) if means is None else means
        params = torch.cat([scales[0].t(), means[0].t()], dim=1).contiguous()
        yhat, lik = self.forward_features(inputs[0].t().contiguous(), params)
        return yhat.t().unsqueeze(0), lik.unsqueeze(0)
