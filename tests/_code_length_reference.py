"""numpy restatement of the code length of a symbol sequence under range-coder tables: the Q16 cost table and the per-symbol
cost as the host coder walks it (one table put per symbol, an escaped value in 4-bit bypass puts).  Independent of the
library: the tests compare the host builder, the GPU kernels and the real coders' stream lengths against this."""
import numpy as np

PRECISION = 16
BYPASS_Q16 = 4 << 16                    # one bypass put codes exactly 4 bits
FLAG_INDEX, FLAG_FREQ0 = 2, 4


def cost_table(cdf, cdf_sizes):
    """int32 [n_tables, stride]: round(65536 * (16 - log2(freq))) for the slots 0 .. cdf_sizes[t] - 2, freq = the low 16 bits of
    cdf[v + 1] - cdf[v] (how the coder reads a frequency); -1 for frequency 0 and for the unused tail of a row"""
    cdf = np.asarray(cdf, dtype=np.int64)
    out = np.full(cdf.shape, -1, dtype=np.int32)
    for t, size in enumerate(np.asarray(cdf_sizes)):
        freq = (cdf[t, 1:size] - cdf[t, :size - 1]) & 0xFFFF
        ok = freq > 0
        bits = PRECISION - np.log2(freq[ok].astype(np.float64))
        row = np.full(size - 1, -1, dtype=np.int64)
        row[ok] = np.rint(65536.0 * bits).astype(np.int64)
        out[t, :size - 1] = row
    return out


def symbol_costs(symbols, indexes, cost, cdf_sizes, offsets):
    """per symbol: (q16 cost int64, coder operations int64, escaped bool, flags int64) — the flags are FLAG_INDEX for a table
    index outside the tables and FLAG_FREQ0 for a slot of frequency 0; a flagged symbol contributes nothing to the sums"""
    symbols = np.asarray(symbols, dtype=np.int64).reshape(-1)
    indexes = np.asarray(indexes, dtype=np.int64).reshape(-1)
    cdf_sizes = np.asarray(cdf_sizes, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_tables = cdf_sizes.size
    bad_ix = (indexes < 0) | (indexes >= n_tables)
    ix = np.where(bad_ix, 0, indexes)
    maxv = cdf_sizes[ix] - 2
    v = symbols - offsets[ix]
    escaped = (v < 0) | (v >= maxv)
    raw = np.where(v < 0, -2 * v - 1, 2 * (v - maxv))
    raw = np.where(escaped, raw, 0)
    nb = np.zeros(raw.shape, dtype=np.int64)
    r = raw.copy()
    while (r > 0).any():                                # nibbles of raw
        nb += r > 0
        r >>= 4
    puts = np.where(escaped, nb + nb // 15 + 1, 0)
    slot = np.where(escaped, maxv, v)
    table = np.asarray(cost, dtype=np.int64)[ix, slot]
    freq0 = ~bad_ix & (table < 0)
    flags = np.where(bad_ix, FLAG_INDEX, 0) | np.where(freq0, FLAG_FREQ0, 0)
    ok = flags == 0
    q16 = np.where(ok, table + puts * BYPASS_Q16, 0)
    ops = np.where(ok, 1 + puts, 0)
    return q16, ops, escaped & ok, flags


def code_length(symbols, indexes, cost, cdf_sizes, offsets):
    """planes [C, N] (or any leading channel axis) -> int64 [C + 3] as the kernels write it: Q16 bits per channel, operations,
    escapes, flags"""
    symbols = np.asarray(symbols)
    c = symbols.shape[0]
    q16, ops, esc, flags = symbol_costs(symbols, indexes, cost, cdf_sizes, offsets)
    out = np.zeros(c + 3, dtype=np.int64)
    out[:c] = q16.reshape(c, -1).sum(axis=1)
    out[c], out[c + 1] = ops.sum(), esc.sum()
    out[c + 2] = np.bitwise_or.reduce(flags) if flags.size else 0
    return out
