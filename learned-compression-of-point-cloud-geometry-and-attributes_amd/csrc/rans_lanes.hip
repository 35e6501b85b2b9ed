// The lane-parallel y stream ("PCL1") coded and decoded where the symbols are: one thread per lane.
//
// The stream deals the y symbol sequence (the [C, N] planes in stream order) to P lanes — lane s owns positions
// s, s + P, ... so adjacent lanes read adjacent memory — and lane s's substream is exactly what the host coder
// (rans_host.cpp) writes for that subsequence alone: 64-bit state, 32-bit words, 16-bit precision, 4-bit bypass
// escapes, 8-byte final state.  The host twin there (pcc_rans_lanes_encode_host / _decode_host) is the statement
// these kernels are tested against, byte for byte.
//
//  * encode: a lane sweeps its symbols backwards (put_sym / put_bits of the host coder, __umul64hi for the
//    reciprocal multiply) and writes its words downwards into its slice of the scratch; symbols, table rows and
//    encoder entries of the next few symbols are loaded in batches ahead of the state chain, which they do not
//    depend on.  A second kernel sums the lane lengths, writes the header and packs the substreams behind it.
//  * decode: a lane carries the state -> slot -> symbol -> state chain of the host decoder.  The first lookup of
//    that chain, the 256-bucket start table, sits in LDS (64 tables x 256 x 8 B = 128 KiB: one workgroup of 256
//    threads per CU, one wave per SIMD); impure buckets finish with the short forward scan over the row in
//    global memory.  Every read of the stream is clamped to the lane's own substream, zeros lie beyond it.
// Escape loops diverge between lanes; that costs the wave the longest lane's time, nothing else.
#include <string.h>

#include "common.h"
#include "rans_lanes.h"

namespace pcc {

constexpr int kPrecision = 16;
constexpr int kBypassBits = 4;
constexpr uint32_t kBypassMax = 15;
constexpr uint64_t kRansL = 1ull << 31;
constexpr int kLdsTables = 64;       // start tables kept in LDS by the decoder (the default scale table has 64 levels)
constexpr int kEncBatch = 4;         // symbols whose loads are issued together, ahead of the encoder's state chain
constexpr int kDecBatch = 8;         // table indexes loaded together, ahead of the decoder's

struct LaneWriter {
    uint32_t* ptr;       // grows downwards
    uint32_t* base;      // lowest writable word of the lane's slice
    bool overflow;
    __device__ __forceinline__ void emit(uint32_t v) {
        if (ptr > base) *--ptr = v;
        else overflow = true;
    }
};

__device__ __forceinline__ void lane_put_bits(uint64_t& x, LaneWriter& w, uint32_t val) {
    const uint64_t x_max = ((kRansL >> 16) << 32) * (1ull << (16 - kBypassBits));
    if (x >= x_max) { w.emit((uint32_t)x); x >>= 32; }
    x = (x << kBypassBits) | val;
}

__global__ __launch_bounds__(256) void rans_lanes_encode_kernel(const int32_t* __restrict__ sym, const int32_t* __restrict__ idx,
                                                                int64_t n, int lanes, const uint8_t* __restrict__ tables,
                                                                uint32_t* __restrict__ lane_words, uint32_t* __restrict__ words,
                                                                int64_t cap_words, int32_t* __restrict__ result) {
    __shared__ LaneTableMeta meta_s[kLanesMaxTables];
    const LaneTablesHeader* h = reinterpret_cast<const LaneTablesHeader*>(tables);
    const int n_tables = h->n_tables;
    if (h->magic != kLanesMagic || n_tables < 1 || n_tables > kLanesMaxTables) {          // (uniform: the whole grid leaves)
        if (threadIdx.x == 0) atomicOr(&result[1], kLanesFlagTables);
        return;
    }
    const LaneTableMeta* meta_g = reinterpret_cast<const LaneTableMeta*>(tables + h->meta_off);
    const LaneEnc* enc = reinterpret_cast<const LaneEnc*>(tables + h->enc_off);
    for (int t = threadIdx.x; t < n_tables; t += 256) meta_s[t] = meta_g[t];
    __syncthreads();
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= lanes) return;                                     // the masked part of the last wave
    const int64_t count = lanes_count(n, lanes, s);
    if (count == 0) { lane_words[s] = 0; return; }
    uint32_t* const top = words + (int64_t)(s + 1) * cap_words;
    LaneWriter w{top, words + (int64_t)s * cap_words, false};
    uint64_t x = kRansL;
    int32_t flags = 0;
    for (int64_t k0 = count - 1; k0 >= 0; k0 -= kEncBatch) {
        int32_t sy[kEncBatch], ix[kEncBatch];
#pragma unroll
        for (int u = 0; u < kEncBatch; ++u) {
            const int64_t k = k0 - u > 0 ? k0 - u : 0;          // (a batch that runs past the lane's first symbol re-reads it)
            const int64_t i = s + k * lanes;
            sy[u] = sym[i];
            ix[u] = idx[i];
        }
        LaneEnc e[kEncBatch];
        uint32_t raw[kEncBatch];
        bool esc[kEncBatch];
#pragma unroll
        for (int u = 0; u < kEncBatch; ++u) {
            int t = ix[u];
            if ((uint32_t)t >= (uint32_t)n_tables) { flags |= kLanesFlagIndex; t = 0; }
            const LaneTableMeta m = meta_s[t];
            int32_t v = sy[u] - m.offset;
            esc[u] = (uint32_t)v >= (uint32_t)m.maxv;           // v < 0 or v >= maxv: escape
            raw[u] = v < 0 ? (uint32_t)(-2 * v - 1) : (uint32_t)(2 * (v - m.maxv));
            v = esc[u] ? m.maxv : v;
            e[u] = enc[m.enc_row + v];
        }
#pragma unroll
        for (int u = 0; u < kEncBatch; ++u) {
            if (k0 - u < 0) break;
            if (esc[u]) {
                int nb = 0;
                while (nb < 8 && (raw[u] >> (nb * kBypassBits)) != 0) ++nb;
                // forward order: main, count chunks (15, 15, ..., rest), nibbles LSB first  => reverse here
                for (int j = nb - 1; j >= 0; --j) lane_put_bits(x, w, (raw[u] >> (j * kBypassBits)) & kBypassMax);
                lane_put_bits(x, w, (uint32_t)nb);              // nb <= 8 < 15: one count chunk
            }
            if (e[u].rcp_shift == kLaneEncInvalid) { flags |= kLanesFlagZeroFreq; continue; }
            const uint64_t x_max = (uint64_t)(65536u - e[u].cmpl_freq) << 47;          // ((2^31 >> 16) << 32) * freq
            if (x >= x_max) { w.emit((uint32_t)x); x >>= 32; }
            const uint64_t q = __umul64hi(x, e[u].rcp_freq) >> e[u].rcp_shift;
            x = x + e[u].bias + q * e[u].cmpl_freq;
        }
    }
    w.emit((uint32_t)(x >> 32));
    w.emit((uint32_t)x);
    if (w.overflow) flags |= kLanesFlagOverflow;
    lane_words[s] = w.overflow ? 0u : (uint32_t)(top - w.ptr);
    if (flags) atomicOr(&result[1], flags);
}

// one wave per lane: the lane's place is the header plus the lengths in front of it
__global__ __launch_bounds__(64) void rans_lanes_pack_kernel(const uint32_t* __restrict__ lane_words, const uint32_t* __restrict__ words,
                                                             int64_t cap_words, int lanes, uint32_t* __restrict__ out,
                                                             int32_t* __restrict__ result) {
    const int s = blockIdx.x;
    uint32_t before = 0;
    for (int j = threadIdx.x; j < s; j += 64) before += lane_words[j];
    for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d, 64);
    const uint32_t len = lane_words[s];
    const int64_t at = lanes_header_bytes(lanes) / 4 + before;
    const uint32_t* src = words + (int64_t)(s + 1) * cap_words - len;
    for (uint32_t t = threadIdx.x; t < len; t += 64) out[at + t] = src[t];
    if (threadIdx.x == 0) {
        out[2 + s] = len * 4u;
        if (s == 0) { out[0] = kLanesMagic; out[1] = (uint32_t)lanes; }
        if (s == lanes - 1) result[0] = (int32_t)((at + len) * 4);
    }
}

__global__ __launch_bounds__(256) void rans_lanes_decode_kernel(const uint32_t* __restrict__ stream, int64_t stream_words, int lanes,
                                                                const int32_t* __restrict__ idx, int64_t n,
                                                                const uint8_t* __restrict__ tables, int32_t* __restrict__ out_sym,
                                                                int32_t* __restrict__ status) {
    __shared__ uint64_t lut_s[kLdsTables * kLanesBuckets];
    __shared__ LaneTableMeta meta_s[kLanesMaxTables];
    __shared__ uint32_t scan_s[256];
    const int tid = threadIdx.x;
    const LaneTablesHeader* h = reinterpret_cast<const LaneTablesHeader*>(tables);
    const int n_tables = h->n_tables;
    if (h->magic != kLanesMagic || n_tables < 1 || n_tables > kLanesMaxTables) {          // (uniform)
        if (tid == 0) atomicOr(status, kLanesFlagTables);
        return;
    }
    const LaneTableMeta* meta_g = reinterpret_cast<const LaneTableMeta*>(tables + h->meta_off);
    const uint64_t* lut_g = reinterpret_cast<const uint64_t*>(tables + h->lut_off);
    const uint32_t* sf = reinterpret_cast<const uint32_t*>(tables + h->sf_off);
    const uint32_t* cdf = reinterpret_cast<const uint32_t*>(tables + h->cdf_off);
    const bool in_lds = n_tables <= kLdsTables;
    for (int t = tid; t < n_tables; t += 256) meta_s[t] = meta_g[t];
    if (in_lds)
        for (int j = tid; j < n_tables * kLanesBuckets; j += 256) lut_s[j] = lut_g[j];

    // where the lane's substream begins: the lengths of the lanes in front of this workgroup, then a scan inside it
    const int s0 = blockIdx.x * 256, s = s0 + tid;
    uint32_t part = 0;
    for (int j = tid; j < s0; j += 256) part += stream[2 + j] >> 2;
    scan_s[tid] = part;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) scan_s[tid] += scan_s[tid + d];
        __syncthreads();
    }
    const uint32_t before = scan_s[0];
    __syncthreads();
    const uint32_t len = s < lanes ? stream[2 + s] >> 2 : 0u;
    scan_s[tid] = len;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t add = tid >= d ? scan_s[tid - d] : 0u;
        __syncthreads();
        scan_s[tid] += add;
        __syncthreads();
    }
    if (s >= lanes) return;                                     // the masked part of the last wave (no barrier below)
    const int64_t count = lanes_count(n, lanes, s);
    if (count == 0) return;
    int64_t first = lanes_header_bytes(lanes) / 4 + before + (scan_s[tid] - len);
    int64_t last = first + len;
    if (last > stream_words) last = stream_words;               // (the host checked the header: never taken)
    if (first > last) first = last;
    const uint32_t* p = stream + first;
    const uint32_t* const end = stream + last;
    // the state's two words, then one word of look-ahead: the refill's load is issued a symbol before it is used
    auto next_word = [&]() -> uint32_t { const uint32_t v = p < end ? *p : 0u; p += p < end ? 1 : 0; return v; };
    uint64_t x = next_word();
    x |= (uint64_t)next_word() << 32;
    uint32_t ahead = p < end ? *p : 0u;
    auto refill = [&]() {
        if (x < kRansL) {
            x = (x << 32) | ahead;
            p += p < end ? 1 : 0;
            ahead = p < end ? *p : 0u;
        }
    };
    auto get_bits = [&]() -> uint32_t { const uint32_t v = (uint32_t)(x & kBypassMax); x >>= kBypassBits; refill(); return v; };
    int32_t flags = 0;
    for (int64_t k0 = 0; k0 < count; k0 += kDecBatch) {
        int32_t ix[kDecBatch];
#pragma unroll
        for (int u = 0; u < kDecBatch; ++u) {
            const int64_t k = k0 + u < count ? k0 + u : count - 1;
            ix[u] = idx[s + k * lanes];
        }
#pragma unroll
        for (int u = 0; u < kDecBatch; ++u) {
            if (k0 + u >= count) break;
            int t = ix[u];
            if ((uint32_t)t >= (uint32_t)n_tables) { flags |= kLanesFlagIndex; t = 0; }
            const LaneTableMeta m = meta_s[t];
            const uint32_t cf = (uint32_t)(x & 0xFFFFu);
            const int slot = t * kLanesBuckets + (int)(cf >> (kPrecision - 8));
            uint64_t e;
            if (in_lds) e = lut_s[slot];
            else e = lut_g[slot];
            int32_t v = (int32_t)((e >> 32) & 0x7FFFu);
            uint32_t sfe = (uint32_t)e;
            if (!(e >> 47)) {
                // == (first j with cdf[j] > cf) - 1; the row ends with 2^16 > cf, so the scan stops in range
                const uint32_t* row = cdf + m.cdf_row;
                while (v <= m.maxv && row[v + 1] <= cf) ++v;
                sfe = sf[m.cdf_row + v];
            }
            x = (uint64_t)(sfe >> 16) * (x >> kPrecision) + cf - (sfe & 0xFFFFu);
            refill();
            int32_t value = v;
            if (value == m.maxv) {
                uint32_t val = get_bits();
                int32_t nb = (int32_t)val;
                while (val == kBypassMax && nb < 64) { val = get_bits(); nb += (int32_t)val; }       // (a valid stream has nb <= 8)
                uint32_t raw = 0;
                for (int32_t j = 0; j < nb; ++j) {
                    const uint32_t b = get_bits();
                    if (j < 8) raw |= b << (j * kBypassBits);
                }
                value = (int32_t)(raw >> 1);
                value = (raw & 1u) ? -value - 1 : value + m.maxv;
            }
            out_sym[s + (k0 + u) * lanes] = value + m.offset;
        }
    }
    // the encoder began at state 2^31 with nothing written: a stream that was decoded as it was written ends there
    if (!(x == kRansL && p == end)) flags |= kLanesFlagEndState;
    if (flags) atomicOr(status, flags);
}

// words per lane slice: the first guess (2 bytes per symbol and a margin; typical streams stay well under 1) or the
// worst case of the format (16 + 4 * 9 bits per symbol, and the final state)
static int64_t lane_cap_words(int64_t n, int lanes, int worst_case) {
    const int64_t per_lane = (n + lanes - 1) / lanes;
    return worst_case ? 2 * per_lane + 4 : per_lane / 2 + 16;
}

}  // namespace pcc

using namespace pcc;

extern "C" {

int64_t pcc_rans_lanes_encode_scratch_bytes(int64_t n, int32_t lanes, int32_t worst_case) {
    if (n < 0 || n >= (1ll << 27) || lanes < 1 || lanes > kLanesMax) { set_error("pcc_rans_lanes_encode_scratch_bytes: n %lld, lanes %d out of range", (long long)n, lanes); return PCC_ERR_ARG; }
    return 4 * ((int64_t)lanes + (int64_t)lanes * lane_cap_words(n, lanes, worst_case));
}

int64_t pcc_rans_lanes_encode_out_bytes(int64_t n, int32_t lanes, int32_t worst_case) {
    if (n < 0 || n >= (1ll << 27) || lanes < 1 || lanes > kLanesMax) { set_error("pcc_rans_lanes_encode_out_bytes: n %lld, lanes %d out of range", (long long)n, lanes); return PCC_ERR_ARG; }
    return lanes_header_bytes(lanes) + 4 * (int64_t)lanes * lane_cap_words(n, lanes, worst_case);
}

int pcc_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, int64_t n, int32_t lanes, const void* tables,
                          int32_t worst_case, void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t out_cap,
                          int32_t* result, void* stream) {
    const int64_t need = pcc_rans_lanes_encode_scratch_bytes(n, lanes, worst_case);
    if (need < 0) return (int)need;
    PCC_REQUIRE(tables && scratch && out && result && (n == 0 || (symbols && indexes)), "pcc_rans_lanes_encode: null argument");
    PCC_REQUIRE(scratch_bytes >= need, "pcc_rans_lanes_encode: scratch of %lld bytes, needs %lld", (long long)scratch_bytes, (long long)need);
    PCC_REQUIRE(out_cap >= pcc_rans_lanes_encode_out_bytes(n, lanes, worst_case), "pcc_rans_lanes_encode: output of %lld bytes, needs %lld",
                (long long)out_cap, (long long)pcc_rans_lanes_encode_out_bytes(n, lanes, worst_case));
    PCC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(tables) & 15) == 0, "pcc_rans_lanes_encode: misaligned buffer");
    const int64_t cap_words = lane_cap_words(n, lanes, worst_case);
    uint32_t* lane_words = static_cast<uint32_t*>(scratch);
    uint32_t* words = lane_words + lanes;
    PCC_CHECK_HIP(hipMemsetAsync(result, 0, 2 * sizeof(int32_t), as_stream(stream)));
    hipLaunchKernelGGL(rans_lanes_encode_kernel, dim3((lanes + 255) / 256), dim3(256), 0, as_stream(stream), symbols, indexes, n, lanes,
                       static_cast<const uint8_t*>(tables), lane_words, words, cap_words, result);
    PCC_LAUNCH_CHECK();
    hipLaunchKernelGGL(rans_lanes_pack_kernel, dim3(lanes), dim3(64), 0, as_stream(stream), lane_words, words, cap_words, lanes,
                       reinterpret_cast<uint32_t*>(out), result);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

int pcc_rans_lanes_decode(const uint8_t* data_host, const uint8_t* data, int64_t nbytes, const int32_t* indexes, int64_t n,
                          const void* tables, int32_t* out_symbols, int32_t* status, void* stream) {
    // the header is checked on the host's copy of the stream before anything is launched on the device's
    const int64_t lanes = pcc_rans_lanes_header(data_host, nbytes);
    if (lanes < 0) return (int)lanes;
    PCC_REQUIRE(n >= 0 && n < (1ll << 27), "pcc_rans_lanes_decode: n %lld out of range", (long long)n);
    PCC_REQUIRE(data && tables && status && (n == 0 || (indexes && out_symbols)), "pcc_rans_lanes_decode: null argument");
    PCC_REQUIRE((reinterpret_cast<uintptr_t>(data) & 3) == 0 && (reinterpret_cast<uintptr_t>(tables) & 15) == 0,
                "pcc_rans_lanes_decode: misaligned buffer");
    for (int s = 0; s < (int)lanes; ++s) {
        uint32_t len;
        memcpy(&len, data_host + 8 + 4 * (int64_t)s, 4);
        if ((lanes_count(n, (int)lanes, s) == 0) != (len == 0)) {
            set_error("pcc_rans_lanes_decode: lane %d holds %u bytes for %lld symbols", s, len, (long long)lanes_count(n, (int)lanes, s));
            return PCC_ERR_DATA;
        }
    }
    PCC_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), as_stream(stream)));
    if (n == 0) return PCC_OK;
    hipLaunchKernelGGL(rans_lanes_decode_kernel, dim3(((int)lanes + 255) / 256), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint32_t*>(data), nbytes / 4, (int)lanes, indexes, n, static_cast<const uint8_t*>(tables),
                       out_symbols, status);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // extern "C"
