// The lane-parallel y stream ("PCL1") — what the host twin (rans_host.cpp) and the kernels
// (rans_lanes.hip) share: the container constants and the layout of the device table blob.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCC_LANES_HD __host__ __device__
#else
#define PCC_LANES_HD
#endif

namespace pcc {

constexpr uint32_t kLanesMagic = 0x314C4350u;      // b"PCL1", little-endian
constexpr int kLanesMax = 4096;                    // lanes per stream (uint16 field, 1 .. 4096)
constexpr int kLanesMaxTables = 256;               // table indexes are 8 bits wide everywhere on the device (pcc_gc_encode_prep*)
constexpr int kLanesBuckets = 256;                 // start-table buckets per CDF row, as in the host decoder

// container header: magic, lanes, 0, then `lanes` byte lengths
PCC_LANES_HD inline int64_t lanes_header_bytes(int lanes) { return 8 + 4 * (int64_t)lanes; }
// symbols of lane s of a sequence of n dealt to `lanes` lanes (positions s, s + lanes, ...)
PCC_LANES_HD inline int64_t lanes_count(int64_t n, int lanes, int s) { return s < n ? (n - s + lanes - 1) / lanes : 0; }

// per-(table, symbol) encoder entry, one 16-byte load: the threshold of the renormalisation is freq << 47 and
// freq = 2^16 - cmpl_freq, so it is not stored.  rcp_shift == kLaneEncInvalid: a symbol of frequency 0.
struct LaneEnc {
    uint64_t rcp_freq;
    uint32_t bias;
    uint16_t cmpl_freq;
    uint16_t rcp_shift;
};
constexpr uint16_t kLaneEncInvalid = 0xFFFFu;

struct LaneTableMeta {
    int32_t enc_row;     // first LaneEnc of the table
    int32_t cdf_row;     // first entry of the table in cdf[] / sf[]
    int32_t maxv;        // cdf_size - 2: the escape symbol
    int32_t offset;
};

// The blob pcc_rans_lanes_tables_build writes (host) and the kernels read (device).  Every section is 16-byte aligned.
//   meta[n_tables]            LaneTableMeta
//   enc[n_enc]                LaneEnc, rows back to back
//   lut[n_tables][256]        uint64: start | freq << 16 | symbol << 32 | pure << 47 (the host decoder's start table)
//   sf[n_cdf + 1]             uint32: start | freq << 16
//   cdf[n_cdf + 1]            uint32: the rows themselves, then a sentinel
struct LaneTablesHeader {
    uint32_t magic;      // kLanesMagic
    int32_t n_tables;
    int64_t total_bytes;
    int64_t meta_off, enc_off, lut_off, sf_off, cdf_off;
    int64_t n_enc, n_cdf;
};

// flag bits of the encoder's result word / the decoder's status word
constexpr int32_t kLanesFlagOverflow = 1;      // encoder: a lane outgrew its scratch slice (repeat with the worst-case capacity)
constexpr int32_t kLanesFlagIndex = 2;         // a table index outside the tables
constexpr int32_t kLanesFlagZeroFreq = 4;      // encoder: a symbol of frequency 0
constexpr int32_t kLanesFlagTables = 8;        // the table blob is not one
constexpr int32_t kLanesFlagEndState = 16;     // decoder: a lane did not end at state 2^31 and the end of its substream

}  // namespace pcc
