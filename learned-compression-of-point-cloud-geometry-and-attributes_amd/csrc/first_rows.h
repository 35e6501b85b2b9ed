// First-row-wins coordinate sets for the operators that live outside coords.hip (the rotation of augment.hip, the voxelisation of
// voxelize.hip): unique candidate rows in order of first appearance, the lowest candidate index wins.
//
// The scheme is the coordinate manager's (coords.hip, unique_coords): claim the candidate's slot in the hashed-voxel table, atomicMin
// the candidate index into the slot's value, flag the winners, scan the flags, and let every winner write its output row and
// turn its slot's value into the row id — so the result does not depend on thread arrival order and the table indexes the output
// set on return.  It lives here because coords.hip is part of the kernel-source stamp of the benchmark's committed HBM-traffic
// profile (bench.py, kernel_source_sha256): operators added beside it must not edit it.  Always the seven-launch form (clear,
// insert, flag, three scan kernels, finalize); the scan and the count word are coords.hip's scan_flags.
//
// An operator supplies two function objects, passed to the kernels by value:
//   Gen:  int4 get(int64_t i)  the candidate's (batch, x, y, z); a candidate to reject gets coordinates coord_in_range refuses
//         bool ok(int64_t i, bool in_range)   the whole validity test: in_range (coord_in_range of get(i)) and whatever else the
//                              operator requires of candidate i, evaluated in that order (nothing is read for one out of range)
//   Sink: void operator()(int32_t row, int64_t i)   what winner i writes beside its output row
// A rejected candidate raises the error word (the count word then reports COUNT_ERR_RANGE) and takes no part in the set.
// The kernels are templates or static: the header is compiled into more than one object.
#pragma once
#include "common.h"
#include "sort.h"

namespace pcc {

// claim (or find) the slot of `key`: the mirror image of table_find (common.h), slot for slot, for a table of tensor stride 1: the
// key's lane first (every 8th slot), then slot by slot.  With cap >= 2 * candidates a free slot exists, so the second loop always
// returns; mask + 1 is unreachable and the callers still guard it.
__device__ __forceinline__ uint64_t table_claim_slot(uint64_t* keys, uint64_t mask, uint64_t key) {
    const uint64_t slot0 = table_slot0(key, mask, 0);
    uint64_t slot = slot0;
    for (uint64_t probe = 0; probe <= mask; probe += TABLE_PROBE_STEP) {
        uint64_t cur = keys[slot];
        if (cur == KEY_EMPTY) {
            cur = (uint64_t)atomicCAS((unsigned long long*)&keys[slot], (unsigned long long)KEY_EMPTY, (unsigned long long)key);
            if (cur == KEY_EMPTY) return slot;
        }
        if (cur == key) return slot;
        slot = (slot + TABLE_PROBE_STEP) & mask;
    }
    for (uint64_t probe = 1; probe <= mask; ++probe) {
        slot = (slot0 + probe) & mask;
        uint64_t cur = keys[slot];
        if (cur == KEY_EMPTY) {
            cur = (uint64_t)atomicCAS((unsigned long long*)&keys[slot], (unsigned long long)KEY_EMPTY, (unsigned long long)key);
            if (cur == KEY_EMPTY) return slot;
        }
        if (cur == key) return slot;
    }
    return mask + 1;
}

// scratch as pcc_scan_scratch_elems(n) lays it out: slot per candidate, flags, the scan's block sums, then the error word
struct FirstRowsScratch {
    int32_t *slot_of, *flags, *block_sums, *err;
    FirstRowsScratch(int32_t* scratch, int64_t n)
        : slot_of(scratch), flags(scratch + n), block_sums(scratch + 2 * n), err(block_sums + (scan_block_sums_elems(n) - 16) + 8) {}
};

static __global__ __launch_bounds__(256) void first_rows_clear_kernel(uint64_t* __restrict__ keys, int32_t* __restrict__ vals,
                                                                      int64_t cap, int32_t* __restrict__ err) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *err = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = KEY_EMPTY;
        vals[i] = 0x7fffffff;
    }
}

template <class Gen>
__global__ __launch_bounds__(256) void first_rows_insert_kernel(Gen gen, int64_t m, uint64_t* __restrict__ keys,
                                                                int32_t* __restrict__ vals, uint64_t mask,
                                                                int32_t* __restrict__ slot_of, int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int4 c = gen.get(i);
    if (!gen.ok(i, coord_in_range(c.x, c.y, c.z, c.w))) {
        *err = 1;
        slot_of[i] = (int32_t)(mask + 1);
        return;
    }
    const uint64_t slot = table_claim_slot(keys, mask, pack_key(c.x, c.y, c.z, c.w));
    slot_of[i] = (int32_t)slot;
    if (slot <= mask) atomicMin(&vals[slot], (int32_t)i);
}

static __global__ __launch_bounds__(256) void first_rows_flag_kernel(int64_t m, const int32_t* __restrict__ vals, uint32_t mask,
                                                                     const int32_t* __restrict__ slot_of,
                                                                     int32_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t slot = (uint32_t)slot_of[i];
    flags[i] = (slot <= mask && vals[slot] == (int32_t)i) ? 1 : 0;       // slot > mask: the candidate was rejected (range error)
}

// incl = inclusive scan of the winner flags: candidate i won iff the scan steps at i, and its output row is incl[i] - 1
template <class Gen, class Sink>
__global__ __launch_bounds__(256) void first_rows_finalize_kernel(Gen gen, Sink sink, int64_t m, int32_t* __restrict__ vals,
                                                                  const int32_t* __restrict__ slot_of,
                                                                  const int32_t* __restrict__ incl, int32_t* __restrict__ out_coords) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int32_t cur = incl[i], prev = i ? incl[i - 1] : 0;
    if (cur != prev) {
        const int32_t row = cur - 1;
        reinterpret_cast<int4*>(out_coords)[row] = gen.get(i);
        sink(row, i);
        vals[slot_of[i]] = row;
    }
}

// The set of candidates 0 .. n-1: out_coords int32 [n,4] and *out_count (device int64: the row count, or COUNT_ERR_RANGE) as the
// header describes them; on return (keys, vals, cap) is the table of the output set and FirstRowsScratch(scratch, n).slot_of holds
// every candidate's slot (mask + 1 for a rejected one).  The caller has checked its arguments (cap a power of two >= 2 n).
// n = 0 clears the table, zeroes the count and launches nothing else.
template <class Gen, class Sink>
static int first_rows_build(const Gen& gen, const Sink& sink, int64_t n, uint64_t* keys, int32_t* vals, int64_t cap, int32_t* scratch,
                            int32_t* out_coords, int64_t* out_count, hipStream_t st) {
    const FirstRowsScratch s(scratch, n);
    hipLaunchKernelGGL(first_rows_clear_kernel, dim3(blocks_for(cap, 256, 4096)), dim3(256), 0, st, keys, vals, cap, s.err);
    if (n == 0) {
        PCC_CHECK_HIP(hipMemsetAsync(out_count, 0, sizeof(int64_t), st));
        return PCC_OK;
    }
    const unsigned nb = blocks_for(n, 256);
    hipLaunchKernelGGL(first_rows_insert_kernel<Gen>, dim3(nb), dim3(256), 0, st, gen, n, keys, vals, (uint64_t)(cap - 1), s.slot_of, s.err);
    hipLaunchKernelGGL(first_rows_flag_kernel, dim3(nb), dim3(256), 0, st, n, (const int32_t*)vals, (uint32_t)(cap - 1),
                       (const int32_t*)s.slot_of, s.flags);
    const int rc = scan_flags(s.flags, n, s.flags, s.block_sums, out_count, 1, st, s.err);
    if (rc) return rc;
    hipLaunchKernelGGL((first_rows_finalize_kernel<Gen, Sink>), dim3(nb), dim3(256), 0, st, gen, sink, n, vals, (const int32_t*)s.slot_of,
                       (const int32_t*)s.flags, out_coords);
    PCC_LAUNCH_CHECK();
    return PCC_OK;
}

}  // namespace pcc
