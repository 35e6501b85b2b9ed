// First-row-wins coordinate sets: unique candidate rows in order of first appearance, the lowest candidate index wins.  The one
// builder of the library: the coordinate manager's stride maps and generative child sets (coords.hip, unique_coords), the rotation
// (augment.hip), the voxelisation (voxelize.hip) and the position scaling (rescale.hip) all go through first_rows_build.
//
// The scheme: claim the candidate's slot in the hashed-voxel table (table_claim, common.h), atomicMin the candidate index into the
// slot's value, flag the winners, scan the flags, and let every winner write its output row and turn its slot's value into the row
// id — so the result does not depend on thread arrival order and the table indexes the output set on return.  Seven launches
// (clear, insert, flag, three scan kernels, finalize); the scan and the count word are coords.hip's scan_flags.  (The coordinate
// manager alone also has a one-workgroup form for small sets, coords.hip unique_small_kernel, over the same generators.)
//
// An operator supplies two function objects, passed to the kernels by value:
//   Gen:  int shift            log2 of the output set's tensor stride (table_slot0); `static constexpr int shift = 0` for a set of
//                              stride 1, which folds the shift out of its kernels
//         int4 get(int64_t i)  the candidate's (batch, x, y, z); a candidate to reject gets coordinates coord_in_range refuses
//         bool ok(int64_t i, bool in_range)   the whole validity test: in_range (coord_in_range of get(i)) and whatever else the
//                              operator requires of candidate i, evaluated in that order (nothing is read for one out of range)
//   Sink: void operator()(int32_t row, int64_t i)   what winner i writes beside its output row
// A rejected candidate raises the error word (the count word then reports COUNT_ERR_RANGE) and takes no part in the set.
// The kernels are templates or static: the header is compiled into more than one object.
#pragma once
#include "common.h"
#include "sort.h"

namespace pcc {

// scratch as pcc_scan_scratch_elems(n) lays it out: slot per candidate, flags, the scan's block sums, then the error word
struct FirstRowsScratch {
    int32_t *slot_of, *flags, *block_sums, *err;
    FirstRowsScratch(int32_t* scratch, int64_t n)
        : slot_of(scratch), flags(scratch + n), block_sums(scratch + 2 * n), err(block_sums + (scan_block_sums_elems(n) - 16) + 8) {}
};

static __global__ __launch_bounds__(256) void first_rows_clear_kernel(uint64_t* __restrict__ keys, int32_t* __restrict__ vals,
                                                                      int64_t cap, int32_t* __restrict__ err) {
    if (err && blockIdx.x == 0 && threadIdx.x == 0) *err = 0;      // (null: a table built without a set, pcc_hash_build)
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
    const uint64_t slot = table_claim(keys, mask, gen.shift, pack_key(c.x, c.y, c.z, c.w));
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

// incl = inclusive scan of the winner flags: candidate i won its slot iff the scan steps at i, and its output row is incl[i] - 1.
// The winner test reads the scan, never `vals`, so the slot can be rewritten to the row id at once.
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
