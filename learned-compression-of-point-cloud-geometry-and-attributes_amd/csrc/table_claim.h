// Slot claim of the hashed-voxel table for the coordinate-set constructions that live outside coords.hip (the rotation of
// augment.hip, the voxelisation of voxelize.hip): coords.hip is part of the kernel-source stamp of the benchmark's committed
// HBM-traffic profile (bench.py, kernel_source_sha256), so operators added beside it must not edit it.  The slot walk is
// table_find's (common.h), slot for slot: the key's lane first (every 8th slot), then slot by slot.
#pragma once
#include "common.h"

namespace pcc {

// claim (or find) the slot of `key`: the mirror image of table_find, for a table of tensor stride 1.  With cap >= 2 * candidates
// a free slot exists, so the second loop always returns; mask + 1 is unreachable and the callers still guard it.
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

}  // namespace pcc
