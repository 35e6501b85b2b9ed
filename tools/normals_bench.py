#!/usr/bin/env python
"""Time of the surface normals (pcc_estimate_normals, csrc/normals.hip) on the config-2 frame (N = 850,824) at radius 2 and 3, and
of the nearest-neighbour search (pcc_nn_search, csrc/metrics.hip) on the same frame and table for comparison: both walk the
same hashed-voxel table, so their time per probe should be of one order.

  python tools/normals_bench.py [--reps 20] [--radii 2 3]

One JSON line per measurement: ms per launch (device events, median of --reps after three warm-up launches), table probes per
launch and per second, ns per probe.  The normals probe every lattice offset of the ball (33 / 123 per point at R = 2 / 3).
pcc_nn_search stops at the first shell that settles the nearest neighbour, so its probes are COUNTED here by replaying its
loop order (shells 0 and 1, a probe skipped when its offset is already farther than the best hit): the frame against itself
(every query hits at shell 0: one probe per point, the kernel's floor) and against the frame shifted by one voxel along x
(shell 1 is scanned wherever the shifted voxel is empty).  Needs the GPU; there is no CPU path.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), float(max(times))


def nn_probe_count(query, target):
    """probes pcc_nn_search makes with max_radius = 1: the replay of nn_search_kernel's loops over shells 0 and 1 for all queries
    at once (int64 [N, 3] device tensors) -> (total probes, queries resolved within shell 1)"""
    def key(p):
        return ((p[:, 0] + 8) << 42) | ((p[:, 1] + 8) << 21) | (p[:, 2] + 8)
    occupied = torch.sort(key(target)).values

    def present(p):
        k = key(p)
        pos = torch.searchsorted(occupied, k).clamp_max(occupied.numel() - 1)
        return occupied[pos] == k
    big = 1 << 40
    best = torch.where(present(query), 0, big)
    probes = query.shape[0]                                      # shell 0: one probe each
    active = best >= 1                                           # the kernel leaves before shell 1 when best < 1
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in ((-1, 1) if dx == 0 and dy == 0 else (-1, 0, 1)):
                d2 = dx * dx + dy * dy + dz * dz
                probed = active & (best >= d2)
                probes += int(probed.sum())
                hit = probed & present(query + torch.tensor([dx, dy, dz], device=query.device))
                best = torch.where(hit & (best > d2), d2, best)
    return probes, int((best < 4).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 3])
    a = ap.parse_args()
    import pcc_amd
    from pcc_amd import _lib, synthetic as syn
    from pcc_amd._lib import check, ptr
    from pcc_amd.normals import estimate_normals
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench.py needs the GPU")
    dev = "cuda:0"
    pts = syn.sphere_shell(**syn.CONFIG2)
    n = pts.shape[0]
    xyz = torch.from_numpy(pts[:, :3].astype(np.int64)).to(dev)
    coords = torch.cat([torch.zeros((n, 1), dtype=torch.int64, device=dev), xyz], dim=1).to(torch.int32).contiguous()
    cmap = pcc_amd.CoordMap(coords, 1, nbatch=1)
    keys, vals, cap = cmap.table()
    L = _lib.lib()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "n": n, "table_slots": int(cap), "reps": a.reps}))

    for R in a.radii:
        per_point = sum(1 for dx in range(-R, R + 1) for dy in range(-R, R + 1) for dz in range(-R, R + 1) if dx * dx + dy * dy + dz * dz <= R * R)
        ms, lo, hi = event_ms(lambda: estimate_normals(coords, radius=R, coord_map=cmap), a.reps)
        normals, count = estimate_normals(coords, radius=R, coord_map=cmap)
        probes = n * per_point
        print(json.dumps({"op": "estimate_normals", "radius": R, "ms": ms, "ms_min": lo, "ms_max": hi, "probes": probes,
                          "probes_per_s": probes / (ms * 1e-3), "ns_per_probe": ms * 1e6 / probes, "mean_neighbours": float(count.double().mean()),
                          "valid_share": float((normals != 0).any(dim=1).double().mean())}))

    idx = torch.empty(n, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.int64, device=dev)
    for name, shift in (("frame against itself", (0, 0, 0)), ("frame shifted by (1, 0, 0) against the frame", (1, 0, 0))):
        q_xyz = xyz + torch.tensor(shift, device=dev)
        q = torch.cat([torch.zeros((n, 1), dtype=torch.int64, device=dev), q_xyz], dim=1).to(torch.int32).contiguous()
        probes, resolved = nn_probe_count(q_xyz, xyz)
        assert resolved == n, "a query is farther than one shell from the frame"

        def search():
            check(L.pcc_nn_search(ptr(q), n, ptr(keys), ptr(vals), cap, 1, None, 1, ptr(idx), ptr(d2), None, None, _lib.stream()))
        ms, lo, hi = event_ms(search, a.reps)
        assert int((idx < 0).sum()) == 0
        print(json.dumps({"op": "nn_search", "queries": name, "ms": ms, "ms_min": lo, "ms_max": hi, "probes": probes,
                          "probes_per_point": probes / n, "probes_per_s": probes / (ms * 1e-3), "ns_per_probe": ms * 1e6 / probes}))


if __name__ == "__main__":
    main()
