#!/usr/bin/env python3
"""Times pcc_amd.voxelize on the config-2 frame (850,824 points, 3 colour channels) at voxel 1 (every point its own voxel), 2
and 8 against the torch composition a user would otherwise write on the same inputs: floor(p / v), torch.unique(dim=0,
return_inverse=True) on the cell indices, index_add_ for the colour sums and the counts.  (That composition sums floats in an
order that depends on the run and returns sorted rows; the operator returns exact sums in order of first appearance.)

HIP events around each call, the median of --calls calls after --warmup warm-ups.  Prints ONE JSON line.

  python tools/voxelize_bench.py [--calls 20] [--warmup 5] [--commit HASH] [--out profiles/voxelize_bench.json]
"""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch


def timed(fn, calls, warmup):
    """median milliseconds of fn() between two HIP events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def torch_composition(P, A, voxel):
    cells = torch.floor(P / voxel).to(torch.int32)
    uniq, inverse = torch.unique(cells, dim=0, return_inverse=True)
    sums = torch.zeros((uniq.shape[0], A.shape[1]), dtype=torch.float32, device=P.device).index_add_(0, inverse, A)
    counts = torch.zeros(uniq.shape[0], dtype=torch.float32, device=P.device).index_add_(0, inverse, torch.ones_like(A[:, 0]))
    return uniq, sums / counts.unsqueeze(1), inverse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pcc_amd
    from pcc_amd import synthetic as syn
    dev = "cuda:0"
    pts = syn.sphere_shell(**syn.CONFIG2)
    P, A = torch.from_numpy(pts[:, :3]).to(dev).contiguous(), torch.from_numpy(pts[:, 3:6]).to(dev).contiguous()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    out = {"tool": "tools/voxelize_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "points": int(P.shape[0]), "channels": 3,
           "calls": args.calls, "warmup": args.warmup, "timer": "HIP events, median (and minimum) of the calls, milliseconds",
           "torch_composition": "floor(p / v).int(), torch.unique(dim=0, return_inverse=True), index_add_ of colours and counts (float32)",
           "voxel": {}}
    for voxel in (1.0, 2.0, 8.0):
        v = pcc_amd.voxelize(P, A, voxel_size=voxel)
        uniq, mean, _ = torch_composition(P, A, voxel)
        assert uniq.shape[0] == v.coords.shape[0], (uniq.shape, v.coords.shape)
        hip_ms, hip_min = timed(lambda: pcc_amd.voxelize(P, A, voxel_size=voxel), args.calls, args.warmup)
        torch_ms, torch_min = timed(lambda: torch_composition(P, A, voxel), args.calls, args.warmup)
        out["voxel"][str(voxel)] = {"voxels": int(v.coords.shape[0]), "max_points_per_voxel": int(v.counts.max()),
                                    "voxelize_ms": round(hip_ms, 4), "voxelize_min_ms": round(hip_min, 4),
                                    "torch_ms": round(torch_ms, 4), "torch_min_ms": round(torch_min, 4),
                                    "torch_over_voxelize": round(torch_ms / hip_ms, 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
