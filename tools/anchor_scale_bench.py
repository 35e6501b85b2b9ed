#!/usr/bin/env python3
"""Times the position scaling of the anchor codec (pcc_amd.rescale, csrc/rescale.hip) on the config-2 frame (850,824 points, 3
colour channels) at the four scales of anchor.GPCC_POINTS: pcc_scaled_cells, pcc_scaled_transfer (the lattice walk), and the SAME
association obtained the way the tree could before the walk existed — metrics.nearest_neighbours of the source into a CoordMap of
the reconstructed positions (pcc_nn_search: (2r+1)^3 hash probes per point behind a retry schedule of radii), table build included
— then anchor.compress / decompress at the point's qstep, and bpp, D1 and Y-PSNR against the original frame for both transfers.

HIP events around each call, the median of --calls calls after --warmup warm-ups.  Prints ONE JSON line.

  python tools/anchor_scale_bench.py [--calls 10] [--warmup 2] [--commit HASH] [--out profiles/anchor_scale_bench.json]
"""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def timed(fn, calls, warmup):
    """median (and minimum) milliseconds of fn() between two HIP events"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pcc_amd import CoordMap, anchor, rescale, synthetic as syn
    from pcc_amd.metrics import PointCloudMetric, nearest_neighbours
    dev = "cuda:0"
    pts = syn.sphere_shell(**syn.CONFIG2)
    X = torch.from_numpy(pts).to(dev).contiguous()
    n = int(X.shape[0])
    xyz = torch.round(X[:, :3]).to(torch.int32)
    C = torch.cat([torch.zeros_like(xyz[:, :1]), xyz], dim=1).contiguous()
    A = X[:, 3:6].contiguous()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    out = {"tool": "tools/anchor_scale_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "points": n, "channels": 3,
           "calls": args.calls, "warmup": args.warmup, "timer": "HIP events, median (and minimum) of the calls, milliseconds",
           "nn_search": "metrics.nearest_neighbours(source, CoordMap(positions)): hash build of the positions + pcc_nn_search over its "
                        "retry schedule of radii; the same (nearest, d2) as pcc_scaled_transfer, without the colour sums",
           "resolution": 1023, "scale": {}}
    for scale, qp in anchor.GPCC_POINTS:
        num, den = rescale.as_scale(scale)
        qstep = anchor.qp_to_qstep(qp)
        cells, _, _, _, _, table = rescale.scaled_cells(C, A, num, den)
        m = int(cells.shape[0])
        nearest, d2, counts, _ = rescale.scaled_transfer(C, A, num, den, table, m)
        recon = torch.cat([cells[:, :1], rescale.positions_of(cells[:, 1:4], num, den)], dim=1).contiguous()

        def parents_way():
            return nearest_neighbours(C, CoordMap(recon, 1))

        idx, nn_d2, _, _ = parents_way()
        assert torch.equal(idx, nearest) and torch.equal(nn_d2, d2)
        cells_ms, cells_min = timed(lambda: rescale.scaled_cells(C, A, num, den), args.calls, args.warmup)
        walk_ms, walk_min = timed(lambda: rescale.scaled_transfer(C, A, num, den, table, m), args.calls, args.warmup)
        nn_ms, nn_min = timed(parents_way, max(3, args.calls // 3), 1)
        entry = {"num": num, "den": den, "qp": qp, "qstep_255": round(qstep * 255, 4), "cells": m, "empty_cells": int((counts == 0).sum()),
                 "max_d2": int(d2.max()), "scaled_cells_ms": round(cells_ms, 4), "scaled_cells_min_ms": round(cells_min, 4),
                 "scaled_transfer_ms": round(walk_ms, 4), "scaled_transfer_min_ms": round(walk_min, 4),
                 "nn_search_ms": round(nn_ms, 4), "nn_search_min_ms": round(nn_min, 4), "nn_search_over_transfer": round(nn_ms / walk_ms, 3)}
        for transfer in rescale.TRANSFERS:
            stream = anchor.compress(X, qstep, scale=(num, den), transfer=transfer)
            rec = anchor.decompress(stream, dev)
            res, _ = PointCloudMetric(X, rec, resolution=1023, device=dev).compute_pointcloud_metrics(drop_duplicates=True)
            enc_ms, _ = timed(lambda: anchor.compress(X, qstep, scale=(num, den), transfer=transfer), max(3, args.calls // 3), 1)
            dec_ms, _ = timed(lambda: anchor.decompress(stream, dev), max(3, args.calls // 3), 1)
            entry[transfer] = {"bytes": len(stream), "bpp": round(len(stream) * 8 / n, 5), "d1_psnr": round(res["sym_psnr_mse"], 4),
                               "y_psnr": round(res["sym_y_psnr"], 4), "ab_y_psnr": round(res["AB_y_psnr"], 4),
                               "ba_y_psnr": round(res["BA_y_psnr"], 4), "compress_ms": round(enc_ms, 3), "decompress_ms": round(dec_ms, 3)}
        out["scale"]["%d/%d" % (num, den)] = entry
        print("%d/%d: %s" % (num, den, json.dumps(entry)), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
