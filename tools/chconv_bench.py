#!/usr/bin/env python
"""Time of the channelwise window convolution (pcc_chconv, csrc/chconv.hip) as the ColorSSIM loss calls it: 32 channels
(30 maps + 2 zero columns), the Gaussian window as a [K, 1] kernel, forward (flip 0) and adjoint (flip 1), window 5, 7, 11.

The set is the union of ground-truth and predicted voxels of one training batch cut like tools/train_bench.py cuts it
(--batch 8 --block 256 from the 10-bit synthetic frame; the prediction is the seeded model's, train mode).

  python tools/chconv_bench.py [--batch 8] [--block 256] [--reps 10] [--windows 5 7 11]

One JSON line per window: ms per launch (device events, median of --reps after two warm-up launches), probes/s
(rows x K table probes), present pairs, and the bytes of the gathered feature rows (128 B per present pair) per second
against the 8 TB/s HBM peak — those rows are mostly re-read from cache (a row is read once per window it lies in), so the
figure is a rate of gathered bytes, not of HBM traffic.  Needs the GPU; there is no CPU path.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12


def union_set(batch, block, dev):
    import pcc_amd
    from pcc_amd import parallel as par, synthetic as syn
    from pcc_amd.loss import _union_map
    from pcc_amd.q_map import Q_Map
    model = syn.make_model(seed=0, device=dev)
    model.train()
    pts = syn.sphere_shell(**syn.CONFIG2, noise=0.02)
    _, rows = par.split_blocks(pts, block)
    rows = [r for r in rows if len(r) >= 2000]
    rng = random.Random(1234)
    random.seed(99)
    cs, fs = [], []
    for b, i in enumerate(rng.sample(range(len(rows)), batch)):
        p = pts[rows[i]]
        xyz = p[:, :3] - np.floor(p[:, :3].min(axis=0) / block) * block
        cs.append(np.concatenate([np.full((p.shape[0], 1), b, np.float32), xyz], axis=1))
        fs.append(p[:, 3:])
    c, f = torch.from_numpy(np.concatenate(cs)).to(dev), torch.from_numpy(np.concatenate(fs)).to(dev)
    inp = pcc_amd.SparseTensor(coordinates=c, features=f, device=dev)
    qgen = Q_Map({"mode": "exponential", "lambda_A_max": 12800, "lambda_A_min": 100, "lambda_G_max": 1600, "lambda_G_min": 25})
    Q, Lam = qgen(inp)
    with torch.no_grad():
        pred = model(inp, Q, Lam)["prediction"]
    return _union_map(inp.C, pred.C), inp.C.shape[0], pred.C.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, nargs="+", default=[5, 7, 11])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chconv_bench.py: needs the GPU (no CPU path)")
    dev = "cuda:0"
    from pcc_amd.autograd import chconv_launch
    from pcc_amd.loss import gaussian_window_3d
    umap, n_gt, n_pred = union_set(args.batch, args.block, dev)
    n = umap.n
    umap.table()
    feats = torch.rand((n, 32), dtype=torch.float32, device=dev)
    ones = torch.ones((n, 1), dtype=torch.float32, device=dev)
    print(json.dumps({"set": "union of gt and prediction", "rows": n, "gt_rows": n_gt, "prediction_rows": n_pred,
                      "batch": args.batch, "block": args.block, "device": torch.cuda.get_device_name(0)}), flush=True)
    for ks in args.windows:
        K = ks ** 3
        w = gaussian_window_3d(ks).to(dev)
        pairs = int(chconv_launch(ones, umap, torch.ones((K, 1), dtype=torch.float32, device=dev), ks, 0).double().sum().item())
        rec = {"window": ks, "channels": 32, "rows": n, "probes": n * K, "present_pairs": pairs, "pairs_per_row": pairs / n}
        for name, flip in (("forward", 0), ("adjoint", 1)):
            for _ in range(2):
                chconv_launch(feats, umap, w, ks, flip)
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                chconv_launch(feats, umap, w, ks, flip)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            ms = float(np.median(times))
            rec[name] = {"ms": ms, "ms_min": min(times), "ms_max": max(times), "probes_per_s": n * K / (ms * 1e-3),
                         "gathered_GB_per_s": pairs * 128 / (ms * 1e-3) / 1e9,
                         "gathered_share_of_8TBps": pairs * 128 / (ms * 1e-3) / HBM_PEAK}
        rec["forward_plus_adjoint_ms"] = rec["forward"]["ms"] + rec["adjoint"]["ms"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
