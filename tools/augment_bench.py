#!/usr/bin/env python3
"""Time the training augmentation (ColorJitter + RandomRotate) of one batch: pcc_amd.augment.TrainAugment on the device
against a torch-CPU restatement of the same two transforms, cube by cube, the way the reference's dataset workers run them
(data/transform.py:107-130, 425-494: about twenty small tensor ops per cube for the jitter, a torch.unique(dim=0) per cube
for the rotation).  The batch: 8 cubes of edge 128 cut from the config-2 synthetic frame.

  python tools/augment_bench.py [--iters 20] [--cpu-iters 3] [--batch 8] [--block 128]

Prints one JSON line.  Both sides get the same per-item parameters; the CPU side removes duplicates (first occurrence wins),
like the device side and unlike the reference, so the two do the same work.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch


def _gray(c):
    return (0.2989 * c[:, 0] + 0.587 * c[:, 1] + 0.114 * c[:, 2]).unsqueeze(1)


def _blend(a, b, f):
    return (f * a + (1.0 - f) * b).clamp(0.0, 1.0)


def _hue(c, f):
    r, g, b = c.unbind(1)
    maxc, minc = c.max(1).values, c.min(1).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + f) % 1.0
    i = torch.floor(h * 6.0)
    t = h * 6.0 - i
    i = i.to(torch.int32) % 6
    p = (maxc * (1.0 - s)).clamp(0.0, 1.0)
    q = (maxc * (1.0 - s * t)).clamp(0.0, 1.0)
    u = (maxc * (1.0 - s * (1.0 - t))).clamp(0.0, 1.0)
    mask = i.unsqueeze(0) == torch.arange(6).view(-1, 1)
    a1 = torch.stack((maxc, q, p, p, u, maxc))
    a2 = torch.stack((u, maxc, maxc, q, p, p))
    a3 = torch.stack((p, p, u, maxc, maxc, q))
    return torch.stack([(mask * a1).sum(0), (mask * a2).sum(0), (mask * a3).sum(0)], dim=1)


def cpu_jitter(c, params, order):
    for op in order:
        f = float(params[op])
        if op == 0:
            c = _blend(c, torch.zeros_like(c), f)
        elif op == 1:
            c = _blend(c, _gray(c).mean(), f)
        elif op == 2:
            c = _blend(c, _gray(c), f)
        else:
            c = _hue(c, f)
    return c


def cpu_rotate(points, colors, R, block):
    rot = torch.mm(points.float() - block / 2, R.T) + block / 2
    rounded = torch.round(rot)
    uniq, inverse = torch.unique(rounded, dim=0, return_inverse=True)
    first = torch.full((uniq.shape[0],), rounded.shape[0], dtype=torch.long)
    first.scatter_reduce_(0, inverse, torch.arange(rounded.shape[0]), reduce="amin")
    first = first.sort().values
    return rounded[first].to(torch.int32), colors[first]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--block", type=int, default=128)
    args = ap.parse_args()
    import pcc_amd
    from pcc_amd import parallel as par, synthetic as syn
    from pcc_amd.augment import TrainAugment
    from pcc_amd.utils import sparse_collate
    dev = "cuda:0"
    cloud = syn.sphere_shell(**syn.CONFIG2)
    _, rows = par.split_blocks(cloud, args.block)
    rows = sorted(rows, key=len, reverse=True)[:args.batch]
    cubes = [cloud[r] for r in rows]
    cs = [torch.from_numpy(p[:, :3] - np.floor(p[:, :3].min(axis=0) / args.block) * args.block) for p in cubes]
    fs = [torch.from_numpy(p[:, 3:6]) for p in cubes]
    C, F = sparse_collate(cs, fs)
    Cd, Fd = C.to(dev), F.to(dev)

    aug = TrainAugment(block_size=args.block, seed=0)
    for _ in range(3):
        out = aug(Cd, Fd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out = aug(Cd, Fd)
    torch.cuda.synchronize()
    gpu_ms = (time.perf_counter() - t0) / args.iters * 1e3

    draws = TrainAugment(block_size=args.block, seed=0).draw([c.shape[0] for c in cs])
    cpu_rows = 0
    t0 = time.perf_counter()
    for _ in range(args.cpu_iters):
        cpu_rows = 0
        for i, (c, f) in enumerate(zip(cs, fs)):
            f2 = cpu_jitter(f.float(), draws[0][i], [int(v) for v in draws[1][i]])
            c2, f2 = cpu_rotate(c, f2, torch.from_numpy(draws[2][i].reshape(3, 3)), args.block)
            cpu_rows += c2.shape[0]
    cpu_ms = (time.perf_counter() - t0) / args.cpu_iters * 1e3
    print(json.dumps({"bench": "augment", "items": len(cs), "points": int(C.shape[0]), "rows_out": int(out[0].shape[0]),
                      "cpu_rows_out": cpu_rows, "device_ms": round(gpu_ms, 3), "torch_cpu_ms": round(cpu_ms, 3),
                      "cpu_threads": torch.get_num_threads()}))


if __name__ == "__main__":
    main()
