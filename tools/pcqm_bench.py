#!/usr/bin/env python3
"""Times pcqm_voxel (pcc_amd/pcqm.py, csrc/pcqm.hip) on the config-2 frame (850,824 points) against its own reconstruction by the
seeded model, at the radii its bounding box implies (the shell's side is 521 voxels: radius 2, neighbourhood 4) and at the (4, 8)
of a 10-bit frame that fills its grid: the two kappa launches, the feature launch, the whole call, and once the nearest-neighbour
search and the colour conversion.  (The seeded weights decode points up to 40 voxels from the source, so the search widens
to its 128-voxel shell and dominates the whole call; that is the search's time on this pair, not the metric's.)

The feature kernel probes both balls of every source point: 2 x 2,109 table probes per point at neighbourhood 8.  Its probes
per second stand beside those of pcc_estimate_normals at radius 8 on the same frame and table, measured in the same run with
tools/normals_bench.py's timer: the only yardstick this repository has for a probe-bound kernel (the normals kernel gathers
nothing; the feature kernel reads 7 or 5 doubles behind every hit).

HIP events around each call, the median of --calls calls after --warmup warm-ups.  No time is required of it: the figures are
written down.  Prints ONE JSON line.

  python tools/pcqm_bench.py [--calls 3] [--warmup 1] [--commit HASH] [--out profiles/pcqm_bench.json]
"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from normals_bench import event_ms


def ball_size(R):
    return sum(1 for dx in range(-R, R + 1) for dy in range(-R, R + 1) for dz in range(-R, R + 1) if dx * dx + dy * dy + dz * dz <= R * R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pcc_amd
    from pcc_amd import metrics, pcqm, synthetic as syn
    from pcc_amd.normals import estimate_normals
    if not torch.cuda.is_available():
        raise SystemExit("pcqm_bench.py needs the GPU")
    dev = "cuda:0"
    model = syn.make_model(0, dev)
    model.update()
    pts = syn.sphere_shell(**syn.CONFIG2)
    qc, qf = syn.uniform_qmap(pts[:, :3], 0.5, 0.5)
    x = torch.from_numpy(pts).to(dev)
    Q = pcc_amd.SparseTensor(coordinates=torch.from_numpy(qc).to(dev), features=torch.from_numpy(qf).to(dev), device=dev)
    strings, shape, k, coords = model.compress(x, Q)
    rec = model.decompress(coordinates=coords, strings=strings, shape=shape, k=k)
    torch.cuda.synchronize()

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    sc, srgb = metrics._drop_duplicated_points(*metrics._as_cloud(x, dev))
    rc, rrgb = metrics._drop_duplicated_points(*metrics._as_cloud(rec, dev))
    smap, rmap = pcc_amd.CoordMap(sc, 1, nbatch=1), pcc_amd.CoordMap(rc, 1, nbatch=1)
    smap.table(), rmap.table()
    radius, h = pcqm.default_radii(sc)
    n_r, n_d = int(sc.shape[0]), int(rc.shape[0])
    out = {"tool": "tools/pcqm_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "n_source": n_r, "n_reconstruction": n_d,
           "radius": radius, "neighbourhood": h, "calls": args.calls, "warmup": args.warmup,
           "timer": "HIP events, median (minimum, maximum) of the calls, milliseconds; measured once, on one machine, at this commit"}

    def entry(fn, probes=None):
        ms, lo, hi = event_ms(fn, args.calls, args.warmup)
        e = {"ms": round(ms, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
        if probes:
            e.update(probes=probes, probes_per_s=probes / (ms * 1e-3), ns_per_probe=ms * 1e6 / probes)
        return e

    out["nn_search"] = entry(lambda: metrics.nearest_neighbours(sc, rmap))
    nn, nn_d2 = metrics.nearest_neighbours(sc, rmap)[:2]
    out["nn_search"]["largest_squared_distance"] = int(nn_d2.max())
    out["lab_planes_both"] = entry(lambda: (pcqm.lab_planes(srgb), pcqm.lab_planes(rrgb)))
    # the yardstick: the normals kernel at radius 8 on the source's table (csrc/normals.hip; its code is the parent commit's,
    # the moment loop and the Jacobi only moved into csrc/ball_moments.h)
    out["estimate_normals_radius_8"] = entry(lambda: estimate_normals(sc, radius=8, coord_map=smap), n_r * ball_size(8))
    metric = metrics.PointCloudMetric(x, rec, device=dev)
    out["at"] = {}
    # the radii the frame's bounding box implies, and the (4, 8) of a 10-bit frame that fills its grid
    for r, nb in dict.fromkeys([(radius, h), (4, 8)]):
        e = out["at"]["radius_%d_neighbourhood_%d" % (r, nb)] = {}
        e["surface_variation_source"] = entry(lambda: pcqm.surface_variation(sc, r, smap), n_r * ball_size(r))
        e["surface_variation_reconstruction"] = entry(lambda: pcqm.surface_variation(rc, r, rmap), n_d * ball_size(r))
        attrs_r, attrs_d = pcqm._attribute_planes(sc, srgb, smap, r), pcqm._attribute_planes(rc, rrgb, rmap, r)
        e["features"] = entry(lambda: pcqm.pcqm_features(sc, smap, attrs_r, rc, rmap, attrs_d, nn, nb, want_features=False),
                              2 * n_r * ball_size(nb))
        e["whole_call"] = entry(lambda: pcqm.pcqm_voxel(x, rec, radius=r, neighbourhood=nb))
        e["compute_pcqm_on_a_built_metric"] = entry(lambda: metric.compute_pcqm(radius=r, neighbourhood=nb))
        e["result"] = metric.compute_pcqm(radius=r, neighbourhood=nb)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
