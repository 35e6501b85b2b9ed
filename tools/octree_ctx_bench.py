#!/usr/bin/env python3
"""Rate and time of the octree coordinate coder with neighbour contexts ("PCO2") against the default stream ("PCO1"), in one run:
on the full-resolution geometry of the config-2 frame (the anchor codec's case) and on its stride-8 latent coordinates (file
mode's case).  Per cloud: bytes and bits per point of both streams, the mode PCO2 chose per level, encode and decode time of both
(median of --runs synchronised runs after --warmup), and the size of the file-mode bitstream with either coder.

  python tools/octree_ctx_bench.py [--runs 7] [--warmup 2] [--out profiles/octree_ctx_bench.json]

The yardstick is PCO1 in the same process.  Every decode is checked against the encoder's input (as a set) before it is timed.
"""
import argparse, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch


def timed(fn, runs, warmup):
    """median wall time of fn() in ms, each run between two device synchronisations"""
    times = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 3), [round(t, 3) for t in times]


def same_set(a, b):
    key = lambda t: torch.sort((t[:, 1].long() << 42) | (t[:, 2].long() << 21) | t[:, 3].long()).values
    return a.shape == b.shape and bool(torch.equal(key(a - a.amin(0)), key(b - b.amin(0))))


def measure(octree, coords, stride, runs, warmup):
    n = int(coords.shape[0])
    row = {"points": n, "stride": stride}
    for name, contexts in (("pco1", False), ("pco2", True)):
        data = octree.encode_coordinates(coords, stride, contexts=contexts)
        if not same_set(octree.decode_coordinates(data, coords.device), coords):
            raise SystemExit(f"{name}: the decoded coordinates are not the input")
        enc, enc_all = timed(lambda: octree.encode_coordinates(coords, stride, contexts=contexts), runs, warmup)
        dec, dec_all = timed(lambda: octree.decode_coordinates(data, coords.device), runs, warmup)
        row[name] = {"bytes": len(data), "bits_per_point": round(len(data) * 8 / n, 4), "encode_ms": enc, "decode_ms": dec,
                     "encode_ms_runs": enc_all, "decode_ms_runs": dec_all}
        if contexts:
            row[name]["depth"] = data[4]
            row[name]["modes"] = octree.level_modes(data)
    row["bytes_ratio"] = round(row["pco2"]["bytes"] / row["pco1"]["bytes"], 4)
    row["encode_time_ratio"] = round(row["pco2"]["encode_ms"] / row["pco1"]["encode_ms"], 3)
    row["decode_time_ratio"] = round(row["pco2"]["decode_ms"] / row["pco1"]["decode_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "octree_ctx_bench.json"))
    args = ap.parse_args()
    if args.runs < 5 or args.warmup < 2:
        raise SystemExit("at least 5 runs after 2 warm-ups")
    import pcc_amd
    from pcc_amd import octree, synthetic as syn
    if not torch.cuda.is_available():
        raise SystemExit("octree_ctx_bench needs the GPU: there is no CPU path to time")
    dev = "cuda:0"
    pts = syn.sphere_shell(**syn.CONFIG2)
    x = torch.from_numpy(pts).to(dev)
    full = torch.cat([torch.zeros((x.shape[0], 1), dtype=torch.int32, device=dev), x[:, :3].round().to(torch.int32)], dim=1).contiguous()
    model = syn.make_model(0, dev)
    model.update()
    qc, qf = syn.uniform_qmap(pts[:, :3], 0.5, 0.5)

    def q_map():
        return pcc_amd.SparseTensor(coordinates=torch.from_numpy(qc).to(dev), features=torch.from_numpy(qf).to(dev), device=dev)

    latent = model.compress(x, q_map())[3].to(torch.int32).contiguous()
    out = {"bench": "octree_ctx", "frame": "config-2 sphere shell", "runs": args.runs, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0),
           "geometry": measure(octree, full, 1, args.runs, args.warmup),
           "latent": measure(octree, latent, model.LATENT_STRIDE, args.runs, args.warmup)}
    file_mode = {}
    with tempfile.TemporaryDirectory() as td:
        for coder in ("pco1", "pco2"):
            model.coord_coder = coder
            path = os.path.join(td, coder + ".bin")
            model.compress(x, q_map(), path=path)
            rec = model.decompress(path=path)
            file_mode[coder] = {"bytes": os.path.getsize(path), "bpp": round(os.path.getsize(path) * 8 / pts.shape[0], 5),
                                "n_decoded": int(rec.shape[0])}
    model.coord_coder = "pco1"
    out["file_mode"] = file_mode
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
