#!/usr/bin/env python3
"""Times one probe of the target-rate search (ColorModel.estimate_bits) against one full ColorModel.compress, and a whole
rate_control.compress_to_target, on the 4,904-point frame (config 1) and the 850,824-point frame (config 2).

Seeded q-responsive weights (synthetic.FILM_GAIN_Q_RESPONSIVE, as tools/rd_sweep.py).  Probe and compress alternate inside one
loop of one process, at q = (0.4, 0.8); each is timed twice over: HIP events around the call, and the host clock around the call
and a device synchronise (both calls read from the device, so the two agree up to the launch of the first kernel).  Median and
minimum of --calls calls after --warmup warm-ups of both.  compress_to_target is timed on the host clock alone, at the target
half-way between the estimates of the two ends, and its probe count recorded.  Also records that every real stream length lay
inside the probe's interval.  Prints ONE JSON line per frame; --out writes them as a JSON list.

  python tools/rate_control_bench.py [--calls 15] [--warmup 3] [--frames config1 config2] [--commit HASH] [--out profiles/rate_control_bench.json]
"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def once(fn):
    """(event milliseconds, host milliseconds) of one fn() that ends in a device synchronise"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", nargs="+", default=["config1", "config2"], choices=["config1", "config2"])
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pcc_amd
    from pcc_amd import synthetic as syn
    from pcc_amd.rate_control import compress_to_target
    dev = "cuda:0"
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    model = syn.make_model(seed=0, device=dev, film_gain=syn.FILM_GAIN_Q_RESPONSIVE)
    model.update()
    rows = []
    for name in args.frames:
        pts = syn.sphere_shell(**getattr(syn, name.upper()))
        x = torch.from_numpy(pts).to(dev)

        def qmap(q):
            qc, qf = syn.uniform_qmap(pts[:, :3], *q)
            return pcc_amd.SparseTensor(coordinates=torch.from_numpy(qc).to(dev), features=torch.from_numpy(qf).to(dev), device=dev)

        q = (0.4, 0.8)
        Q = qmap(q)
        probe = lambda: model.estimate_bits(x, Q)
        code = lambda: model.compress(x, Q)
        for _ in range(args.warmup):
            probe(), code()
        pe, ph, ce, ch = [], [], [], []
        for _ in range(args.calls):                      # alternating: both see the same clocks and the same neighbours
            a, b = once(probe)
            pe.append(a), ph.append(b)
            a, b = once(code)
            ce.append(a), ch.append(b)
        est = probe()
        strings = code()[0]
        ly, lz = len(strings[0][0]), len(strings[1][0])
        ends = [model.estimate_bits(x, qmap(e))["bytes"][1] for e in ((0.0, 0.0), (1.0, 1.0))]
        target = (ends[0] + ends[1]) // 2
        found = compress_to_target(model, x, target_bytes=target)              # (warm-up: the maps of every probed q exist afterwards)
        whole = []
        for _ in range(max(3, args.calls // 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            found = compress_to_target(model, x, target_bytes=target)
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
        row = {"tool": "tools/rate_control_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "frame": name,
               "points": int(pts.shape[0]), "q": q, "calls": args.calls, "warmup": args.warmup,
               "timer": "per call: HIP events, and the host clock around the call plus a device synchronise; probe and compress alternate in one loop",
               "baseline": "compress of the same commit; this change leaves compress as its parent's",
               "probe_events": stats(pe), "probe_host": stats(ph), "compress_events": stats(ce), "compress_host": stats(ch),
               "compress_over_probe_host_median": round(statistics.median(ch) / statistics.median(ph), 3),
               "estimate": {k: est[k] for k in ("y", "z", "bytes", "escapes")}, "stream_bytes": {"y": ly, "z": lz},
               "stream_inside_interval": bool(est["y"][0] <= ly <= est["y"][1] and est["z"][0] <= lz <= est["z"][1]),
               "search": {"ends_upper_bytes": ends, "target_bytes": target, "probes": len(found["log"]), "reached": found["reached"],
                          "t": found["t"], "estimate": found["estimate"], "bytes": found["bytes"], "host": stats(whole),
                          "runs": len(whole)}}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
