#!/usr/bin/env python3
"""Times the RAHT operators (pcc_amd.raht: plan, forward, inverse) on the config-2 frame (850,824 voxels, 3 colour channels).

plan = Morton keys, radix sort, the closed-form per-row plan, the step buckets, and the one read of the status and offset words;
forward = the gather into Morton order plus one launch per non-empty step; inverse = a copy plus the same launches top first.
HIP events around each call, the median of --calls calls after --warmup warm-ups.  Also records whether the coefficients are
bit-equal to the numpy restatement of the tests on a 20,000-voxel cut of the frame.  Prints ONE JSON line.

  python tools/raht_bench.py [--calls 20] [--warmup 5] [--commit HASH] [--out profiles/raht_bench.json]
"""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch


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
    return round(statistics.median(ms), 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pcc_amd
    from pcc_amd import raht, synthetic as syn
    dev = "cuda:0"
    pts = syn.sphere_shell(**syn.CONFIG2)
    coords = torch.from_numpy(pts[:, :3]).to(dev).to(torch.int32).contiguous()
    attrs = torch.from_numpy(pts[:, 3:6]).to(dev).to(torch.float64).contiguous()
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    p = raht.plan(coords)
    co = raht.forward(p, attrs)
    back = raht.inverse(p, co)
    source = attrs.index_select(0, p.perm.long())
    rows = np.diff(p.step_offsets)
    fold = len(rows)                                  # csrc/raht.hip: the maximal run of top steps of at most 256 rows is one launch
    while fold > 0 and rows[fold - 1] <= 256:
        fold -= 1
    if len(rows) - fold < 2:
        fold = len(rows)
    out = {"tool": "tools/raht_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "voxels": p.n, "channels": 3,
           "depth": p.depth, "steps_with_rows": int((rows > 0).sum()),
           "transform_launches": int((rows[:fold] > 0).sum()) + (1 if fold < len(rows) else 0), "steps_in_the_folded_launch": len(rows) - fold, "calls": args.calls, "warmup": args.warmup,
           "timer": "HIP events, median (and minimum) of the calls, milliseconds",
           "energy_relative_error": float(abs((co ** 2).sum() - (attrs ** 2).sum()) / (attrs ** 2).sum()),
           "inverse_max_error": float((back - source).abs().max())}
    out["plan_ms"], out["plan_min_ms"] = timed(lambda: raht.plan(coords), args.calls, args.warmup)
    out["forward_ms"], out["forward_min_ms"] = timed(lambda: raht.forward(p, attrs), args.calls, args.warmup)
    out["inverse_ms"], out["inverse_min_ms"] = timed(lambda: raht.inverse(p, co), args.calls, args.warmup)
    # against the numpy restatement of the tests (tests/_raht_reference.py), on a cut small enough for its per-row Python loop
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import _raht_reference as ref
        cut = pts[:20000]
        rp = ref.plan(cut[:, :3].astype(np.int64))
        want = ref.forward(rp, cut[:, 3:6].astype(np.float64))
        sp = raht.plan(torch.from_numpy(cut[:, :3]).to(dev).to(torch.int32))
        got = raht.forward(sp, cut[:, 3:6].astype(np.float64)).cpu().numpy()
        out["numpy_cut_voxels"] = int(cut.shape[0])
        out["numpy_bit_equal"] = bool(np.array_equal(got, want))
        out["numpy_max_abs_difference"] = float(np.abs(got - want).max())
        out["numpy_inverse_bit_equal"] = bool(np.array_equal(raht.inverse(sp, want).cpu().numpy(), ref.inverse(rp, want)))
    except ImportError:
        out["numpy_bit_equal"] = None
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
