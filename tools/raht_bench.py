#!/usr/bin/env python3
"""Times the RAHT operators (pcc_amd.raht: plan, forward, inverse) on the config-2 frame (850,824 voxels, 3 colour channels).

plan = Morton keys, radix sort, the closed-form per-row plan, the step buckets, and the one read of the status and offset words;
forward = the gather into Morton order plus one launch per non-empty step; inverse = a copy plus the same launches top first.
HIP events around each call, the median of --calls calls after --warmup warm-ups.  Also records whether the coefficients are
bit-equal to the numpy restatement of the tests on a 20,000-voxel cut of the frame.  Prints ONE JSON line.

--region adds "region": the kernels of the region-wise quantisation (PCR2: blocks, block levels, coefficient levels, quantise,
dequantise) timed beside the transform in the same run, and the bytes of the PCR2 stream under a two-halves map and a
camera-visibility map beside PCR1's at the two uniform levels, the bytes spent on levels, and the payload without the table
shift.  Recorded, not gated.

  python tools/raht_bench.py [--calls 20] [--warmup 5] [--commit HASH] [--region] [--out profiles/raht_bench.json]
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


def region_figures(p, co, pts, calls, warmup, qstep=4 / 255, span=24, block_log2=3):
    """--region: the level kernels and the quantiser timed beside the transform, and the bytes of the PCR2 stream for a
    two-halves map and a camera-visibility map beside PCR1's at the two uniform levels, with and without the table shift"""
    import struct
    from pcc_amd import raht, render
    from pcc_amd.entropy import _rans_encode
    from pcc_amd.q_map import visibility_score
    dev = co.device
    xyz = torch.from_numpy(pts[:, :3]).to(dev)
    lo, hi = pts[:, :3].min(axis=0), pts[:, :3].max(axis=0)
    centre, extent = (lo + hi) / 2.0, float((hi - lo).max())
    camera = render.Camera(tuple((centre + np.array([0.0, 0.0, 2.0 * extent])).tolist()), look_at=tuple(centre.tolist()), fov_y=30.0, H=1024, W=1024)
    behind, _, _ = render.camera_visibility(xyz, [camera], device=dev)
    maps = {"two_halves": (xyz[:, 0] > float(centre[0])).to(torch.float64),
            "camera_visibility": visibility_score(behind, 2, 8, 0.0).to(torch.float64)}
    steps = raht.level_steps(qstep)
    out = {"qstep_255": qstep * 255.0, "span": span, "block_log2": block_log2, "coarse_step_over_qstep": float(steps[span] / steps[0])}
    levels = raht.quality_levels(maps["two_halves"], span)
    block_of_row, n_blocks = raht.blocks(p, block_log2)
    block_level = raht.block_levels(p, levels, block_of_row, n_blocks)
    reg = raht.region(p, levels, block_log2)
    sym = raht.quantize_levels(co, reg.coeff_level, steps)
    for name, fn in (("blocks", lambda: raht.blocks(p, block_log2)),              # (with the one read of the block count)
                     ("block_levels", lambda: raht.block_levels(p, levels, block_of_row, n_blocks)),      # (with the read of its status word)
                     ("coeff_levels", lambda: raht.coeff_levels(p, block_level, block_of_row)),
                     ("quantize_levels", lambda: raht.quantize_levels(co, reg.coeff_level, steps)),     # (with the read of its status word)
                     ("dequantize_levels", lambda: raht.dequantize_levels(sym, reg.coeff_level, steps)),
                     ("quantize_uniform_torch", lambda: raht.quantize(co, qstep)),
                     ("forward_same_run", lambda: raht._transform(p, co.clone(), 0))):
        out[name + "_ms"], out[name + "_min_ms"] = timed(fn, calls, warmup)
    fine, coarse = len(raht.encode_coefficients(p, co, qstep)), len(raht.encode_coefficients(p, co, float(steps[span])))
    out["pcr1_bytes_at_qstep"], out["pcr1_bytes_at_coarse_step"] = fine, coarse
    c = int(co.shape[1])
    for name, q in maps.items():
        reg = raht.region(p, raht.quality_levels(q, span), block_log2)
        data, sym_h = raht.encode_region(p, co, qstep, reg, return_symbols=True)
        n_blocks, _, levels_len = struct.unpack("<IBI", data[20:29])
        (payload_len,) = struct.unpack("<I", data[29 + levels_len + 8 * c + 3 * p.depth * c:][:4])
        # the same symbols with one table per context and no shift by level (not a stream a decoder reads: its bytes only)
        high = np.ascontiguousarray(sym_h[1:].T).reshape(-1)
        contexts = (p.step_host()[1:][None, :] * c + np.arange(c, dtype=np.int64)[:, None]).reshape(-1)
        table = raht.choose_tables(high, contexts, 3 * p.depth * c, shift=None)
        plain = _rans_encode(high.astype(np.int32), raht._stream_indexes(p, table, c), *raht.gaussian_tables())
        levels_host = reg.host()[0]
        out[name] = {"pcr2_bytes": len(data), "n_blocks": int(n_blocks), "levels_bytes": int(levels_len), "payload_bytes": int(payload_len),
                     "payload_bytes_shift_none": len(plain), "shift_saving": 1.0 - payload_len / len(plain),
                     "rows_at_level_0": int((reg.coeff_level == 0).sum()), "block_levels_used": int(np.unique(levels_host).size)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--region", action="store_true", help="also time the region-wise quantisation kernels and record the PCR2 bytes")
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
    if args.region:
        out["region"] = region_figures(p, co, pts, args.calls, args.warmup)
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
