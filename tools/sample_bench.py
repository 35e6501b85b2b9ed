#!/usr/bin/env python3
"""Times the back-projection of images onto points (csrc/render.hip: pcc_view_sample, pcc_camera_sample) on the config-2 shell
(850,824 voxels): the front view at 1024 x 512 and an oblique pinhole camera (tools/camera_bench.py's framing camera moved off the
axis: the same field of view and distance, looking at the shell's centre from the direction (1, 0.6, 1)) at the same size, with
1 and 4 channels, own pixels and tolerance 2.

The yardstick is the visibility walk on the same rows, in the same run of the same process: render.visibility /
render.camera_visibility (``api``) and pcc_view_visibility / pcc_camera_visibility (``entry``).  The sample kernel does the
visibility kernel's walk plus at most C image reads per pixel that counts, so the ratio says what those reads cost.  HIP events
around each call, the median of --calls calls after --warmup warm-ups (tools/normals_bench.py's timer).  No time is required of
it: the figures are written down.  Prints ONE JSON line.

  python tools/sample_bench.py [--calls 20] [--warmup 5] [--commit HASH] [--out profiles/sample_bench.json]
"""
import argparse, json, math, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
from normals_bench import event_ms
from camera_bench import FOV_Y, framing_camera

H, W = 1024, 512
DIRECTION = (1.0, 0.6, 1.0)
CASES = [(C, tol) for C in (1, 4) for tol in (None, 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pcc_amd  # noqa: F401
    from pcc_amd import _lib, render, synthetic as syn
    from pcc_amd._lib import check, ptr
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench.py needs the GPU")
    dev = "cuda:0"
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    pts = syn.sphere_shell(**syn.CONFIG2)
    cloud = torch.from_numpy(pts).to(dev)
    n = int(cloud.shape[0])
    centre, radius = (syn.CONFIG2["grid"] - 1) / 2.0, syn.CONFIG2["radius"] + syn.CONFIG2["half_width"] + 1.0
    front, up = render.VIEWS["front"]
    _, distance = framing_camera(render, centre, radius, H, W)
    unit = np.asarray(DIRECTION) / math.sqrt(sum(v * v for v in DIRECTION))
    camera = render.Camera(tuple(centre + distance * unit), look_at=(centre, centre, centre), fov_y=FOV_Y, H=H, W=W)
    q = camera.quantised()
    pos, axes = np.asarray(q.pos_q, dtype=np.int32), np.asarray(q.axes_q, dtype=np.int32).reshape(9)
    frame = render.view_frame(cloud, front, up, H, W)
    u_min, _, _, v_max, scale, ox, oy = frame
    vecs = [np.asarray(a, dtype=np.int32) for a in render.view_axes(front, up)]

    def entry(fn):
        ms, lo, hi = event_ms(fn, args.calls, args.warmup)
        return {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}

    L = _lib.lib()
    coords, _, _ = render._sorted_rows(L, cloud, cloud[:, :3].to(torch.int32), dev, colours=False)
    behind, won, depth = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    zbytes = L.pcc_render_scratch_bytes(H, W)
    zbuf = torch.empty(zbytes, dtype=torch.uint8, device=dev)
    out = {"tool": "tools/sample_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "n": n, "H": H, "W": W,
           "calls": args.calls, "warmup": args.warmup,
           "timer": "HIP events, median (minimum, maximum) of the calls, milliseconds; measured once, on one machine, at this commit",
           "view": {"front": list(front), "up": list(up), "scale": scale, "point_size": scale},
           "camera": {"direction": list(DIRECTION), "distance": round(distance, 2), "fov_y": FOV_Y, "pos_q": list(q.pos_q), "focal_q": q.focal_q},
           "api": {}, "entry": {}}
    out["api"]["visibility"] = entry(lambda: render.visibility(cloud, [(front, up)], H, W, frames=[frame]))
    out["api"]["camera_visibility"] = entry(lambda: render.camera_visibility(cloud, [camera]))
    out["entry"]["pcc_view_visibility"] = entry(lambda: check(L.pcc_view_visibility(
        ptr(coords), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, scale, H, W, ptr(zbuf), zbytes, 0, ptr(behind),
        ptr(won), _lib.stream())))
    out["entry"]["pcc_camera_visibility"] = entry(lambda: check(L.pcc_camera_visibility(
        ptr(coords), n, ptr(pos), ptr(axes), q.focal_q, q.near_q, H, W, 16, ptr(zbuf), zbytes, 0, ptr(behind), ptr(won), ptr(depth),
        _lib.stream())))
    rng = np.random.default_rng(0)
    for C, tol in CASES:
        name = "C%d_%s" % (C, "own" if tol is None else "tol%d" % tol)
        image = torch.from_numpy(rng.integers(0, 256, size=(H, W, C)).astype(np.int32)).to(dev)
        total = torch.empty((n, C), dtype=torch.int64, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        peak = torch.empty((n, C), dtype=torch.int32, device=dev)
        t = -1 if tol is None else tol
        res = {
            "api_sample_views": entry(lambda: render.sample_views(cloud, [(front, up)], [image], H, W, frames=[frame], tolerance=tol)),
            "api_sample_cameras": entry(lambda: render.sample_cameras(cloud, [camera], [image], tolerance=tol)),
            "pcc_view_sample": entry(lambda: check(L.pcc_view_sample(
                ptr(coords), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, scale, H, W, ptr(zbuf), zbytes, 0,
                ptr(image), C, t, ptr(total), ptr(count), ptr(peak), _lib.stream()))),
        }
        res["counted_view"] = int((count > 0).sum())
        res["pcc_camera_sample"] = entry(lambda: check(L.pcc_camera_sample(
            ptr(coords), n, ptr(pos), ptr(axes), q.focal_q, q.near_q, H, W, 16, ptr(zbuf), zbytes, 0, ptr(image), C, t, ptr(total),
            ptr(count), ptr(peak), _lib.stream())))
        res["counted_camera"] = int((count > 0).sum())
        res["api_view_over_visibility"] = round(res["api_sample_views"]["ms"] / out["api"]["visibility"]["ms"], 3)
        res["api_camera_over_camera_visibility"] = round(res["api_sample_cameras"]["ms"] / out["api"]["camera_visibility"]["ms"], 3)
        res["entry_view_over_visibility"] = round(res["pcc_view_sample"]["ms"] / out["entry"]["pcc_view_visibility"]["ms"], 3)
        res["entry_camera_over_camera_visibility"] = round(res["pcc_camera_sample"]["ms"] / out["entry"]["pcc_camera_visibility"]["ms"], 3)
        out[name] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
