#!/usr/bin/env python3
"""Times the camera views (csrc/render.hip: pcc_render_camera, pcc_camera_visibility) on the config-2 shell (850,824 voxels) at
1024 x 512 and at 2048 x 2048, for a camera with a vertical field of view of 30 degrees on the +z axis through the shell's
centre, far enough to frame the whole body.  The yardstick is the orthographic pair on the same rows, the front view at the
same image size, timed in the same run of the same process: render.render_view / render.visibility, whose kernels this feature
leaves as they were.

Two kinds of figures, as tools/visibility_bench.py.  ``api``: the Python calls as a user makes them (they sort the rows, allocate;
the orthographic ones are given their frame).  ``entry``: the C entries alone on rows already sorted.  HIP events around each
call, the median of --calls calls after --warmup warm-ups (tools/normals_bench.py's timer).

What the splat's cost scales with is its atomics: s^2 per drawn point for the camera (s: the projected voxel edge, 1 .. 16),
point_size^2 per point for the orthographic view.  ``mean_s`` and both atomic counts are worked out on the host from the same
integers the kernels use, so the times can be held against the ratio of the counts.  No time is required of it: the figures
are written down.  Prints ONE JSON line.

  python tools/camera_bench.py [--calls 20] [--warmup 5] [--commit HASH] [--out profiles/camera_bench.json]
"""
import argparse, json, math, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
from normals_bench import event_ms

SIZES = ((1024, 512), (2048, 2048))
FOV_Y = 30.0
MARGIN = 0.95            # the body fills this share of the narrower half-angle


def framing_camera(render, centre, radius, H, W):
    """on the +z axis through ``centre``, looking back at it, at the distance from which a sphere of ``radius`` fills MARGIN of
    the narrower of the two half-angles of the image"""
    half_v = math.radians(FOV_Y) / 2.0
    half_h = math.atan(math.tan(half_v) * W / H)
    distance = radius / math.sin(MARGIN * min(half_v, half_h))
    return render.Camera((centre, centre, centre + distance), look_at=(centre, centre, centre), fov_y=FOV_Y, H=H, W=W), distance


def splat_sizes(xyz, camera, ps_q=16):
    """s of every drawn point (int64 numpy), from the integers of include/pcc_hip.h's projection"""
    q = camera.quantised()
    e = 16 * xyz.astype(np.int64) - np.asarray(q.pos_q, dtype=np.int64)
    D = -(e @ np.asarray(q.axes_q[2], dtype=np.int64))
    D = D[D >= q.near_q * 2 ** 14]
    return np.clip(-((-(q.focal_q * ps_q * 1024)) // D), 1, 16)


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
        raise SystemExit("camera_bench.py needs the GPU")
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
    out = {"tool": "tools/camera_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "n": n, "fov_y": FOV_Y,
           "calls": args.calls, "warmup": args.warmup,
           "timer": "HIP events, median (minimum, maximum) of the calls, milliseconds; measured once, on one machine, at this commit",
           "sizes": {}}

    def entry(fn):
        ms, lo, hi = event_ms(fn, args.calls, args.warmup)
        return {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}

    # rows sorted once for the entries
    L = _lib.lib()
    coords, rgb8, _ = render._sorted_rows(L, cloud, cloud[:, :3].to(torch.int32), dev, colours=True)
    behind, won, depth = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    bg = np.full(3, 255, dtype=np.uint8)
    xyz = pts[:, :3].astype(np.int64)

    for H, W in SIZES:
        camera, distance = framing_camera(render, centre, radius, H, W)
        q = camera.quantised()
        pos, axes = np.asarray(q.pos_q, dtype=np.int32), np.asarray(q.axes_q, dtype=np.int32).reshape(9)
        frame = render.view_frame(cloud, front, up, H, W)
        u_min, _, _, v_max, scale, ox, oy = frame
        vecs = [np.asarray(a, dtype=np.int32) for a in render.view_axes(front, up)]
        zbytes = L.pcc_render_scratch_bytes(H, W)
        zbuf = torch.empty(zbytes, dtype=torch.uint8, device=dev)
        image = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        s = splat_sizes(xyz, camera)
        res = {"camera": {"distance": round(distance, 2), "focal": round(camera.focal, 3), "pos_q": list(q.pos_q), "focal_q": q.focal_q},
               "orthographic": {"scale": scale, "point_size": scale},
               "drawn": int(s.shape[0]), "mean_s": round(float(s.mean()), 4), "max_s": int(s.max()),
               "atomics_camera": int((s * s).sum()), "atomics_orthographic": n * scale * scale}
        res["atomics_ratio"] = round(res["atomics_camera"] / res["atomics_orthographic"], 4)
        res["api"] = {
            "render_camera": entry(lambda: render.render_camera(cloud, camera)),
            "camera_visibility": entry(lambda: render.camera_visibility(cloud, [camera])),
            "render_view": entry(lambda: render.render_view(cloud, front, up, H, W, frame=frame)),
            "visibility": entry(lambda: render.visibility(cloud, [(front, up)], H, W, frames=[frame])),
        }
        res["entry"] = {
            "pcc_render_camera": entry(lambda: check(L.pcc_render_camera(
                ptr(coords), ptr(rgb8), n, ptr(pos), ptr(axes), q.focal_q, q.near_q, H, W, 16, ptr(bg), ptr(zbuf), zbytes, ptr(image),
                _lib.stream()))),
            "pcc_camera_visibility": entry(lambda: check(L.pcc_camera_visibility(
                ptr(coords), n, ptr(pos), ptr(axes), q.focal_q, q.near_q, H, W, 16, ptr(zbuf), zbytes, 0, ptr(behind), ptr(won), ptr(depth),
                _lib.stream()))),
            "pcc_render_view": entry(lambda: check(L.pcc_render_view(
                ptr(coords), ptr(rgb8), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, scale, H, W, ptr(bg),
                ptr(zbuf), zbytes, ptr(image), _lib.stream()))),
            "pcc_view_visibility": entry(lambda: check(L.pcc_view_visibility(
                ptr(coords), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, scale, H, W, ptr(zbuf), zbytes, 0,
                ptr(behind), ptr(won), _lib.stream()))),
        }
        for kind, cam_name, ortho_name in (("api", "render_camera", "render_view"), ("api", "camera_visibility", "visibility"),
                                           ("entry", "pcc_render_camera", "pcc_render_view"),
                                           ("entry", "pcc_camera_visibility", "pcc_view_visibility")):
            res[kind][cam_name + "_over_" + ortho_name] = round(res[kind][cam_name]["ms"] / res[kind][ortho_name]["ms"], 3)
        b, w, d = render.camera_visibility(cloud, [camera])
        res["counts"] = {"on_front": int((b == 0).sum()), "offscreen": int((b == render.OFFSCREEN).sum()), "pixels_won": int(w.sum()),
                         "depth_min": int(d.min()), "depth_max": int(d[d != render.OFFSCREEN].max())}
        out["sizes"]["%dx%d" % (H, W)] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
