#!/usr/bin/env python3
"""Times render.visibility (csrc/render.hip, pcc_view_visibility) on the config-2 shell (850,824 points) at 1024 x 512 for one view
(front) and for two (front and the opposite view), beside render.render_view on the same frame: both do the renderer's clear and
splat; visibility then reads each point's splat once more where the renderer resolves the pixels to colours.

Two kinds of figures.  ``api``: the Python calls as a user makes them (they sort the rows canonically, frame the cloud, allocate).
``entry``: the C entries alone on rows already sorted and a frame already known — the three launches of pcc_view_visibility
against the three of pcc_render_view.  HIP events around each call, the median of --calls calls after --warmup warm-ups
(tools/normals_bench.py's timer).  No time is required of it: the figures are written down.

Also recorded: how many points lie on the z-buffer front, within the default tolerance of it, and off-screen (the shell is 521
voxels across and the image 512 wide, so its rim is cut), and the rates of the "uniform" and "visible" rows of
harness.evaluate_view_dependent on this frame.  Those rates come from SEEDED weights: they exercise the pipeline and have no
rate-distortion meaning.  Prints ONE JSON line.

  python tools/visibility_bench.py [--calls 20] [--warmup 3] [--commit HASH] [--out profiles/visibility_bench.json] [--no-rows]
"""
import argparse, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
from normals_bench import event_ms

H, W = 1024, 512
TOLERANCE = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD when there is a work tree)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-rows", action="store_true", help="skip the two coded rows (times and counts only)")
    args = ap.parse_args()
    import pcc_amd  # noqa: F401
    from pcc_amd import _lib, render, synthetic as syn
    from pcc_amd._lib import check, ptr
    if not torch.cuda.is_available():
        raise SystemExit("visibility_bench.py needs the GPU")
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
    front, up = render.VIEWS["front"]
    back = (tuple(-a for a in front), up)
    frame = render.view_frame(cloud, front, up, H, W)
    out = {"tool": "tools/visibility_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit, "n": n, "H": H, "W": W,
           "scale": frame[4], "point_size": frame[4], "calls": args.calls, "warmup": args.warmup,
           "timer": "HIP events, median (minimum, maximum) of the calls, milliseconds; measured once, on one machine, at this commit"}

    def entry(fn):
        ms, lo, hi = event_ms(fn, args.calls, args.warmup)
        return {"ms": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}

    back_frame = render.view_frame(cloud, back[0], back[1], H, W)
    out["api"] = {                                     # every call is given its frames: framing (two reductions and a read-back) is not timed
        "render_view": entry(lambda: render.render_view(cloud, front, up, H, W, frame=frame)),
        "visibility_one_view": entry(lambda: render.visibility(cloud, [(front, up)], H, W, frames=[frame])),
        "visibility_two_views": entry(lambda: render.visibility(cloud, [(front, up), back], H, W, frames=[frame, back_frame])),
        "visibility_two_views_framing_itself": entry(lambda: render.visibility(cloud, [(front, up), back], H, W)),
    }

    # the entries alone: rows sorted once, the frames known, every buffer allocated
    L = _lib.lib()
    coords, rgb8, _ = render._sorted_rows(L, cloud, cloud[:, :3].to(torch.int32), dev, colours=True)
    zbytes = L.pcc_visibility_scratch_bytes(H, W)
    zbuf = torch.empty(zbytes, dtype=torch.uint8, device=dev)
    image = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    behind, won = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    bg = np.full(3, 255, dtype=np.uint8)
    frames = {"front": ((front, up), frame), "back": (back, back_frame)}

    def vis(name, accumulate):
        (f, u), fr = frames[name]
        vecs = [np.asarray(a, dtype=np.int32) for a in render.view_axes(f, u)]
        u_min, _, _, v_max, scale, ox, oy = fr
        check(L.pcc_view_visibility(ptr(coords), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, scale, H, W,
                                    ptr(zbuf), zbytes, accumulate, ptr(behind), ptr(won), _lib.stream()))

    def draw():
        vecs = [np.asarray(a, dtype=np.int32) for a in render.view_axes(front, up)]
        u_min, _, _, v_max, scale, ox, oy = frame
        check(L.pcc_render_view(ptr(coords), ptr(rgb8), n, ptr(vecs[0]), ptr(vecs[1]), ptr(vecs[2]), u_min, v_max, ox, oy, scale, scale, H, W,
                                ptr(bg), ptr(zbuf), zbytes, ptr(image), _lib.stream()))

    out["entry"] = {
        "pcc_render_view": entry(draw),
        "pcc_view_visibility_one_view": entry(lambda: vis("front", 0)),
        "pcc_view_visibility_two_views": entry(lambda: (vis("front", 0), vis("back", 1))),
    }
    out["entry"]["one_view_over_render_view"] = round(out["entry"]["pcc_view_visibility_one_view"]["ms"] / out["entry"]["pcc_render_view"]["ms"], 3)
    out["api"]["one_view_over_render_view"] = round(out["api"]["visibility_one_view"]["ms"] / out["api"]["render_view"]["ms"], 3)

    for name, views in (("one_view", [(front, up)]), ("two_views", [(front, up), back])):
        b, w = render.visibility(cloud, views, H, W)
        out["counts_" + name] = {"on_front": int((b == 0).sum()), "within_tolerance_%d" % TOLERANCE: int((b <= TOLERANCE).sum()),
                                 "offscreen": int((b == render.OFFSCREEN).sum()), "pixels_won": int(w.sum())}

    if not args.no_rows:
        from pcc_amd.harness import evaluate_view_dependent
        model = syn.make_model(seed=0, device=dev)
        model.update()
        data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
        with tempfile.TemporaryDirectory() as tmp:
            rows = evaluate_view_dependent("bench", model, data, 0.8, 0.4, dev, tmp, view="front", H=H, W=W, visibility={"views": ["front"]})
        out["rows"] = {"note": "SEEDED weights: these rates exercise the pipeline and have no rate-distortion meaning", "q_a": 0.8, "q_g": 0.4,
                       "tolerance": TOLERANCE, "falloff": 8, "floor": 0.0,
                       "uniform_bpp": rows["uniform"]["bpp"], "visible_bpp": rows["visible"]["bpp"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
