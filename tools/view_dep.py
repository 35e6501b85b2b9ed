#!/usr/bin/env python3
"""The view-dependent / region-of-interest experiment of the reference's evaluate_view_dep.py on one frame: the frame is coded
with a uniform, a view-dependent and a region-of-interest quality map (harness.evaluate_view_dependent), every
reconstruction is rendered from a fixed view in the source's frame and compared with the source's view in YUV.  Writes
<out>/<experiment>/view_dep.csv (the reference's table, :303-305) and the four PNGs under <out>/<experiment>/renders_view/.

The frame is a PLY path or a synthetic shell ("config1", "config2", or --grid / --radius).  Seeded random weights unless
--weights is given: their rates and qualities exercise the pipeline, they are not codec quality.  The gradient and cut-off
numbers the reference keeps per sequence (:58-77) are arguments here; left out, they follow the frame's extent.

usage: view_dep.py [config1 | config2 | frame.ply] [--out DIR] [--view front|side] [--height 1024] [--width 512]
                   [--q-g 0.4] [--q-a 0.8] [--gradient AXIS LO HI] [--roi AXIS PLANE] [--weights W.pt] [--repeat N]
                   [--facing [--facing-radius 3] [--facing-floor 0.0]]     (a fourth row: quality by the angle between the
                   points' normals and the viewing direction)
                   [--visibility [--vis-views front side] [--vis-tolerance 2] [--vis-falloff 8] [--vis-floor 0.0]]     (a row
                   "visible": quality by how far a point lies behind what the views show, render.visibility; --vis-views are names
                   of the active view table, the judged view when left out)
                   [--camera X,Y,Z --look-at X,Y,Z --fov 30]     (a pinhole camera at a position in place of the axis view:
                   every image is render.render_camera's at --height x --width, --fov the full vertical angle in degrees; --look-at
                   defaults to the middle of the frame's bounding box; --visibility then asks render.camera_visibility of this camera)
                   [--anchor [--anchor-qstep Q] [--anchor-span 24]]     (one row "anchor_<key>" per row: the octree + RAHT anchor
                   codec with the row's map as region-wise quantisation, searched to the bytes of the model's row, or coded at
                   --anchor-qstep (in 1/255 units) when that is given; the CSV gains the columns codec and qstep)
                   [--screen-box R0,R1,C0,C1 | --screen-mask FILE.png | --gaze ROW,COL,RADIUS,FALLOFF] [--screen-tolerance 2]     (a row
                   "screen": quality by an image in the judged view — a box, a painted mask (an 8-bit PNG of the view's size, its first
                   channel), a gaze point — carried back to the points, render.sample_views; the CSV gains the columns psnr_roi and
                   ssim_roi, every row judged inside the region; --screen-tolerance -1 samples only the pixels that show a point)"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import pcc_amd  # noqa: E402,F401
from pcc_amd import io, render, synthetic as syn  # noqa: E402
from pcc_amd.harness import evaluate_view_dependent  # noqa: E402


def xyz(text):
    parts = text.split(",")
    if len(parts) != 3:
        raise argparse.ArgumentTypeError("three comma-separated numbers, got %r" % text)
    return tuple(float(v) for v in parts)


def numbers(count, kind):
    def parse(text):
        parts = text.split(",")
        if len(parts) != count:
            raise argparse.ArgumentTypeError("%d comma-separated numbers, got %r" % (count, text))
        return tuple(kind(v) for v in parts)
    return parse


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("frame", nargs="?", default="config1")
    ap.add_argument("--out", default=os.path.join(ROOT, "job_out", "view_dep"))
    ap.add_argument("--experiment", default="seeded")
    ap.add_argument("--view", default="front", choices=sorted(render.VIEWS))
    ap.add_argument("--mvub", action="store_true", help="the MVUB pair of views (up = +z) instead of the 8iVFB pair")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--q-g", type=float, default=0.4)
    ap.add_argument("--q-a", type=float, default=0.8)
    ap.add_argument("--gradient", nargs=3, type=float, metavar=("AXIS", "LO", "HI"))
    ap.add_argument("--roi", nargs=2, type=float, metavar=("AXIS", "PLANE"))
    ap.add_argument("--grid", type=int)
    ap.add_argument("--radius", type=float)
    ap.add_argument("--weights")
    ap.add_argument("--facing", action="store_true", help="add the facing row: quality by the normals' angle to the view's front axis")
    ap.add_argument("--facing-radius", type=int, default=3)
    ap.add_argument("--facing-floor", type=float, default=0.0)
    ap.add_argument("--visibility", action="store_true", help="add the visible row: quality by the depth behind the z-buffer front of the views")
    ap.add_argument("--vis-views", nargs="+", choices=sorted(render.VIEWS), help="views whose visibility counts (default: the judged view)")
    ap.add_argument("--vis-tolerance", type=int, default=2)
    ap.add_argument("--vis-falloff", type=int, default=8)
    ap.add_argument("--vis-floor", type=float, default=0.0)
    ap.add_argument("--camera", type=xyz, metavar="X,Y,Z", help="judge from a pinhole camera at this position instead of the axis view")
    ap.add_argument("--look-at", type=xyz, metavar="X,Y,Z", help="the point the camera looks at (default: the middle of the bounding box)")
    ap.add_argument("--fov", type=float, default=30.0, help="the camera's full vertical field of view in degrees")
    ap.add_argument("--anchor", action="store_true", help="add one anchor-codec row per row, matched to the model row's bytes")
    ap.add_argument("--anchor-qstep", type=float, help="code the anchor rows at this step (1/255 units) instead of matching bytes")
    ap.add_argument("--anchor-span", type=int, default=24, help="levels between quality 1 and quality 0 (raht.quality_levels)")
    ap.add_argument("--screen-box", type=numbers(4, int), metavar="R0,R1,C0,C1", help="add the screen row: full quality inside this box of the judged view")
    ap.add_argument("--screen-mask", metavar="FILE.png", help="add the screen row: quality from this 8-bit PNG of the judged view's size")
    ap.add_argument("--gaze", type=numbers(4, float), metavar="ROW,COL,RADIUS,FALLOFF", help="add the screen row: quality around a gaze point")
    ap.add_argument("--screen-tolerance", type=int, default=2, help="voxels behind the front a sampled pixel may lie (-1: own pixels only)")
    ap.add_argument("--repeat", type=int, default=0, help="time render_view and view_metrics over N further calls")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()

    if a.frame.lower().endswith(".ply"):
        pts = io.read_ply(a.frame)
    elif a.grid:
        pts = syn.sphere_shell(grid=a.grid, radius=a.radius or 0.25 * a.grid, half_width=0.5)
    else:
        pts = syn.sphere_shell(**{"config1": syn.CONFIG1, "config2": syn.CONFIG2}[a.frame])
    dev = a.device
    model = syn.make_model(seed=0, device=dev)
    if a.weights:
        model.load_state_dict(torch.load(a.weights, map_location=dev))
    model.update()
    data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
    view = (render.VIEWS_MVUB if a.mvub else render.VIEWS)[a.view]
    gradient = None if a.gradient is None else (int(a.gradient[0]), a.gradient[1], a.gradient[2])
    roi = None if a.roi is None else (int(a.roi[0]), a.roi[1])
    details = {}
    facing = {"radius": a.facing_radius, "floor": a.facing_floor} if a.facing else None
    visibility = None
    camera = None
    if a.look_at is not None and a.camera is None:
        ap.error("--look-at needs --camera")
    if a.camera is not None:
        if a.vis_views:
            ap.error("--vis-views are axis views: with --camera the visibility is the camera's")
        look_at = a.look_at if a.look_at is not None else tuple(((pts[:, :3].min(axis=0) + pts[:, :3].max(axis=0)) / 2.0).tolist())
        camera = render.Camera(a.camera, look_at=look_at, up=(0, 0, 1) if a.mvub else (0, 1, 0), fov_y=a.fov, H=a.height, W=a.width)
        if a.visibility:
            visibility = {"tolerance": a.vis_tolerance, "falloff": a.vis_falloff, "floor": a.vis_floor}
    elif a.visibility:
        table = render.VIEWS_MVUB if a.mvub else render.VIEWS
        visibility = {"views": [table[name] for name in (a.vis_views or [a.view])], "tolerance": a.vis_tolerance, "falloff": a.vis_falloff,
                      "floor": a.vis_floor}
    anchor = None
    if a.anchor:
        anchor = {"span": a.anchor_span}
        if a.anchor_qstep is not None:
            anchor.update(match=False, qstep=a.anchor_qstep / 255.0)
    screen = None
    if sum(v is not None for v in (a.screen_box, a.screen_mask, a.gaze)) > 1:
        ap.error("--screen-box, --screen-mask and --gaze exclude each other")
    if a.screen_box is not None:
        screen = {"box": a.screen_box}
    elif a.screen_mask is not None:
        mask = io.read_png(a.screen_mask)
        screen = {"image": mask if mask.ndim == 2 else mask[:, :, 0]}
    elif a.gaze is not None:
        screen = {"gaze": a.gaze}
    if screen is not None:
        screen["tolerance"] = None if a.screen_tolerance < 0 else a.screen_tolerance
    t0 = time.time()
    rows = evaluate_view_dependent(a.experiment, model, data, a.q_a, a.q_g, dev, a.out, view=view if a.mvub else a.view, H=a.height,
                                   W=a.width, gradient=gradient, roi=roi, save_images=True, details=details, facing=facing,
                                   visibility=visibility, camera=camera, anchor=anchor, screen=screen)
    t_all = time.time() - t0
    anchor_rows = {k: r for k, r in rows.items() if k.startswith("anchor_")}
    path = os.path.join(a.out, a.experiment, "view_dep.csv")
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["bpp", "q_a", "q_g", "key", "psnr", "ssim"] + (["codec", "qstep"] if a.anchor else [])
                           + (["psnr_roi", "ssim_roi"] if screen is not None else []),
                           extrasaction="ignore")
        w.writeheader()
        for row in rows.values():
            w.writerow(row)
    for key, row in rows.items():
        print("%-*s bpp %.4f  view psnr %.3f dB  view ssim %.5f" % (14 if a.anchor else 8, key, row["bpp"], row["psnr"], row["ssim"]))
    result = {"frame": a.frame, "n_points": int(pts.shape[0]), "H": a.height, "W": a.width, "view": a.view, "t_three_rows_s": t_all}
    if camera is not None:
        result["view"] = "camera"
        q = camera.quantised()
        result["camera"] = {"position": list(a.camera), "look_at": list(look_at), "fov_y": a.fov, "pos_q": list(q.pos_q),
                            "axes_q": [list(r) for r in q.axes_q], "focal_q": q.focal_q, "near_q": q.near_q}
    if a.facing or a.visibility or screen is not None:
        result["t_%s_rows_s" % {4: "four", 5: "five", 6: "six"}[len(rows) - len(anchor_rows)]] = result.pop("t_three_rows_s")
    if a.anchor:
        result["t_with_anchor_rows_s"] = result.pop(next(k for k in result if k.startswith("t_") and k.endswith("_rows_s")))
        result["anchor"] = {k: {"qstep_255": r["qstep"] * 255.0, "reached": r["reached"], "levels_bytes": r["levels_bytes"]}
                            for k, r in anchor_rows.items()}
    if a.visibility:
        behind = details["visibility"][0]
        result["visibility"] = {"views": ["camera"] if camera is not None else (a.vis_views or [a.view]), "tolerance": a.vis_tolerance, "falloff": a.vis_falloff, "floor": a.vis_floor,
                                "on_front": int((behind == 0).sum()), "within_tolerance": int((behind <= a.vis_tolerance).sum()),
                                "offscreen": int((behind == render.OFFSCREEN).sum())}
    if screen is not None:
        _, count, _, score = details["screen"]
        result["screen"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in screen.items() if k != "image"}
        result["screen"].update(sampled=int((count > 0).sum()), full=int((score >= 1.0).sum()), mean_score=float(score.mean()))
    if a.repeat > 0:
        src, ref_img = details["source"]
        rec, img = details["uniform"]
        front, up = view
        frame = None if camera is not None else render.view_frame(src, front, up, a.height, a.width)

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            t = time.time()
            for _ in range(a.repeat):
                fn()
            torch.cuda.synchronize()
            return (time.time() - t) / a.repeat * 1e3

        if camera is not None:
            result["render_camera_ms"] = timed(lambda: render.render_camera(rec, camera))
        else:
            result["render_view_ms"] = timed(lambda: render.render_view(rec, front, up, a.height, a.width, frame=frame))
            result["scale"] = frame[4]
        result["view_metrics_ms"] = timed(lambda: render.view_metrics(ref_img, img))
    print(json.dumps(result))
    print("wrote", path)


if __name__ == "__main__":
    main()
