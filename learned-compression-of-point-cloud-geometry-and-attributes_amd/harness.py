"""Evaluation harness: one frame through file-mode compress / decompress with the reference's timing
bracket (mirror of ``compress_model_ours``, /root/reference/utils.py:418-472, as driven by
evaluate.py:55-216), plus the quality numbers the sweep records.

Differences in form only: clouds are ``[N, 6]`` GPU tensors instead of open3d objects, and the
metrics come from metrics.PointCloudMetric on the GPU instead of the external ``pc_error`` binary
(utils.py:206-290) — same quantities (D1 / Y / U / V PSNR, symmetric = worse direction).

``evaluate_view_dependent`` mirrors the rows of evaluate_view_dep.py:139-301: one frame coded with a uniform, a
view-dependent and a region-of-interest quality map, each judged by rendering a fixed view (render.render_view instead
of an open3d window) and comparing it with the source's view in YUV (render.view_metrics instead of scikit-image).
"""
import os
import time

import numpy as np
import torch

from . import render
from .io import write_png
from .metrics import PointCloudMetric
from .normals import estimate_normals
from .q_map import box_image, facing_score, gaze_image, image_score, visibility_score
from .sparse import SparseTensor


def build_q_map(points, q_g, q_a, device):
    """utils.py:436-445: scalar q -> uniform map; per-point arrays -> that map.  Channels [q_g, q_a]."""
    n = points.shape[0]
    coords = torch.cat([torch.zeros((n, 1), device=device), points.to(device, dtype=torch.float32)], dim=1)
    if isinstance(q_a, (float, int, np.floating)):
        feats = torch.cat([torch.ones((n, 1), device=device) * float(q_g), torch.ones((n, 1), device=device) * float(q_a)], dim=1)
    else:
        feats = torch.cat([torch.as_tensor(q_g).reshape(n, 1), torch.as_tensor(q_a).reshape(n, 1)], dim=1).to(device, torch.float32)
    return SparseTensor(coordinates=coords, features=feats, device=device)


def compress_model_ours(experiment, model, data, q_a, q_g, device, base_path):
    """-> (source [N,6], reconstruction [N',6], bpp, t_compress, t_decompress); the bitstream goes
    through ``<base_path>/<experiment>/tmp/bitstream.bin`` like the reference's."""
    points = data["src"]["points"].to(device, dtype=torch.float)
    colors = data["src"]["colors"].to(device, dtype=torch.float)
    source = torch.cat([points, colors], dim=2)[0]
    n = source.shape[0]
    bin_dir = os.path.join(base_path, experiment, "tmp")
    os.makedirs(bin_dir, exist_ok=True)
    bin_path = os.path.join(bin_dir, "bitstream.bin")
    q_map = build_q_map(points[0], q_g, q_a, device)

    torch.cuda.synchronize()
    t0 = time.time()
    model.compress(source, q_map, path=bin_path)
    torch.cuda.synchronize()
    t_compress = time.time() - t0

    torch.cuda.synchronize()
    t0 = time.time()
    reconstruction = model.decompress(path=bin_path)
    torch.cuda.synchronize()
    t_decompress = time.time() - t0

    bpp = os.path.getsize(bin_path) * 8 / n
    return source, reconstruction, bpp, t_compress, t_decompress


def downsample_frame(data, factor, device, q_a=None, q_g=None):
    """the frame ``data`` on a grid ``factor`` times coarser (voxelize.downsample: cell indices, exact mean colours) ->
    (data', q_a', q_g'); per-point quality arrays follow their voxel's first point, scalars pass through"""
    from .voxelize import voxelize
    points = data["src"]["points"][0].to(device, dtype=torch.float)
    colors = data["src"]["colors"][0].to(device, dtype=torch.float)
    v = voxelize(points, colors, voxel_size=factor)

    def follow(q):
        if q is None or isinstance(q, (float, int, np.floating)):
            return q
        return torch.as_tensor(q).reshape(points.shape[0], 1).to(device)[v.first.long()]

    small = dict(data)
    small["src"] = dict(data["src"], points=v.coords[None, :, 1:].to(torch.float), colors=v.features[None])
    return small, follow(q_a), follow(q_g)


def evaluate_frame(experiment, model, data, q_a, q_g, device, base_path, resolution=1023, d2_radius=None, downsample=None, pcqm=False):
    """one row of the sweep table (evaluate.py:100-160): rate, times, D1 and colour PSNRs; with ``d2_radius`` (the radius of the
    normal estimation, in voxels) also ``sym_d2_psnr``, the point-to-plane figure of utils.py:263-288; with ``pcqm`` also
    ``pcqm_voxel`` and ``pcqm_f1`` .. ``pcqm_f8`` (pcqm.py: a voxel-grid stand-in for the PCQM column of evaluate.py:126, NOT
    comparable with the PCQM binary's numbers).

    ``downsample`` (a factor, e.g. 2, 4, 8: the reference's "QA" sequences, data/utils/RawLoader.py:48-57): the frame is first
    voxelised on a grid that many times coarser (downsample_frame); source and quality map are built on the down-sampled
    cloud, the metrics are taken against it, and ``resolution`` (the peak of the geometry PSNR, 2^bits - 1) is scaled to the
    coarser grid: (resolution + 1) / factor - 1.  The row gains ``downsample`` and ``n_input``, the frame's own point count."""
    n_input = None
    if downsample is not None:
        if not float(downsample) >= 1.0:
            raise ValueError(f"downsample {downsample}: a factor of at least 1")
        n_input = int(data["src"]["points"].shape[1])
        data, q_a, q_g = downsample_frame(data, downsample, device, q_a, q_g)
        resolution = max(1, int(round((resolution + 1) / float(downsample))) - 1)
    src, rec, bpp, t_c, t_d = compress_model_ours(experiment, model, data, q_a, q_g, device, base_path)
    metric = PointCloudMetric(src, rec, resolution=resolution, device=device)
    res, _ = metric.compute_pointcloud_metrics(drop_duplicates=True)
    row = {"q_g": float(np.mean(q_g)), "q_a": float(np.mean(q_a)), "bpp": bpp, "t_compress": t_c, "t_decompress": t_d,
            "n_source": int(src.shape[0]), "n_decoded": int(rec.shape[0]),
            "sym_p2p_psnr": res["sym_psnr_mse"], "sym_y_psnr": res["sym_y_psnr"], "sym_u_psnr": res["sym_u_psnr"],
            "sym_v_psnr": res["sym_v_psnr"]}
    if d2_radius is not None:
        row["sym_d2_psnr"] = metric.compute_d2(radius=d2_radius)["sym_d2_psnr"]
    if pcqm:
        row.update(_pcqm_columns(metric))
    if downsample is not None:
        row["downsample"], row["n_input"] = float(downsample), n_input
    return row


def _pcqm_columns(metric):
    """``pcqm_voxel`` and ``pcqm_f1`` .. ``pcqm_f8`` of a PointCloudMetric: the voxel-grid stand-in (pcqm.py), not PCQM's number"""
    res = metric.compute_pcqm()
    return {k: v for k, v in res.items() if k.startswith("pcqm_")}


# the qsteps evaluate_view_dependent searches for an anchor row that matches a model row's bytes: from a quarter of an 8-bit level
# up to four times the colour range, where little but the DC survives, so that a model row of very low rate still finds its match
ANCHOR_MATCH_QSTEPS = (0.25 / 255, 1024 / 255)


def _levels_bytes(stream):
    """the bytes a PCA1 stream spends on block levels: the levels payload of its PCR2 attributes, 0 for PCR1"""
    import struct
    from . import raht
    (glen,) = struct.unpack("<I", stream[8:12])
    attributes = stream[12 + glen:]
    if attributes[:4] != raht.MAGIC_REGION:
        return 0
    return int(struct.unpack("<I", attributes[25:29])[0])


def evaluate_anchor(data, qstep, device, resolution=1023, downsample=None, colorspace="yuv", pcqm=False, contexts=False, quality=None,
                    block_log2=3, span=24, scale=None, transfer="nearest"):
    """one row of the sweep table for the octree + RAHT anchor codec (anchor.py) at quantisation step ``qstep``: the keys of
    ``evaluate_frame``'s row without the quality-map pair, plus ``qstep`` and ``codec``.  ``bpp`` counts the whole PCA1 stream;
    the geometry is lossless, so ``sym_p2p_psnr`` is inf and ``n_decoded`` equals ``n_source``.  ``downsample`` and
    ``resolution`` mean what they mean in ``evaluate_frame``: the anchor's lossy-geometry rate points are coarser grids; so does
    ``pcqm``.  ``contexts``: the anchor's geometry as PCO2 (octree.py: neighbour contexts) instead of PCO1.

    ``quality`` (a per-point map as ``anchor.compress`` takes it, with ``block_log2`` and ``span``): region-wise quantisation;
    with ``downsample`` the map follows each voxel's first point.  The row gains ``levels_bytes``, what the stream spends on
    the block levels (0 without a map).

    ``scale`` (what ``rescale.as_scale`` takes; not together with ``downsample``): lossy geometry by position scaling, the PCA2
    stream (anchor.compress's ``scale`` and ``transfer``).  The decoded cloud lives on the ORIGINAL grid, so the metrics are
    ``PointCloudMetric(original, decoded, resolution)`` at the resolution given and ``bpp`` is bits per original point: the row
    stands on the axes of the model's rows.  ``n_decoded`` is the number of cells, ``sym_p2p_psnr`` is finite, and the row gains
    ``scale`` (a float), ``scale_num``, ``scale_den`` and ``transfer``."""
    from . import anchor, rescale
    if scale is not None:
        if downsample is not None:
            raise ValueError("evaluate_anchor: scale and downsample are two ways to the same end; give one")
        num, den = rescale.as_scale(scale)
        if transfer not in rescale.TRANSFERS:
            raise ValueError(f"transfer {transfer!r}: 'nearest' or 'cell'")
    n_input = None
    if downsample is not None:
        if not float(downsample) >= 1.0:
            raise ValueError(f"downsample {downsample}: a factor of at least 1")
        n_input = int(data["src"]["points"].shape[1])
        if quality is not None:
            quality = torch.as_tensor(quality).reshape(n_input, -1)[:, -1]
        data, quality, _ = downsample_frame(data, downsample, device, quality)
        resolution = max(1, int(round((resolution + 1) / float(downsample))) - 1)
    points = data["src"]["points"].to(device, dtype=torch.float)
    colors = data["src"]["colors"].to(device, dtype=torch.float)
    src = torch.cat([points, colors], dim=2)[0]

    torch.cuda.synchronize()
    t0 = time.time()
    extra = {} if scale is None else {"scale": (num, den), "transfer": transfer}
    stream = anchor.compress(src, qstep, colorspace=colorspace, contexts=contexts, quality=quality, block_log2=block_log2, span=span, **extra)
    torch.cuda.synchronize()
    t_c = time.time() - t0

    torch.cuda.synchronize()
    t0 = time.time()
    rec = anchor.decompress(stream, device)
    torch.cuda.synchronize()
    t_d = time.time() - t0

    metric = PointCloudMetric(src, rec, resolution=resolution, device=device)
    res, _ = metric.compute_pointcloud_metrics(drop_duplicates=True)
    row = {"codec": "octree+raht", "qstep": float(qstep), "bpp": len(stream) * 8 / src.shape[0], "t_compress": t_c, "t_decompress": t_d,
           "n_source": int(src.shape[0]), "n_decoded": int(rec.shape[0]), "levels_bytes": _levels_bytes(stream),
           "sym_p2p_psnr": res["sym_psnr_mse"], "sym_y_psnr": res["sym_y_psnr"], "sym_u_psnr": res["sym_u_psnr"],
           "sym_v_psnr": res["sym_v_psnr"]}
    if pcqm:
        row.update(_pcqm_columns(metric))
    if downsample is not None:
        row["downsample"], row["n_input"] = float(downsample), n_input
    if scale is not None:
        row.update(scale=num / den, scale_num=num, scale_den=den, transfer=transfer)
    return row


def _extent(points, axis):
    c = points[:, axis]
    return float(c.min()), float(c.max())


def evaluate_view_dependent(experiment, model, data, q_a, q_g, device, base_path, view="front", H=1024, W=512, gradient=None, roi=None,
                            save_images=False, details=None, facing=None, visibility=None, camera=None, anchor=None, screen=None):
    """The three rows of evaluate_view_dep.py:139-301 for one frame -> {"uniform": row, "view": row, "roi": row}, each row
    {"bpp", "q_a", "q_g", "key", "psnr", "ssim"}.

    ``facing`` (a dict) appends a fourth row "facing", judged by the same rendered view: quality by the angle between each
    point's normal and the viewing ray (q_map.facing_score; evaluate_view_dep.py:354-376).  Its keys: ``radius`` of the normal
    estimation (3), ``camera`` (a position) or ``direction`` (the view's front axis when neither is given), ``floor`` (0.0).

    ``visibility`` (a dict) appends a row "visible" after the others, judged by the same rendered view: quality by what the
    views can show (render.visibility on the source's points at H x W, each view framing the source; q_map.visibility_score).
    Its keys: ``views`` (a list of presets or (front, up) pairs; the judged view when left out), ``tolerance`` (2), ``falloff``
    (8), ``floor`` (0.0), ``point_size`` (None: each frame's scale).  ``details["visibility"]`` receives (behind, score).

    ``view``: a preset of render.VIEWS or a (front, up) pair.  ``gradient=(axis, lo, hi)``: the view-dependent map, score =
    clip((p[axis] - lo) / (hi - lo), 0, 1) with axis 0..2 over x, y, z (:209-215; lo > hi makes quality rise towards
    smaller coordinates); ``roi=(axis, plane)``: score = 1 where p[axis] >= plane, else 0 (:254-260).  Both maps scale
    (q_g, q_a) per point.  The reference keeps these numbers per sequence (:58-77); they stay with the caller.  None
    derives them from the frame: the gradient runs along the viewing axis from the farthest voxel (0) to the nearest (1),
    the region of interest is the half of the frame towards the view's right.

    All four images (the source and the three reconstructions) are rendered in the SOURCE's frame.  ``save_images`` writes
    them as PNG under ``<base_path>/<experiment>/renders_view/`` (the reference's names, :188-278).  ``details`` (a dict)
    receives ``{"source" | "uniform" | "view" | "roi" (| "facing") (| "visible"): (cloud, image)}`` for callers that want the tensors.

    ``camera`` (a render.Camera): the viewer stands at a point.  The source and every reconstruction are then rendered and
    judged by render.render_camera, and ``view``, ``H`` and ``W`` are not used (the image size is the camera's; the images are
    tagged "camera").  The default gradient runs along the camera's dominant front axis and the default region of interest
    along its dominant right axis; ``facing`` defaults its ``camera`` to the camera's position; ``visibility`` takes ``cameras``
    (a list of render.Camera; ``[camera]`` when left out) in place of ``views`` and uses render.camera_visibility, with
    ``point_size`` a voxel edge (1.0).  With ``camera=None`` nothing changes.

    ``anchor`` (a dict): a conventional baseline for every row.  After the model's rows one row ``"anchor_<key>"`` per map is
    appended (uniform, view, roi, and facing / visible when present): the source coded by the octree + RAHT anchor codec
    (anchor.py) with that row's score as its quality map (score 1 at the row's qstep, lower scores coarser; the uniform row has
    no map and is the plain PCR1 stream), rendered and judged by the same view or camera in the source's frame.  Its keys:
    ``match`` (True: every anchor row is searched, anchor.compress_to_bytes over ANCHOR_MATCH_QSTEPS, to at most the bytes of
    the model's row with the same key; False: it is coded at ``qstep``), ``qstep`` (needed without ``match``), ``block_log2``, ``span``, ``colorspace``,
    ``contexts`` (anchor.compress's).  The rows carry ``"codec": "anchor"``, the ``qstep`` used, ``reached`` (False when even
    the coarsest step of the search is above the bytes to match), ``levels_bytes``, and q_a = q_g = None.  Images are saved as
    ``anchor_<key>_<tag>.png``.  With ``anchor=None`` nothing changes.

    ``screen`` (a dict) appends a row "screen" after the others: quality by an IMAGE in the judged view — a detector's box, a
    painted mask, a gaze point — carried back to the source's points by render.sample_views (render.sample_cameras with
    ``camera``) through the judged view in the source's frame, and scored by q_map.image_score.  Its keys: exactly one of
    ``image`` (an integer [H, W] array of the judged view's size, 255 = full quality), ``box`` (r0, r1, c0, c1: q_map.box_image)
    and ``gaze`` (row, col, radius, falloff: q_map.gaze_image); ``tolerance`` (2: the pixels within two voxels of the point's
    surface; None: only the pixels that show it), ``reduce`` ("max"), ``floor`` (0.0), ``point_size`` (as ``visibility``'s).
    ``details["screen"]`` receives (total, count, peak, score), so the row's own (cloud, image) pair goes to
    ``details["screen_row"]``.  Every row, anchor rows included, then also carries ``psnr_roi``
    and ``ssim_roi``: render.view_metrics with ``mask = image > 0``, so that the uniform and plane-ROI rows can be compared with
    the screen row INSIDE the region.  With ``screen=None`` nothing changes."""
    if anchor is not None:
        unknown = set(anchor) - {"qstep", "match", "block_log2", "span", "colorspace", "contexts"}
        if unknown:
            raise ValueError("anchor: unknown keys %s" % sorted(unknown))
        if not anchor.get("match", True) and anchor.get("qstep") is None:
            raise ValueError("anchor: without match the rows need a qstep")
    if camera is not None:
        if not isinstance(camera, render.Camera):
            raise ValueError("camera is a render.Camera, got %r" % (camera,))
        right, up, front = ([float(v) for v in a] for a in (camera.right, camera.up, camera.front))
        tag = "camera"
    else:
        front, up = render._view(view)
        right, up, front = render.view_axes(front, up)
        tag = view if isinstance(view, str) else "custom"

    def dominant(axis):
        mags = [abs(a) for a in axis]
        return mags.index(max(mags))

    points = data["src"]["points"][0].to(device, dtype=torch.float)
    if gradient is None:
        axis = dominant(front)
        lo, hi = _extent(points, axis)
        gradient = (axis, lo, hi) if front[axis] > 0 else (axis, hi, lo)
    if roi is None:
        axis = dominant(right)
        lo, hi = _extent(points, axis)
        roi = (axis, (lo + hi) / 2.0)
    g_axis, g_lo, g_hi = gradient
    r_axis, r_plane = roi
    maps = {
        "uniform": None,
        "view": torch.clamp((points[:, g_axis] - float(g_lo)) / (float(g_hi) - float(g_lo)), 0, 1),
        "roi": (points[:, r_axis] >= float(r_plane)).to(torch.float),
    }
    if facing is not None:
        eye, direction = facing.get("camera"), facing.get("direction")
        if eye is None and direction is None:
            if camera is not None:
                eye = [float(v) for v in camera.position]
            else:
                direction = front
        normals, _ = estimate_normals(points, radius=facing.get("radius", 3))
        maps["facing"] = facing_score(points, normals, eye, direction, facing.get("floor", 0.0)).to(torch.float)
    if visibility is not None:
        unknown = set(visibility) - {"views" if camera is None else "cameras", "tolerance", "falloff", "floor", "point_size"}
        if unknown:
            raise ValueError("visibility: unknown keys %s" % sorted(unknown))
        if camera is None:
            behind, _ = render.visibility(points, visibility.get("views", [view]), H, W, point_size=visibility.get("point_size"), device=device)
        else:
            size = visibility.get("point_size")
            behind, _, _ = render.camera_visibility(points, visibility.get("cameras", [camera]), point_size=1.0 if size is None else size,
                                                    device=device)
        vis_score = visibility_score(behind, visibility.get("tolerance", 2), visibility.get("falloff", 8), visibility.get("floor", 0.0))
        maps["visible"] = vis_score.to(torch.float)
        if details is not None:
            details["visibility"] = (behind, vis_score)
    roi_mask = None
    if screen is not None:
        unknown = set(screen) - {"image", "box", "gaze", "tolerance", "reduce", "floor", "point_size"}
        if unknown:
            raise ValueError("screen: unknown keys %s" % sorted(unknown))
        if sum(k in screen for k in ("image", "box", "gaze")) != 1:
            raise ValueError("screen: give exactly one of image, box and gaze")
        s_h, s_w = (camera.H, camera.W) if camera is not None else (int(H), int(W))
        if "box" in screen:
            s_img = box_image(s_h, s_w, screen["box"])
        elif "gaze" in screen:
            g_row, g_col, g_radius, g_falloff = screen["gaze"]
            s_img = gaze_image(s_h, s_w, (g_row, g_col), g_radius, g_falloff)
        else:
            s_img = screen["image"]
        s_img = s_img if torch.is_tensor(s_img) else torch.as_tensor(np.asarray(s_img))
        if s_img.dim() != 2 or tuple(s_img.shape) != (s_h, s_w):
            raise ValueError("screen: the image is [H, W] of the judged view's size %d x %d, got %s" % (s_h, s_w, tuple(s_img.shape)))
        size = screen.get("point_size")
        if camera is None:
            sampled = render.sample_views(points, [view], [s_img], H, W, point_size=size, tolerance=screen.get("tolerance", 2), device=device)
        else:
            sampled = render.sample_cameras(points, [camera], [s_img], point_size=1.0 if size is None else size,
                                            tolerance=screen.get("tolerance", 2), device=device)
        screen_score = image_score(*sampled, reduce=screen.get("reduce", "max"), floor=screen.get("floor", 0.0))
        maps["screen"] = screen_score.to(torch.float)
        roi_mask = (s_img > 0).to(device)
        if details is not None:
            details["screen"] = sampled + (screen_score,)
    img_dir = os.path.join(base_path, experiment, "renders_view")
    if save_images:
        os.makedirs(img_dir, exist_ok=True)
    rows, frame, ref_img = {}, None, None

    def judge_region(row, img):
        if roi_mask is not None:
            m_roi = render.view_metrics(ref_img, img, mask=roi_mask)
            row["psnr_roi"], row["ssim_roi"] = m_roi["psnr"], m_roi["ssim"]

    for key, score in maps.items():
        qa = q_a if score is None else (float(q_a) * score).reshape(-1, 1)
        qg = q_g if score is None else (float(q_g) * score).reshape(-1, 1)
        src, rec, bpp, _, _ = compress_model_ours(experiment, model, data, qa, qg, device, base_path)
        if camera is not None:
            draw = lambda cloud: render.render_camera(cloud, camera)
        else:
            if frame is None:
                frame = render.view_frame(src, front, up, H, W)
            draw = lambda cloud: render.render_view(cloud, front, up, H, W, frame=frame)
        if ref_img is None:
            ref_img = draw(src)
            if save_images:
                write_png(os.path.join(img_dir, "ref_%s.png" % tag), ref_img)
            if details is not None:
                details["source"] = (src, ref_img)
        img = draw(rec)
        m = render.view_metrics(ref_img, img)
        rows[key] = {"bpp": bpp, "q_a": q_a, "q_g": q_g, "key": key, "psnr": m["psnr"], "ssim": m["ssim"]}
        judge_region(rows[key], img)
        if save_images:
            write_png(os.path.join(img_dir, "%s_a%s_g%s_%s.png" % (key, str(q_a), str(q_g), tag)), img)
        if details is not None:
            details["screen_row" if key == "screen" else key] = (rec, img)      # details["screen"] holds the sampled arrays
    if anchor is not None:
        from . import anchor as anchor_codec
        match, qstep = anchor.get("match", True), anchor.get("qstep")
        kw = {k: anchor[k] for k in ("block_log2", "span", "colorspace", "contexts") if k in anchor}
        n = int(src.shape[0])
        for key, score in maps.items():
            if match:
                stream, step, reached = anchor_codec.compress_to_bytes(src, int(round(rows[key]["bpp"] * n / 8)), quality=score,
                                                                       qstep_lo=ANCHOR_MATCH_QSTEPS[0], qstep_hi=ANCHOR_MATCH_QSTEPS[1], **kw)
            else:
                stream, step, reached = anchor_codec.compress(src, qstep, quality=score, **kw), float(qstep), True
            rec = anchor_codec.decompress(stream, device)
            img = draw(rec)
            m = render.view_metrics(ref_img, img)
            name = "anchor_" + key
            rows[name] = {"bpp": len(stream) * 8 / n, "q_a": None, "q_g": None, "key": name, "psnr": m["psnr"], "ssim": m["ssim"],
                          "codec": "anchor", "qstep": step, "reached": reached, "levels_bytes": _levels_bytes(stream)}
            judge_region(rows[name], img)
            if save_images:
                write_png(os.path.join(img_dir, "%s_%s.png" % (name, tag)), img)
            if details is not None:
                details[name] = (rec, img)
    return rows
