#!/usr/bin/env python3
"""RD sweep of BASELINE config 3: 4 synthetic frames with the point counts of
redandblack / loot / longdress / soldier x the 4 (q_g, q_a) pairs of plot.py:31-32, each through
file-mode compress / decompress + GPU metrics; Bjontegaard deltas between the frames' curves.
Seeded random weights in their q-RESPONSIVE variant (synthetic.FILM_GAIN_Q_RESPONSIVE: FiLM heads with gain 1.0, so the rate
follows the quality map; PCC_SWEEP_FILM_GAIN overrides): the rate axis is a real sweep, the distortion axis is that of random
weights — not codec quality.

usage: rd_sweep.py [--d2 R] [--pcqm] [--downsample F] [--anchor] [--anchor-contexts] [--anchor-scales] [--target-bpp B [B ...]] [out.json] [weights.pt]
  --d2 R: add the point-to-plane PSNR, normals over R voxels
  --pcqm: add ``pcqm_voxel`` (pcc_amd.pcqm: PCQM's structure on the voxel grid, a stand-in that is NOT comparable with the numbers
          of the PCQM binary behind the reference's ``pcqm`` column) and its pooled features to every row; with --anchor also the
          BD-rate over the quality axis 1 - pcqm_voxel against the anchor
  --downsample F: code every frame on a grid F times coarser (pcc_amd.voxelize: exact mean colours; the reference's "QA" factors
                  are 1, 2, 4, 8), metrics against the down-sampled source
  --anchor: also code every frame with the octree + RAHT anchor codec (pcc_amd.anchor) at qstep = {2, 4, 8, 16, 32, 64} / 255 and
            report the model's BD-rate and BD-PSNR (Y) against the anchor's curve of the same frame
  --anchor-contexts: --anchor with the anchor's geometry coded as PCO2 (pcc_amd.octree: neighbour contexts) instead of PCO1
  --anchor-scales: also code every frame with the anchor at the joint operating points at which the reference places G-PCC
            (pcc_amd.anchor.GPCC_POINTS: position scale 0.125 .. 0.75 with the qstep of its QP, anchor.qp_to_qstep) — lossy geometry by
            position scaling, judged against the original frame like the model's rows ("anchor_scaled_rows" of the output) — and
            report the model's BD-rate and BD-PSNR against that curve over Y-PSNR and, since both codecs now lose geometry, over D1
            (with --anchor-contexts the cells are coded as PCO2; not together with --downsample)
  --target-bpp B [B ...]: add rows coded to a target instead of a q pair (pcc_amd.rate_control.compress_to_target: the y + z payload
            in bits per input point stays at or below B); each row is the frame evaluated at the (q_g, q_a) the search chose, with
            the target, the probe count and whether it was reached ("target_rows" of the output; the q-grid rows are unchanged)"""
import json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import pcc_amd
from pcc_amd import synthetic as syn
from pcc_amd.harness import evaluate_anchor, evaluate_frame
from pcc_amd.metrics import Bjontegaard_Delta, Bjontegaard_Model

dev = "cuda:0"
d2_radius = None
if "--d2" in sys.argv:
    at = sys.argv.index("--d2")
    d2_radius = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
with_pcqm = "--pcqm" in sys.argv
if with_pcqm:
    sys.argv.remove("--pcqm")
downsample = None
if "--downsample" in sys.argv:
    at = sys.argv.index("--downsample")
    downsample = float(sys.argv[at + 1])
    del sys.argv[at:at + 2]
anchor_contexts = "--anchor-contexts" in sys.argv
if anchor_contexts:
    sys.argv.remove("--anchor-contexts")
with_scales = "--anchor-scales" in sys.argv
if with_scales:
    sys.argv.remove("--anchor-scales")
    if downsample is not None:
        sys.exit("--anchor-scales and --downsample are two ways to the same end; give one")
with_anchor = (anchor_contexts and not with_scales) or "--anchor" in sys.argv
if "--anchor" in sys.argv:
    sys.argv.remove("--anchor")
target_bpps = []
if "--target-bpp" in sys.argv:
    at = end = sys.argv.index("--target-bpp")
    while end + 1 < len(sys.argv):
        try:
            target_bpps.append(float(sys.argv[end + 1]))
        except ValueError:
            break
        end += 1
    if not target_bpps:
        sys.exit("--target-bpp needs at least one number")
    del sys.argv[at:end + 1]
ANCHOR_QSTEPS = [q / 255 for q in (2, 4, 8, 16, 32, 64)]
FRAMES = {"redandblack~": 247.0, "loot~": 255.0, "longdress~": 261.5, "soldier~": 294.5}   # shell radii -> ~0.76 / 0.81 / 0.86 / 1.09 M
QS = [(0.05, 0.1), (0.1, 0.2), (0.2, 0.4), (0.4, 0.8)]
film_gain = float(os.environ.get("PCC_SWEEP_FILM_GAIN", syn.FILM_GAIN_Q_RESPONSIVE))
model = syn.make_model(seed=0, device=dev, film_gain=film_gain)
if len(sys.argv) > 2:
    model.load_state_dict(torch.load(sys.argv[2], map_location=dev))
model.update()
rows, anchor_rows, target_rows, scaled_rows = [], [], [], []
with tempfile.TemporaryDirectory() as td:
    for name, radius in FRAMES.items():
        pts = syn.sphere_shell(grid=1024, radius=radius, half_width=0.5, noise=0.02)
        data = {"src": {"points": torch.from_numpy(pts[None, :, :3]), "colors": torch.from_numpy(pts[None, :, 3:])}}
        for q_g, q_a in QS:
            t0 = time.time()
            row = evaluate_frame("sweep", model, data, q_a, q_g, dev, td, d2_radius=d2_radius, downsample=downsample, pcqm=with_pcqm)
            row["frame"] = name
            rows.append(row)
            print(f"{name:13s} N={row['n_source']:8d} q=({q_g},{q_a}) bpp {row['bpp']:.3f} D1 {row['sym_p2p_psnr']:.2f} Y {row['sym_y_psnr']:.2f} "
                  + (f"D2 {row['sym_d2_psnr']:.2f} " if d2_radius is not None else "") + (f"pcqm_voxel {row['pcqm_voxel']:.5f} " if with_pcqm else "") +
                  f"t_enc {row['t_compress']*1e3:.0f} ms t_dec {row['t_decompress']*1e3:.0f} ms (row {time.time()-t0:.1f} s)", flush=True)
        for bpp in target_bpps:
            from pcc_amd.harness import downsample_frame
            from pcc_amd.rate_control import compress_to_target
            t0 = time.time()
            coded = data if downsample is None else downsample_frame(data, downsample, dev)[0]
            src = torch.cat([coded["src"]["points"], coded["src"]["colors"]], dim=2)[0].to(dev, dtype=torch.float)
            found = compress_to_target(model, src, target_bpp=bpp)
            q_g, q_a = found["q"]
            row = evaluate_frame("sweep", model, data, q_a, q_g, dev, td, d2_radius=d2_radius, downsample=downsample, pcqm=with_pcqm)
            row.update(frame=name, target_bpp=bpp, target_reached=found["reached"], t=found["t"], probes=len(found["log"]),
                       payload_bpp=found["bytes"] * 8 / src.shape[0], estimate_bpp=found["estimate"] * 8 / src.shape[0])
            target_rows.append(row)
            print(f"{name:13s} N={row['n_source']:8d} target {bpp} bpp -> q=({q_g:.4f},{q_a:.4f}) payload {row['payload_bpp']:.3f} bpp "
                  f"({'reached' if found['reached'] else 'NOT reached'}, {row['probes']} probes) file {row['bpp']:.3f} bpp Y {row['sym_y_psnr']:.2f} "
                  f"(row {time.time()-t0:.1f} s)", flush=True)
        for qstep in (ANCHOR_QSTEPS if with_anchor else ()):
            t0 = time.time()
            row = evaluate_anchor(data, qstep, dev, downsample=downsample, pcqm=with_pcqm, contexts=anchor_contexts)
            row["frame"] = name
            anchor_rows.append(row)
            print(f"{name:13s} N={row['n_source']:8d} anchor qstep {qstep * 255:.0f}/255 bpp {row['bpp']:.3f} Y {row['sym_y_psnr']:.2f} "
                  f"t_enc {row['t_compress']*1e3:.0f} ms t_dec {row['t_decompress']*1e3:.0f} ms (row {time.time()-t0:.1f} s)", flush=True)
        for scale, qp in (pcc_amd.anchor.GPCC_POINTS if with_scales else ()):
            t0 = time.time()
            row = evaluate_anchor(data, pcc_amd.anchor.qp_to_qstep(qp), dev, pcqm=with_pcqm, contexts=anchor_contexts, scale=scale)
            row.update(frame=name, qp=qp)
            scaled_rows.append(row)
            print(f"{name:13s} N={row['n_source']:8d} anchor scale {scale} QP {qp} M={row['n_decoded']} bpp {row['bpp']:.3f} "
                  f"D1 {row['sym_p2p_psnr']:.2f} Y {row['sym_y_psnr']:.2f} t_enc {row['t_compress']*1e3:.0f} ms "
                  f"t_dec {row['t_decompress']*1e3:.0f} ms (row {time.time()-t0:.1f} s)", flush=True)
bd = {}
names = list(FRAMES)
ref = [r for r in rows if r["frame"] == names[0]]
for nm in names[1:]:
    cur = [r for r in rows if r["frame"] == nm]
    try:
        m1 = Bjontegaard_Model([r["bpp"] for r in ref], [r["sym_y_psnr"] for r in ref])
        m2 = Bjontegaard_Model([r["bpp"] for r in cur], [r["sym_y_psnr"] for r in cur])
        bd[nm] = {"bd_psnr_y_vs_" + names[0]: float(Bjontegaard_Delta().compute_BD_PSNR(m1, m2))}
    except Exception as e:      # degenerate curves (seeded weights) must not lose the table
        bd[nm] = {"error": repr(e)}
for nm in (names if with_anchor else ()):
    cur, anc = [r for r in rows if r["frame"] == nm], [r for r in anchor_rows if r["frame"] == nm]
    entry = bd.setdefault(nm, {})
    try:                        # model1 = the anchor: the deltas are the model's against it (negative BD-rate = the model needs fewer bits)
        m1 = Bjontegaard_Model([r["bpp"] for r in anc], [r["sym_y_psnr"] for r in anc])
        m2 = Bjontegaard_Model([r["bpp"] for r in cur], [r["sym_y_psnr"] for r in cur])
        # (a delta is a mean over the interval both curves cover; without one there is nothing to average)
        if max(m1.psnr_values.min(), m2.psnr_values.min()) < min(m1.psnr_values.max(), m2.psnr_values.max()):
            entry["bd_rate_y_vs_anchor"] = float(Bjontegaard_Delta().compute_BD_Rate(m1, m2))
        else:
            entry["bd_rate_y_vs_anchor"] = None
            entry["error_vs_anchor"] = "the Y-PSNR ranges of the model's and the anchor's curve do not overlap: no BD-rate"
        if max(m1.bitrates.min(), m2.bitrates.min()) < min(m1.bitrates.max(), m2.bitrates.max()):
            entry["bd_psnr_y_vs_anchor"] = float(Bjontegaard_Delta().compute_BD_PSNR(m1, m2))
        else:
            entry["bd_psnr_y_vs_anchor"] = None
            entry["error_vs_anchor"] = entry.get("error_vs_anchor", "") + " the rate ranges do not overlap: no BD-PSNR"
    except Exception as e:      # curves that do not overlap, or degenerate fits
        entry["error_vs_anchor"] = repr(e)
    if with_pcqm:               # the same delta over the quality axis 1 - pcqm_voxel (higher = better, like a PSNR)
        try:
            m1 = Bjontegaard_Model([r["bpp"] for r in anc], [1.0 - r["pcqm_voxel"] for r in anc])
            m2 = Bjontegaard_Model([r["bpp"] for r in cur], [1.0 - r["pcqm_voxel"] for r in cur])
            if max(m1.psnr_values.min(), m2.psnr_values.min()) < min(m1.psnr_values.max(), m2.psnr_values.max()):
                entry["bd_rate_pcqm_voxel_vs_anchor"] = float(Bjontegaard_Delta().compute_BD_Rate(m1, m2))
            else:
                entry["bd_rate_pcqm_voxel_vs_anchor"] = None
                entry["error_pcqm_voxel_vs_anchor"] = "the 1 - pcqm_voxel ranges of the model's and the anchor's curve do not overlap: no BD-rate"
        except Exception as e:
            entry["error_pcqm_voxel_vs_anchor"] = repr(e)

def deltas_vs_scaled(entry, anc, cur, key, tag):
    """the model's BD-rate and BD-PSNR over ``key`` against the scaled anchor's curve, with the overlap guards of the entries above"""
    try:
        m1 = Bjontegaard_Model([r["bpp"] for r in anc], [r[key] for r in anc])
        m2 = Bjontegaard_Model([r["bpp"] for r in cur], [r[key] for r in cur])
        if max(m1.psnr_values.min(), m2.psnr_values.min()) < min(m1.psnr_values.max(), m2.psnr_values.max()):
            entry[f"bd_rate_{tag}_vs_anchor_scaled"] = float(Bjontegaard_Delta().compute_BD_Rate(m1, m2))
        else:
            entry[f"bd_rate_{tag}_vs_anchor_scaled"] = None
            entry[f"error_{tag}_vs_anchor_scaled"] = f"the {key} ranges of the model's and the scaled anchor's curve do not overlap: no BD-rate"
        if max(m1.bitrates.min(), m2.bitrates.min()) < min(m1.bitrates.max(), m2.bitrates.max()):
            entry[f"bd_psnr_{tag}_vs_anchor_scaled"] = float(Bjontegaard_Delta().compute_BD_PSNR(m1, m2))
        else:
            entry[f"bd_psnr_{tag}_vs_anchor_scaled"] = None
            entry[f"error_{tag}_vs_anchor_scaled"] = entry.get(f"error_{tag}_vs_anchor_scaled", "") + " the rate ranges do not overlap: no BD-PSNR"
    except Exception as e:      # degenerate fits
        entry[f"error_{tag}_vs_anchor_scaled"] = repr(e)


for nm in (names if with_scales else ()):
    cur, anc = [r for r in rows if r["frame"] == nm], [r for r in scaled_rows if r["frame"] == nm]
    deltas_vs_scaled(bd.setdefault(nm, {}), anc, cur, "sym_y_psnr", "y")
    deltas_vs_scaled(bd.setdefault(nm, {}), anc, cur, "sym_p2p_psnr", "d1")
out = {"rows": rows, "bjontegaard": bd,
       "note": ("weights from " + os.path.basename(sys.argv[2]) if len(sys.argv) > 2 else "seeded random weights") +
               f" (FiLM-head gain {film_gain}); synthetic shells sized like the 8iVFB frames",
       **({"anchor_rows": anchor_rows, "anchor": "octree + RAHT (pcc_amd.anchor): lossless " + ("PCO2" if anchor_contexts else "PCO1") + " geometry, BT.709 YUV attributes, "
                                                  "qstep = {2, 4, 8, 16, 32, 64} / 255"} if with_anchor else {}),
       **({"anchor_scaled_rows": scaled_rows,
           "anchor_scaled": "octree + RAHT with position scaling (pcc_amd.anchor, PCA2): the cells coded as " + ("PCO2" if anchor_contexts else "PCO1") +
                            ", colours transferred to the nearest reconstructed position, (scale, QP) = anchor.GPCC_POINTS with "
                            "qstep = anchor.qp_to_qstep(QP); metrics against the original frame, bpp per original point"} if with_scales else {}),
       **({"target_rows": target_rows} if target_bpps else {}),
       **({"pcqm_voxel": "PCQM's structure on the voxel grid (pcc_amd.pcqm); a stand-in, not comparable with the PCQM binary's numbers"}
          if with_pcqm else {}),
       "rate_axis_monotone_in_q": {nm: [r["bpp"] for r in rows if r["frame"] == nm] == sorted(r["bpp"] for r in rows if r["frame"] == nm)
                                   for nm in names}}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gpurun_out", "rd_sweep.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
json.dump(out, open(path, "w"), indent=1)
print("wrote", path)
