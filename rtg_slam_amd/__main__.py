"""Command-line entry points, the reference's two scripts on recorded datasets:

    python -m rtg_slam_amd slam   --config configs/replica/office0.yaml     (slam.py)
    python -m rtg_slam_amd metric --config configs/replica/office0.yaml     (metric.py)
    python -m rtg_slam_amd mesh   --config configs/replica/office0.yaml     (no counterpart: a triangle mesh of the map)

`slam` writes, under the config's save_path: config.yaml (the merged config), save_model/frame_XXXX/iter_XXXX*.ply (at frame 0,
every save_step frames and after the final global optimisation), save_traj/pose_es.npy, pose_gt.npy and ate.txt (the ATE in
cm of every prefix of the trajectory), performance.json, eval_metric/slam_eval.csv (the in-loop evaluation rows) and
run_report.json (run_sequence's report plus the I/O statistics of the frame source and the frame size).  With
`resolution_scales: [S]` in the config, or --resolution-scale S (which overrides it and is written into config.yaml), both
commands run on frames resized to 1/S of the decoded size as the reference's loadCam resizes them, on the device.  With --pcd-densify and a config that
sets pcd_densify, it then writes save_model/pcd_densify.ply: 150 points on concentric ellipses around every stable Gaussian
(Mapping.save_densified, slam.py:146-150), theta drawn from a generator seeded with the config's seed.  `metric` evaluates a
saved model over the same frames and writes statis_frame_F_iter_I.csv; when the config sets pcd_densify and
save_model/pcd_densify.ply exists, the reconstruction metrics are computed on that file's points (metric.py:156-163).
`mesh` selects the model file as `metric` does, fuses the map's rendered depth and colour (or, with --depth-source sensor, the
dataset's own) over the trajectory into a TSDF volume and writes save_model/mesh_tsdf.ply and save_model/mesh_report.json
(rtg_slam_amd.meshing); --volume sparse keeps planes only for the 8x8x8 bricks near the surface, for boxes whose dense planes
would be refused; --texture also bakes a texture atlas for the final mesh from the map rendered at the fused poses
(meshing.texture_mesh) and writes save_model/mesh_textured.obj, mesh_textured.mtl and mesh_texture.png.
`metric --mesh` computes the reconstruction metrics on 1 M points sampled from that mesh instead.
`metric --cull-gt` scores them against the part of the GT mesh the evaluated frames saw (evaluation.VisibilityCull) and writes
eval_metric/gt_mesh_culled.ply and eval_metric/gt_cull_report.json; --cull-depth mesh decides that against the GT mesh's own
rendered depth, not the sensor's.  `metric --mesh-depth` renders save_model/mesh_tsdf.ply at every evaluated pose
(evaluation.MeshRenderer) and writes its depth L1 to eval_metric/mesh_depth_frame_F_iter_I.csv and mesh_depth_report.json.
`metric --mesh-color {vertex,texture,both}` renders save_model/mesh_tsdf.ply in its vertex colours and / or
save_model/mesh_textured.obj with its atlas at every evaluated pose (evaluation.MeshRenderer.render_color), scores the pictures
against the frames' colour (PSNR, MS-SSIM, colour L1 over the whole picture, a hole counting as black; the hit ratio and the colour
L1 over the hit pixels) and writes eval_metric/mesh_color_frame_F_iter_I.csv and mesh_color_report.json; --mesh-color-save-every K
also writes every K-th render as eval_metric/mesh_color/frame_XXXX_vertex.png / frame_XXXX_texture.png.
`mesh --cull-unseen` removes the surface no fused view could see before the mesh is written.
`metric --mesh --surface-distance` scores save_model/mesh_tsdf.ply against the GT mesh's SURFACE by exact point-to-triangle
distances (evaluation.eval_mesh_surface), with the normal consistency, and writes eval_metric/surface_distance_frame_F_iter_I.json.
`--surface-max-distance D` truncates it: only the nearest face within D metres is asked for, a distance beyond D counts as D.
`metric --align [--align-max-distance 0.10] [--align-iterations 30]` registers the scored geometry rigidly to the full GT surface
(evaluation.align_to_gt: point-to-plane ICP on exact nearest faces), scores it again under that transform and writes the transform,
the registration report and the unaligned and aligned figures to eval_metric/aligned_frame_F_iter_I.json: the transform measures
the tracker's drift, the aligned figures the shape.
`slam --rgbd-refine [--rgbd-refine-photo-weight L] [--rgbd-refine-huber D]` refines every ICP pose with the joint photometric and
geometric RGB-D alignment (rtg_slam_amd.rgbd_align) against the previous frame's colour; the keys go into config.yaml only when
given and run_report.json gains `rgbd_refine` (mean iterations, photometric inliers and ms per frame).
`--rgbd-refine-target model` takes the map's rendered colour as that target instead, and `--rgbd-refine-exposure` adds a gain
and an offset between the frame and its target to the unknowns; both need --rgbd-refine, and the report gains `target`,
`exposure` and the gain / offset statistics only when they are given.
`slam --map-exposure` brings every frame's colour into the map's exposure before the mapper sees it (rtg_slam_amd.map_exposure: a
gain and an offset per frame, fitted on the device against the map rendered at the frame's pose; frame 0 defines the map's
exposure); the key goes into config.yaml only when given and run_report.json gains `map_exposure` (the gains and offsets, the
frames fitted, those that fell back and why, the settings in force).  `--map-exposure-channels rgb` fits a gain and an offset per
colour channel (white balance) instead of one on the grey values; it needs map_exposure to be on and is written only when given.
`slam --loop-closure [--loop-closure-min-gap N ...]` closes loops once, after the last frame and before the final global
optimisation (rtg_slam_amd.loop_closure): keyframe pairs whose estimated poses lie close are registered with the RGB-D alignment,
the accepted ones join a keyframe pose graph, and the trajectory, the keyframes and the map's Gaussians move with the optimum.
save_traj/pose_es.npy is then the corrected trajectory, save_traj/pose_es_before_loop_closure.npy the tracked one, and
run_report.json gains `loop_closure`; the keys go into config.yaml only when given.  Not with use_gt_pose.
The Gaussians' centres and rotations move; their higher SH bands keep pointing where they did unless `--loop-closure-rotate-sh`
(config key loop_closure_rotate_sh; needs --loop-closure, written only when given) turns them with each frame's correction as
well (rtg_slam_amd.sh_rotation, rtgs_map_deform_sh); the report then gains `sh_rotated` and its `seconds` the stage `sh_table`.
`--loop-closure-candidates appearance` (or `both`) finds the pairs by what the keyframes look like instead of (or besides) where
the trajectory puts them (rtg_slam_amd.place_recognition: thumbnails compared by ZNCC over a horizontal shift, depth thumbnails
as a second witness), so that a loop whose drift exceeds --loop-closure-max-trans is still found; --loop-closure-thumb-width,
--loop-closure-max-shift, --loop-closure-min-score and --loop-closure-max-depth-rel set it up.  All five need --loop-closure,
are written only when given, and the report's candidates gain `source` (and `score`, `shift`, `depth_rel`) and the report
`appearance` only then.
`--relocalise` (off by default; rtg_slam_amd.relocalisation) gives the loop a lost state: a frame the ICP tracker cannot hold is
not mapped, and it and the frames after it are searched for among the keyframes until one is recovered; run_report.json gains
`relocalisation` and `ate_rmse_tracked_m`.  `--loop-closure-keypoint-ransac device` runs the keypoint pose's RANSAC in one launch.
`--loop-closure-appearance-init keypoints` (with candidates appearance or both) starts each appearance candidate's registration
from a relative pose computed from the two keyframes alone (rtg_slam_amd.keypoints: FAST-9 corners, 256-bit descriptors, a
brute-force Hamming match on the device, a 3-D - 3-D RANSAC over the matches' depth on the host) wherever that pose has
--loop-closure-keypoint-min-inliers inliers, and from the thumbnail shift's yaw otherwise, so that a revisit from 0.5 m and 12
degrees away registers; `keypoints_strict` refuses the candidate instead of falling back.  The --loop-closure-keypoint-* values
set it up; the candidates then gain `init_source`, `init` and `keypoints`, the report's `seconds` the three keypoints_* stages.
Pixel-centre corners, thresholds chosen on a synthetic room; single scale unless `--loop-closure-keypoint-levels N` (2 .. 5)
takes the keypoints from an image pyramid (scales 1, 3/2, 2, 3, 4), so that a revisit from another distance matches.
`--loop-closure-candidates keypoints` finds the revisits by those keypoints alone - every keyframe pair is matched and its
filtered matches counted on the device, the --loop-closure-keypoint-shortlist best per keyframe go through the device RANSAC and
start from its pose - where the thumbnails refuse a view from further away; the report gains `keypoint_search`.
`--relocalise-search keypoints` shortlists a lost frame's keyframes the same way, `--relocalise-keypoint-levels` sets its pyramid.
`metric --exposure-aware` also scores every render in the frame's own exposure and white balance (an affine correction per
channel, fitted on the device): eval_metric/exposure_frame_F_iter_I.csv and exposure_report.json, nothing else changes.

What the reference's configs ask for and this package does not do: device_list (the device is --device), the ORB-SLAM2 back
end (use_orb_backend: the trajectory is tracked with ICP only; --loop-closure stands in for its loop closing) and rendered
pictures."""
from __future__ import annotations

import argparse
import json
import math
import os
import shutil
import sys
import time

import numpy as np


def log(msg: str) -> None:
    print(f"[rtg_slam_amd] {msg}", flush=True)


def horn_ate_cm(pose_estimate, pose_gt) -> float:
    """SLAM/utils.py:455-503 eval_ate: align `pose_estimate`'s positions (model) onto `pose_gt`'s (data) with Horn's
    closed form, then the RMSE of the residuals, in cm.  Inputs [n,3] positions."""
    model = np.asarray(pose_estimate, dtype=np.float64).T
    data = np.asarray(pose_gt, dtype=np.float64).T
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    Wm = mz @ dz.T
    U, _, Vh = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    trans = data.mean(1, keepdims=True) - rot @ model.mean(1, keepdims=True)
    err = rot @ model + trans - data
    e = np.sqrt((err * err).sum(0))
    return float(np.sqrt(np.dot(e, e) / len(e)) * 100)


def prefix_ates(pose_es, pose_gt):
    """tracker.py:297-302, 374-380: the ATE of every prefix 1..n.  The reference passes the GT trajectory as the estimate
    (eval_ate(pose_gt, pose_es)), i.e. the GT positions are aligned onto the estimated ones; kept."""
    es = np.stack([np.asarray(p)[:3, 3] for p in pose_es])
    gt = np.stack([np.asarray(p)[:3, 3] for p in pose_gt])
    return [horn_ate_cm(gt[:i], es[:i]) for i in range(1, len(gt) + 1)]


def _save_model(mapper, save_path: str, frame: int) -> str:
    d = os.path.join(save_path, "save_model", f"frame_{frame:04d}")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"iter_{int(mapper.iter):04d}")
    mapper.save_model(path)
    return path


def _dump_config(args, path: str) -> None:
    import yaml
    d = {}
    for k, v in vars(args).items():
        d[k] = list(v) if isinstance(v, tuple) else v
    with open(path, "w") as f:
        yaml.safe_dump(d, f, sort_keys=False)


def _apply_resolution_scale(args, opts) -> None:
    """--resolution-scale S overrides the config's resolution_scales[0] (loadCam's resolution_scale)."""
    if opts.resolution_scale is not None:
        scales = list(getattr(args, "resolution_scales", None) or [1.0])
        scales[0] = float(opts.resolution_scale)
        args.resolution_scales = scales


def _apply_map_exposure(args, opts) -> None:
    """--map-exposure turns the mapper's exposure stage on (the config's `map_exposure`, absent from every preset)."""
    if getattr(opts, "map_exposure", False):
        args.map_exposure = True


def _apply_map_exposure_channels(args, opts) -> str | None:
    """--map-exposure-channels sets the config's `map_exposure_channels` (absent from every preset), only when given; -> what is
    wrong with it, or None.  Call it after _apply_map_exposure."""
    ch = getattr(opts, "map_exposure_channels", None)
    if ch is None:
        return None
    if not getattr(args, "map_exposure", False):
        return "--map-exposure-channels needs --map-exposure (or map_exposure: true in the config)"
    args.map_exposure_channels = ch
    return None


LOOP_CLOSURE_FLAGS = (("min_gap", int, "N", "keyframes between the two ends of a loop edge (default 10)"),
                      ("max_trans", float, "M", "metres between the estimated poses of a candidate pair (default 0.5)"),
                      ("max_rot_deg", float, "DEG", "degrees between them (default 30)"),
                      ("max_per_keyframe", int, "N", "candidates registered per keyframe, nearest first (default 2)"),
                      ("min_inlier_ratio", float, "R", "geometric inliers / valid source pixels an edge needs (default 0.3)"),
                      ("max_rms", float, "M", "point-to-plane rms an edge may have, metres (default 0.02)"),
                      ("max_correction_trans", float, "M", "metres a registration may move the estimate (default 0.2)"),
                      ("max_correction_rot_deg", float, "DEG", "degrees a registration may turn it (default 5)"),
                      ("odometry_weights", (float, float), ("W_ROT", "W_TRANS"), "weights of the odometry edges (default 1 1)"),
                      ("loop_weights", (float, float), ("W_ROT", "W_TRANS"), "weights of the loop edges (default 1 1)"),
                      ("candidates", str, None, "where the candidate pairs come from: the estimated poses (default), the "
                                                "keyframes' thumbnails (rtg_slam_amd.place_recognition), both, or the keyframes' "
                                                "matched keypoints alone (every pair voted on, the best few through the RANSAC)"),
                      ("thumb_width", int, "N", "columns of a keyframe's thumbnail (default 40)"),
                      ("max_shift", int, "N", "thumbnail columns searched to either side, the yaw of the first guess (default 4)"),
                      ("min_score", float, "R", "ZNCC two thumbnails need at their best shift (default 0.9)"),
                      ("max_depth_rel", float, "R", "relative difference their depth thumbnails may have (default 0.1)"),
                      ("appearance_init", str, None, "first guess of an appearance candidate: the thumbnail shift's yaw (default), "
                                                     "the pose from matched keypoints where it has its inliers "
                                                     "(rtg_slam_amd.keypoints), or that pose or no registration at all"),
                      ("keypoint_threshold", int, "N", "FAST-9 score a corner must exceed, of 255 grey levels (default 20)"),
                      ("keypoint_cell", int, "N", "pixels: one keypoint per N x N cell, 8 .. 32 (default 16)"),
                      ("keypoint_oriented", str, None, "turn the descriptor with the patch's intensity centroid (default true)"),
                      ("keypoint_max_hamming", int, "N", "bits of 256 two matched descriptors may differ in (default 64)"),
                      ("keypoint_ratio", float, "R", "best distance <= R x second best (default 0.8)"),
                      ("keypoint_ransac_iters", int, "N", "triplets drawn (default 512)"),
                      ("keypoint_inlier_dist", float, "M", "metres a match may miss the hypothesis by (default 0.05)"),
                      ("keypoint_min_inliers", int, "N", "inliers the keypoint pose needs to be used (default 8)"),
                      ("keypoint_levels", int, "N", "levels of the image pyramid the keypoints are taken from, 1 .. 5: scales 1, 3/2, "
                                                    "2, 3, 4 (default 1, single scale)"),
                      ("keypoint_shortlist", int, "N", "with candidates keypoints: older keyframes per keyframe, most votes first, "
                                                       "that go through the RANSAC (default 3)"))
LOOP_CLOSURE_CHOICES = {"candidates": ("pose", "appearance", "both", "keypoints"), "appearance_init": ("yaw", "keypoints", "keypoints_strict"),
                        "keypoint_oriented": ("true", "false")}


def _apply_loop_closure(args, opts) -> str | None:
    """--loop-closure and its --loop-closure-* values set the config's `loop_closure*` keys (absent from every preset), only when
    given; -> what is wrong with them, or None."""
    given = [(name, getattr(opts, "loop_closure_" + name, None)) for name, *_ in LOOP_CLOSURE_FLAGS]
    if getattr(opts, "loop_closure", False):
        args.loop_closure = True
    for name, value in given:
        if value is None:
            continue
        if not getattr(args, "loop_closure", False):
            return f"--loop-closure-{name.replace('_', '-')} needs --loop-closure (or loop_closure: true in the config)"
        if name == "keypoint_oriented":
            value = value == "true"
        setattr(args, "loop_closure_" + name, list(value) if isinstance(value, (list, tuple)) else value)
    if getattr(opts, "loop_closure_keypoint_ransac", None) is not None:      # not one of LOOP_CLOSURE_FLAGS: no key of DEFAULTS
        if not getattr(args, "loop_closure", False):
            return "--loop-closure-keypoint-ransac needs --loop-closure (or loop_closure: true in the config)"
        args.loop_closure_keypoint_ransac = opts.loop_closure_keypoint_ransac
    if getattr(opts, "loop_closure_rotate_sh", False):                       # a store_true flag, no key of DEFAULTS either
        if not getattr(args, "loop_closure", False):
            return "--loop-closure-rotate-sh needs --loop-closure (or loop_closure: true in the config)"
        args.loop_closure_rotate_sh = True
    if not getattr(args, "loop_closure", False):
        return None
    if getattr(args, "use_gt_pose", False):
        return "loop_closure with use_gt_pose: there is no estimated trajectory to correct"
    try:
        from .loop_closure import LoopCloser
        LoopCloser(args)
    except ValueError as e:
        return str(e)
    return None


RELOCALISE_FLAGS = (("candidates", int, "N", "keyframes a lost frame is matched against, best thumbnail score first (default 3)"),
                    ("min_score", float, "R", "ZNCC a keyframe's thumbnail needs against the lost frame's (default: loop closure's, 0.9)"),
                    ("max_depth_rel", float, "R", "relative difference their depth thumbnails may have (default: loop closure's, 0.1)"),
                    ("thumb_width", int, "N", "columns of a thumbnail (default: loop closure's, 40)"),
                    ("max_shift", int, "N", "thumbnail columns searched to either side (default: loop closure's, 4)"),
                    ("min_inliers", int, "N", "RANSAC inliers the keypoint pose needs (default: loop closure's, 8)"),
                    ("min_inlier_ratio", float, "R", "registration gate (default: loop closure's, 0.3)"),
                    ("max_rms", float, "M", "registration gate, metres (default: loop closure's, 0.02)"),
                    ("max_correction_trans", float, "M", "registration gate, metres (default: loop closure's, 0.2)"),
                    ("max_correction_rot_deg", float, "DEG", "registration gate, degrees (default: loop closure's, 5)"),
                    ("keypoint_levels", int, "N", "levels of the keypoints' image pyramid, 1 .. 5 (default: loop closure's, 1)"))


def _apply_relocalise(args, opts) -> str | None:
    """--relocalise and its --relocalise-* values set the config's `relocalise*` keys (absent from every preset), only when given;
    -> what is wrong with them, or None."""
    if getattr(opts, "relocalise", False):
        args.relocalise = True
    for name, *_ in RELOCALISE_FLAGS:
        value = getattr(opts, "relocalise_" + name, None)
        if value is None:
            continue
        if not getattr(args, "relocalise", False):
            return f"--relocalise-{name.replace('_', '-')} needs --relocalise (or relocalise: true in the config)"
        setattr(args, "relocalise_" + name, value)
    if getattr(opts, "relocalise_search", None) is not None:           # not one of RELOCALISE_FLAGS: no loop closure key behind it
        if not getattr(args, "relocalise", False):
            return "--relocalise-search needs --relocalise (or relocalise: true in the config)"
        args.relocalise_search = opts.relocalise_search
    if not getattr(args, "relocalise", False):
        return None
    try:
        from .relocalisation import Relocaliser
        Relocaliser(args)
    except ValueError as e:
        return str(e)
    return None


def cmd_slam(opts) -> int:
    import torch
    from . import config, datasets, io_formats as iof
    from .mapping import Mapping
    from .slam import run_sequence
    args = config.load_config(opts.config)
    _apply_resolution_scale(args, opts)
    if opts.frames is not None:
        args.frame_num = int(opts.frames)
    for flag, value in (("--rgbd-refine-photo-weight", opts.rgbd_refine_photo_weight), ("--rgbd-refine-huber", opts.rgbd_refine_huber)):
        if value is not None and not value > 0:
            log(f"{flag} must be positive, not {value}")
            return 2
        if value is not None and not opts.rgbd_refine:
            log(f"{flag} needs --rgbd-refine")
            return 2
    for flag, given in (("--rgbd-refine-target", opts.rgbd_refine_target is not None), ("--rgbd-refine-exposure", opts.rgbd_refine_exposure)):
        if given and not opts.rgbd_refine:
            log(f"{flag} needs --rgbd-refine")
            return 2
    if opts.rgbd_refine:
        if opts.rgbd_refine_target is not None:
            args.rgbd_refine_target = opts.rgbd_refine_target
        if opts.rgbd_refine_exposure:
            args.rgbd_refine_exposure = True
        args.rgbd_refine = True
        if opts.rgbd_refine_photo_weight is not None:
            args.rgbd_refine_photo_weight = float(opts.rgbd_refine_photo_weight)
        if opts.rgbd_refine_huber is not None:
            args.rgbd_refine_huber = float(opts.rgbd_refine_huber)
    _apply_map_exposure(args, opts)
    wrong = _apply_map_exposure_channels(args, opts)
    if wrong is not None:
        log(wrong)
        return 2
    wrong = _apply_loop_closure(args, opts)
    if wrong is not None:
        log(wrong)
        return 2
    wrong = _apply_relocalise(args, opts)
    if wrong is not None:
        log(wrong)
        return 2
    save_path = args.save_path
    if os.path.isdir(save_path) and os.listdir(save_path):
        if not opts.overwrite:
            log(f"save_path {save_path} is not empty; pass --overwrite to replace it")
            return 2
        shutil.rmtree(save_path)
    for sub in ("save_model", "save_traj", "eval_metric"):
        os.makedirs(os.path.join(save_path, sub), exist_ok=True)
    if getattr(args, "use_orb_backend", False):
        log("use_orb_backend: the ORB-SLAM2 back end is not available; tracking with ICP only")
    if getattr(args, "rgbd_refine", False):
        from . import rgbd_align
        log(f"rgbd refine: on (photo weight {getattr(args, 'rgbd_refine_photo_weight', rgbd_align.DEFAULT_PHOTO_WEIGHT):g}, "
            f"huber {getattr(args, 'rgbd_refine_huber', rgbd_align.DEFAULT_HUBER):g})")
        if hasattr(args, "rgbd_refine_target") or getattr(args, "rgbd_refine_exposure", False):
            log(f"rgbd refine: target {getattr(args, 'rgbd_refine_target', 'frame')}, "
                f"exposure {'on' if getattr(args, 'rgbd_refine_exposure', False) else 'off'}")
    if getattr(args, "map_exposure", False):
        log("map exposure: on (every frame's colour is fitted to the map's exposure)")
        if hasattr(args, "map_exposure_channels"):
            log(f"map exposure: channels {args.map_exposure_channels}")
    if getattr(args, "loop_closure", False):
        log("loop closure: on (once, after the last frame: keyframe pose graph, corrected trajectory, deformed map"
            + (", higher SH bands turned with it)" if getattr(args, "loop_closure_rotate_sh", False) else ")"))
    if getattr(args, "relocalise", False):
        log("relocalise: on (a frame ICP cannot hold is not mapped; lost frames are searched for among the keyframes)")
    if "device_list" in vars(args):
        log(f"device_list {args.device_list} ignored; running on {opts.device}")
    device = torch.device(opts.device)
    torch.cuda.set_device(device)
    _dump_config(args, os.path.join(save_path, "config.yaml"))
    info = datasets.load_dataset(args)
    source = datasets.FrameSource(info, device, io_workers=opts.io_workers)
    cam = info.camera()
    size = f"{info.width}x{info.height}"
    if info.resized:
        size += f" (resized on the device from {info.crop_width}x{info.crop_height}, resolution scale {info.resolution_scale:g})"
    log(f"{info.type} {info.source_path}: {len(info)} frames {size}, {source.io_workers} io workers")
    mapper = Mapping(args, device)
    save_step = int(getattr(args, "save_step", 2000))
    loop = {"t0": None, "t_last": None}

    def on_frame(frame_id, frame, frame_map, mapper_, tracker):
        t = mapper_.time
        if t == 0 or (t + 1) % save_step == 0:
            _save_model(mapper_, save_path, t)
        loop["t_last"] = time.perf_counter()

    torch.cuda.synchronize(device)
    loop["t0"] = time.perf_counter()
    mapper, tracker, report = run_sequence(cam, source, args, device, mapper=mapper, on_frame=on_frame, final_global=True,
                                           eval_every=save_step)
    n = report["frames"]
    if n == 0:
        log("no frames")
        return 1
    _save_model(mapper, save_path, mapper.time)
    iof.save_trajectories(save_path, tracker.pose_es, tracker.pose_gt)
    if "loop_closure" in report:
        lc = report["loop_closure"]
        np.save(os.path.join(save_path, "save_traj", POSE_ES_BEFORE_LOOP_CLOSURE),
                np.stack([np.asarray(p) for p in tracker.pose_es_before_loop_closure], axis=0))
        log(f"loop closure: {lc['edges']} edges of {len(lc['candidates'])} candidates over {lc['keyframes']} keyframes, correction "
            f"max {100 * lc.get('correction_max_m', 0.0):.2f} cm / mean {100 * lc.get('correction_mean_m', 0.0):.2f} cm, ATE "
            f"{100 * lc['ate_rmse_m_before']:.3f} -> {100 * lc['ate_rmse_m']:.3f} cm (aligned "
            f"{100 * lc['ate_rmse_aligned_m_before']:.3f} -> {100 * lc['ate_rmse_aligned_m']:.3f} cm) in {lc['seconds']['total']:.3f} s")
    if "relocalisation" in report:
        rl = report["relocalisation"]
        log(f"relocalise: {len(rl['lost_frames'])} frames lost, {len(rl['events'])} recoveries in {rl['attempts']} attempts, "
            f"refusals {rl['refusals']}")
    ates = prefix_ates(tracker.pose_es, tracker.pose_gt)
    with open(os.path.join(save_path, "save_traj", "ate.txt"), "w") as f:
        f.write("".join(f"{a!r}\n" for a in ates))
    rec = iof.Recorder(device.index or 0)
    for t_track, t_map, _, _ in report["per_frame"]:
        rec.update_mean("tracking", t_track, 1)
        rec.update_mean("mapping", t_map, 1)
    if getattr(args, "record_mem", False):
        rec.watch_gpu()
    rec.cal_fps()
    rec.save(save_path)
    iof.save_metrics_csv(os.path.join(save_path, "eval_metric", "slam_eval.csv"), report.get("eval", []))
    st = source.stats()
    loop_s = loop["t_last"] - loop["t0"]
    report.update(io_wait_s_mean=st["io_wait_s_mean"], io_wait_s=st["io_wait_s"], decode_ms_per_frame=st["decode_ms_per_frame"],
                  io_workers=st["io_workers"], prefetch=st["prefetch"], h2d_bytes_per_frame=st["h2d_bytes_per_frame"],
                  wall_fps_including_io=n / loop_s if loop_s > 0 else None, ate_cm=ates[-1], width=st["width"],
                  height=st["height"], resolution_scale=st["resolution_scale"])
    with open(os.path.join(save_path, "run_report.json"), "w") as f:
        json.dump(report, f, indent=1, default=float)
    log(f"{n} frames: fps {report['fps']:.2f} (1 / mapping), wall fps with I/O {report['wall_fps_including_io']:.2f}, "
        f"io wait {1e3 * st['io_wait_s_mean']:.3f} ms/frame, ATE {ates[-1]:.3f} cm -> {save_path}")
    if getattr(args, "pcd_densify", False):
        if opts.pcd_densify:
            path = os.path.join(save_path, "save_model", DENSIFY_PLY)
            seed = getattr(args, "seed", None)
            gen = torch.Generator().manual_seed(0 if seed is None else int(seed))
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            n_points = mapper.save_densified(path, 1, 30, 5, generator=gen)      # slam.py:147: densify(1, 30, 5)
            log(f"pcd_densify: {n_points} points from {mapper.get_stable_num} stable Gaussians in "
                f"{time.perf_counter() - t0:.3f} s -> {path if n_points else '(empty stable cloud: no file)'}")
        else:
            log("pcd_densify skipped (pass --pcd-densify to write save_model/pcd_densify.ply)")
    return 0


POSE_ES_BEFORE_LOOP_CLOSURE = "pose_es_before_loop_closure.npy"
DENSIFY_PLY = "pcd_densify.ply"
MESH_PLY = "mesh_tsdf.ply"
MESH_REPORT = "mesh_report.json"
MESH_TEXTURED_OBJ = "mesh_textured.obj"
MESH_TEXTURE_PNG = "mesh_texture.png"
GT_CULL_PLY = "gt_mesh_culled.ply"
GT_CULL_REPORT = "gt_cull_report.json"
MESH_DEPTH_REPORT = "mesh_depth_report.json"
MESH_COLOR_REPORT = "mesh_color_report.json"
EXPOSURE_REPORT = "exposure_report.json"
EXPOSURE_COLUMNS = ("frame", "psnr", "psnr_ea", "ssim_ea", "color_l1_ea", "gain_r", "gain_g", "gain_b", "offset_r", "offset_g",
                    "offset_b", "code")
MESH_COLOR_DIR = "mesh_color"


def geometry_ply(args, model_base: str, select_ply: str) -> str:
    """metric.py:156-163: the file the reconstruction metrics are computed on - save_model/pcd_densify.ply when the config
    sets pcd_densify and the file exists, the selected model file otherwise."""
    if getattr(args, "pcd_densify", False):
        path = os.path.join(model_base, DENSIFY_PLY)
        if os.path.exists(path):
            return path
    return select_ply


def filter_models(frame_path: str, eval_merge: bool, load_iter):
    """metric.py:37-66: the model files of a frame directory to evaluate (the stable cloud by default, the merged one with
    eval_merge; the highest iteration unless load_iter names some)."""
    exclude, include = ("stable", "merge") if eval_merge else ("merge", "stable")
    total = [i for i in os.listdir(frame_path) if "sibr" not in i and exclude not in i]
    if not total:
        raise FileNotFoundError(f"rtg_slam_amd: no model file to evaluate in {frame_path} (eval_merge={eval_merge}; an empty "
                                "cloud is not written)")
    select = []
    if len(load_iter) > 0:
        for it in load_iter:
            model_iter = [i for i in total if "%04d" % it in i]
            merged = [i for i in model_iter if include in i]
            select.extend(merged if merged else model_iter)
    else:
        max_iter = sorted([i[5:9] for i in total], reverse=True)[0]
        total = [i for i in total if max_iter in i]
        merged = [i for i in total if include in i]
        select.extend(merged if merged else total)
    return select


def load_map(args, device, ply_path: str):
    """A saved model file as a Mapping: load_model_ply -> model_to_packed -> append_rows, confidence kept, capacity = rows."""
    import torch
    from . import io_formats as iof
    from .mapping import Mapping
    m = iof.load_model_ply(ply_path, int(args.max_sh_degree))
    packed = iof.model_to_packed(m)
    n = int(packed.shape[0])
    if n == 0:
        raise ValueError(f"rtg_slam_amd: {ply_path} holds no Gaussians")
    mapper = Mapping(args, device, capacity=n)
    mapper.opt.append_rows(torch.from_numpy(packed).to(device),
                           aux={"confidence": torch.from_numpy(m["confidence"]).to(device)})
    return mapper


def select_model(args, opts):
    """metric.py:120-135: the frame directory (--load-frame, default the last) and the model file in it (filter_models) ->
    (save_model directory, frame directory name, model path, its iteration as the 4 digits of the file name)."""
    model_base = os.path.join(args.save_path, "save_model")
    frames = sorted(i for i in os.listdir(model_base) if os.path.isdir(os.path.join(model_base, i)))
    if opts.load_frame < 0:
        check_frame = frames[-1]
    else:
        check_frame = [i for i in frames if "%04d" % opts.load_frame in i][0]
    frame_path = os.path.join(model_base, check_frame)
    model = filter_models(frame_path, opts.eval_merge, opts.load_iter)[0]
    return model_base, check_frame, os.path.join(frame_path, model), model[5:9]


def cmd_mesh(opts) -> int:
    import torch
    from . import config, datasets, io_formats as iof, meshing
    args = config.load_config(opts.config)
    _apply_resolution_scale(args, opts)
    device = torch.device(opts.device)
    torch.cuda.set_device(device)
    model_base, check_frame, select_ply, test_iter = select_model(args, opts)
    last = int(check_frame.split("_")[-1])
    n_frames = last if opts.frames is None or opts.frames < 0 else min(opts.frames, last)
    if opts.simplify < 0 or opts.min_component_faces < 0:
        log("--simplify and --min-component-faces must be >= 0")
        return 2
    if opts.simplify > 0 and not opts.simplify > opts.voxel:
        log(f"--simplify {opts.simplify:g}: the cell must be larger than the voxel ({opts.voxel:g} m); a cell that holds one vertex "
            "simplifies nothing")
        return 2
    if opts.cull_unseen_tolerance is not None and (not opts.cull_unseen or opts.cull_unseen_tolerance < 0):
        log("--cull-unseen-tolerance must be >= 0 and needs --cull-unseen")
        return 2
    if not 0 <= opts.decimate < 1:
        log(f"--decimate {opts.decimate:g}: the share of faces to keep must be >= 0 (off) and < 1")
        return 2
    if opts.decimate_max_error is not None and not (opts.decimate > 0 and opts.decimate_max_error > 0):
        log("--decimate-max-error must be > 0 and needs --decimate")
        return 2
    texture_texel = 0.0
    if opts.texture:
        texture_texel = opts.voxel if opts.texture_texel is None else opts.texture_texel
        if not (math.isfinite(texture_texel) and texture_texel > 0):
            log(f"--texture-texel {texture_texel:g}: the texel must be finite and > 0")
            return 2
        if not 1 <= opts.texture_max_level <= meshing.TEXTURE_MAX_LEVEL:
            log(f"--texture-max-level {opts.texture_max_level}: the level must lie in 1..{meshing.TEXTURE_MAX_LEVEL}")
            return 2
    elif opts.texture_texel is not None or opts.texture_max_level != meshing.TEXTURE_MAX_LEVEL:
        log("--texture-texel and --texture-max-level need --texture")
        return 2
    cleanup = opts.min_component_faces > 0 or opts.simplify > 0 or opts.normals or opts.decimate > 0
    log(f"meshing {select_ply} over {n_frames} frames ({opts.depth_source} depth, every {opts.every}, voxel {opts.voxel:g} m)")
    mapper = load_map(args, device, select_ply)
    mapper.time = int(check_frame.split("_")[1])
    mapper.iter = int(test_iter)
    poses = None
    if not args.use_gt_pose:
        poses = np.load(os.path.join(args.save_path, "save_traj", "pose_es.npy")).reshape(-1, 4, 4)[int(args.frame_start):]
    args.frame_num = n_frames
    info = datasets.load_dataset(args)
    source = datasets.FrameSource(info, device, io_workers=opts.io_workers)
    log(f"fusing at {info.width}x{info.height} (resolution scale {info.resolution_scale:g})")
    t0 = time.perf_counter()
    texture_options = {"texture_texel": texture_texel, "texture_max_level": opts.texture_max_level} if opts.texture else {}
    try:
        vertices, faces, colors, report, *normals = meshing.mesh_from_map(
            mapper, info.camera(), poses, source, voxel=opts.voxel, depth_source=opts.depth_source, every=opts.every,
            trunc=opts.trunc_voxels * opts.voxel, min_weight=opts.min_weight, args=args, device=device, volume=opts.volume,
            min_component_faces=opts.min_component_faces, simplify_cell=opts.simplify, normals=opts.normals,
            cull_unseen=opts.cull_unseen, cull_unseen_tolerance=opts.cull_unseen_tolerance, decimate=opts.decimate,
            decimate_max_error=opts.decimate_max_error, **texture_options)
    except ValueError as e:
        if not (opts.texture and "atlas" in str(e)):
            raise
        log(f"--texture: {e}")
        return 2
    texture = normals.pop() if opts.texture else None
    report["total_s"] = time.perf_counter() - t0
    path = os.path.join(model_base, MESH_PLY)
    t0 = time.perf_counter()
    iof.save_mesh_ply(path, vertices, faces, colors, *normals)
    report["write_s"] = time.perf_counter() - t0
    report["model"] = select_ply
    if texture is not None:
        obj = os.path.join(model_base, MESH_TEXTURED_OBJ)
        iof.save_textured_obj(obj, vertices, faces, texture["uv"], texture["image"], *normals, image_name=MESH_TEXTURE_PNG)
    with open(os.path.join(model_base, MESH_REPORT), "w") as f:
        json.dump(report, f, indent=1, default=float)
    log(f"mesh: {report['V']} vertices, {report['F']} faces from {report['frames_fused']} frames into a "
        f"{'x'.join(str(d) for d in report['dims'])} grid: render {report['render_s']:.3f} s, integrate "
        f"{report['integrate_s']:.3f} s, extract {report['extract_s']:.3f} s, write {report['write_s']:.3f} s -> {path}")
    if opts.cull_unseen:
        log(f"cull unseen: {report['F_unseen_removed']} of {report['F_raw']} faces and {report['V_unseen_removed']} of "
            f"{report['V_raw']} vertices no fused view saw (tolerance {report['cull_unseen']:g} m) removed: render "
            f"{report['cull_render_s']:.3f} s")
    if cleanup:
        log(f"clean-up: {report['V_raw']} vertices, {report['F_raw']} faces raw -> {report['V']} vertices, {report['F']} faces; "
            f"{report.get('components_removed', 0)} of {report.get('components', 'all')} components removed"
            f"{', simplified at %g m' % report['simplify_cell'] if report['simplify_cell'] > 0 else ''}"
            f"{', with normals' if report['normals'] else ''}: {report['cleanup_s']:.3f} s")
    if opts.decimate > 0:
        log(f"decimation: {report['F_before_decimate']} faces -> {report['F']} faces ({100 * opts.decimate:g} % asked for"
            f"{', error <= %g m' % report['decimate_max_error'] if report['decimate_max_error'] is not None else ''}); "
            f"{report['decimate_collapses']} collapses in {report['decimate_rounds']} rounds, target "
            f"{'reached' if report['decimate_target_reached'] else 'NOT reached'}: {report['decimate_s']:.3f} s")
    if texture is not None:
        stats = texture["stats"]
        log(f"texture: {stats['size'][0]} x {stats['size'][1]}, {100 * stats['fill']:.1f} % filled, {100 * stats['seen_share']:.1f} % of "
            f"the assigned texels seen by {stats['views']} views -> {obj}")
    if opts.volume == "sparse":
        log(f"sparse volume: {report['bricks']} bricks, {100 * report['brick_share']:.2f} % of the grid's, "
            f"{report['pool_bytes'] / 2 ** 20:.1f} MiB of pool where the dense planes would take {report['dense_bytes'] / 2 ** 20:.1f} MiB")
    return 0


def cmd_metric(opts) -> int:
    import torch
    from . import config, datasets, evaluation, io_formats as iof
    args = config.load_config(opts.config)
    _apply_resolution_scale(args, opts)
    device = torch.device(opts.device)
    torch.cuda.set_device(device)
    model_base, check_frame, select_ply, test_iter = select_model(args, opts)
    last = int(check_frame.split("_")[-1])
    max_cams = last if opts.eval_frames < 0 else min(opts.eval_frames, last)
    log(f"evaluating {select_ply} over {max_cams} frames")
    pcd_path = geometry_ply(args, model_base, select_ply)
    log(f"geometry eval ply: {pcd_path}")
    mesh_path = None
    if opts.mesh:
        mesh_path = os.path.join(model_base, MESH_PLY)
        if not os.path.isfile(mesh_path):
            log(f"--mesh: {mesh_path} does not exist; write it first with `python -m rtg_slam_amd mesh --config {opts.config}`")
            return 2
    if opts.mesh_depth:
        mesh_depth_path = os.path.join(model_base, MESH_PLY)
        if not os.path.isfile(mesh_depth_path):
            log(f"--mesh-depth: {mesh_depth_path} does not exist; write it first with `python -m rtg_slam_amd mesh --config {opts.config}`")
            return 2
    if opts.mesh_color_save_every is not None and (opts.mesh_color is None or opts.mesh_color_save_every < 1):
        log("--mesh-color-save-every K needs --mesh-color and K >= 1")
        return 2
    color_ply, color_obj = None, None
    if opts.mesh_color in ("vertex", "both"):
        path = os.path.join(model_base, MESH_PLY)
        if not os.path.isfile(path):
            log(f"--mesh-color {opts.mesh_color}: {path} does not exist; write it first with `python -m rtg_slam_amd mesh --config {opts.config}`")
            return 2
        color_ply = iof.load_mesh_ply(path, with_colors=True)
        if color_ply[2] is None:
            log(f"--mesh-color {opts.mesh_color}: {path} holds no vertex colours; write it again with `python -m rtg_slam_amd mesh "
                f"--config {opts.config}`")
            return 2
    if opts.mesh_color in ("texture", "both"):
        path = os.path.join(model_base, MESH_TEXTURED_OBJ)
        if not os.path.isfile(path):
            log(f"--mesh-color {opts.mesh_color}: {path} does not exist; write it first with `python -m rtg_slam_amd mesh --config "
                f"{opts.config} --texture`")
            return 2
        color_obj = iof.load_textured_obj(path)
    if opts.surface_distance and not opts.mesh:
        log("--surface-distance needs --mesh")
        return 2
    if opts.surface_max_distance is not None:
        if not opts.surface_distance:
            log("--surface-max-distance needs --surface-distance")
            return 2
        if not (0.03 < opts.surface_max_distance < float("inf")):        # NaN too
            log("--surface-max-distance must be a finite number of metres above the F-score threshold 0.03")
            return 2
    if opts.align and (not opts.align_max_distance > 0 or opts.align_iterations < 1):
        log("--align-max-distance must be > 0 (metres) and --align-iterations >= 1")
        return 2
    if opts.cull_depth == "mesh" and not opts.cull_gt:
        log("--cull-depth mesh needs --cull-gt")
        return 2
    if opts.cull_gt and (opts.cull_tolerance < 0 or opts.cull_min_views < 1):
        log("--cull-tolerance must be >= 0 and --cull-min-views >= 1")
        return 2
    mapper = load_map(args, device, select_ply)
    mapper.time = int(check_frame.split("_")[1])
    mapper.iter = int(test_iter)
    poses = None
    if not args.use_gt_pose:
        poses = np.load(os.path.join(args.save_path, "save_traj", "pose_es.npy")).reshape(-1, 4, 4)[int(args.frame_start):]
    args.frame_num = max_cams
    info = datasets.load_dataset(args)
    if opts.cull_gt and not (info.mesh_path and os.path.isfile(info.mesh_path)):
        log(f"--cull-gt: there is no GT mesh to cull ({info.mesh_path or 'this dataset type has none'})")
        return 2
    if opts.surface_distance and not (info.mesh_path and os.path.isfile(info.mesh_path)):
        log(f"--surface-distance: there is no GT mesh to measure against ({info.mesh_path or 'this dataset type has none'})")
        return 2
    if opts.align and not (info.mesh_path and os.path.isfile(info.mesh_path)):
        log(f"--align: there is no GT mesh to align to ({info.mesh_path or 'this dataset type has none'})")
        return 2
    source = datasets.FrameSource(info, device, io_workers=opts.io_workers)
    log(f"evaluating at {info.width}x{info.height} (resolution scale {info.resolution_scale:g})")
    gt_points, transform, rec_points, gt_cull = None, None, None, None
    mesh_renderer, gt_mesh_renderer = None, None
    if info.mesh_path and os.path.isfile(info.mesh_path):
        v, f = iof.load_mesh_ply(info.mesh_path)
        transform = datasets.read_pose_t0(args)
        if opts.cull_gt:                     # the GT points are sampled from the culled mesh, after the last frame
            gt_cull = evaluation.VisibilityCull(v, f, info.camera(), transform=transform, tolerance=opts.cull_tolerance,
                                                min_views=opts.cull_min_views, any_vertex=opts.cull_keep == "any", device=device)
        else:
            gt_points, _ = iof.sample_mesh_surface(v, f, 1_000_000)
        if opts.mesh_depth or opts.cull_depth == "mesh":
            gt_mesh_renderer = evaluation.MeshRenderer(v, f, info.camera(), transform=transform, device=device)
        if mesh_path is not None:
            log(f"geometry eval mesh: {mesh_path}")
            mv, mf = iof.load_mesh_ply(mesh_path)
            if mf.shape[0] == 0:
                raise ValueError(f"rtg_slam_amd: {mesh_path} holds no faces")
            rec_points = evaluation.sample_mesh_points(mv, mf, 1_000_000, 0, device)
        elif pcd_path != select_ply:
            xyz, _ = iof.load_point_cloud_ply(pcd_path)
            if xyz.shape[0] == 0:
                raise ValueError(f"rtg_slam_amd: {pcd_path} holds no points")
            rec_points = torch.from_numpy(xyz).to(device=device, dtype=torch.float32)
    if opts.mesh_depth or color_ply is not None:       # the mesh lies in the stream's frame: no transform
        mv, mf, mc = color_ply if color_ply is not None else (*iof.load_mesh_ply(os.path.join(model_base, MESH_PLY)), None)
        mesh_renderer = evaluation.MeshRenderer(mv, mf, info.camera(), device=device, colors=mc)
    color_kw, texture_renderer = {}, None
    if color_obj is not None:                # the OBJ's own vertices and faces: the final mesh, which the PLY need not be
        texture_renderer = evaluation.MeshRenderer(color_obj[0], color_obj[1], info.camera(), device=device, uv=color_obj[2],
                                                   texture=color_obj[3])
        if mesh_renderer is None:
            mesh_renderer = texture_renderer
        else:
            color_kw["mesh_texture_renderer"] = texture_renderer
    md_dir = os.path.join(args.save_path, "eval_metric")
    if opts.mesh_color is not None:
        color_kw["mesh_color"] = opts.mesh_color
        if opts.mesh_color_save_every is not None:
            from PIL import Image
            os.makedirs(os.path.join(md_dir, MESH_COLOR_DIR), exist_ok=True)

            def save_render(i, name, picture):
                if i % opts.mesh_color_save_every == 0:
                    q = torch.floor(picture * 255.0 + 0.5).clamp(0.0, 255.0).to(torch.uint8).permute(1, 2, 0).contiguous()
                    Image.fromarray(q.cpu().numpy()).save(os.path.join(md_dir, MESH_COLOR_DIR, f"frame_{i:04d}_{name}.png"))
            color_kw["mesh_color_hook"] = save_render
    res = evaluation.evaluate_sequence(mapper, info.camera(), source, poses=poses, args=args, gt_points=gt_points,
                                       dist_thres=[0.03], transform=transform, sample_nums=1_000_000, rec_points=rec_points,
                                       gt_cull=gt_cull, mesh_renderer=mesh_renderer, gt_mesh_renderer=gt_mesh_renderer,
                                       gt_cull_depth=opts.cull_depth, exposure_aware=bool(opts.exposure_aware), **color_kw)
    if opts.exposure_aware:
        os.makedirs(md_dir, exist_ok=True)
        ea_path = os.path.join(md_dir, f"exposure_frame_{mapper.time}_iter_{test_iter}.csv")
        rows = res["exposure_rows"]
        with open(ea_path, "w") as fo:
            fo.write(",".join(EXPOSURE_COLUMNS) + "\n")
            fo.write("".join(",".join(repr(r[k]) for k in EXPOSURE_COLUMNS) + "\n" for r in rows))
        ea = dict(res["exposure_mean"])
        ea.update(frames=len(rows), gates=evaluation.exposure_settings(info.height, info.width), device_s=res["exposure_seconds"])
        with open(os.path.join(md_dir, EXPOSURE_REPORT), "w") as fo:
            json.dump(ea, fo, indent=1, default=float)
        log(f"exposure-aware: PSNR {ea.get('psnr', float('nan')):.3f} -> {ea.get('psnr_ea', float('nan')):.3f} dB over {len(rows)} "
            f"frames, {ea['frames_refused']} refused -> {ea_path}")
    if gt_cull is not None:
        cull_dir = os.path.join(args.save_path, "eval_metric")
        os.makedirs(cull_dir, exist_ok=True)
        cull_path = os.path.join(cull_dir, GT_CULL_PLY)
        iof.save_mesh_ply(cull_path, *gt_cull.mesh())
        report = gt_cull.report()
        report["gt_mesh"] = info.mesh_path
        if opts.cull_depth == "mesh":
            report["depth"] = "mesh"
        with open(os.path.join(cull_dir, GT_CULL_REPORT), "w") as fo:
            json.dump(report, fo, indent=1, default=float)
        log(f"geometry eval gt: culled {report['F_kept']} of {report['F']} faces over {report['frames']} frames -> {cull_path}")
    if opts.mesh_depth:
        os.makedirs(md_dir, exist_ok=True)
        md_path = os.path.join(md_dir, f"mesh_depth_frame_{mapper.time}_iter_{test_iter}.csv")
        rows = res["mesh_depth_rows"]
        with open(md_path, "w") as fo:
            keys = list(rows[0]) if rows else ["frame", "mesh_valid_ratio", "mesh_depth_l1"]
            fo.write(",".join(keys) + "\n")
            fo.write("".join(",".join(repr(r[k]) for k in keys) + "\n" for r in rows))
        md = dict(res["mesh_depth_mean"])
        md.update(frames=len(rows), near=mesh_renderer.near, mesh=os.path.join(model_base, MESH_PLY),
                  render_s=mesh_renderer.seconds, gt_render_s=gt_mesh_renderer.seconds if gt_mesh_renderer is not None else None)
        with open(os.path.join(md_dir, MESH_DEPTH_REPORT), "w") as fo:
            json.dump(md, fo, indent=1, default=float)
        log(f"mesh depth: L1 {100 * md.get('mesh_depth_l1', float('nan')):.3f} cm over {md.get('mesh_valid_ratio', float('nan')):.4f} "
            f"of the pixels, {len(rows)} frames -> {md_path}")
    if opts.mesh_color is not None:
        os.makedirs(md_dir, exist_ok=True)
        mc_path = os.path.join(md_dir, f"mesh_color_frame_{mapper.time}_iter_{test_iter}.csv")
        rows = res["mesh_color_rows"]
        suffixes = [s for s, name in (("", "vertex"), ("_tex", "texture")) if opts.mesh_color in (name, "both")]
        keys = ["frame"] + [k + s for s in suffixes for k in ("mesh_hit_ratio", "mesh_psnr", "mesh_ssim", "mesh_color_l1", "mesh_color_l1_hit")]
        with open(mc_path, "w") as fo:
            fo.write(",".join(keys) + "\n")
            fo.write("".join(",".join(repr(r[k]) for k in keys) + "\n" for r in rows))
        mc = dict(res["mesh_color_mean"])
        mc.update(frames=len(rows), source=opts.mesh_color, near=mesh_renderer.near,
                  mesh=os.path.join(model_base, MESH_PLY) if color_ply is not None else None,
                  textured_mesh=os.path.join(model_base, MESH_TEXTURED_OBJ) if color_obj is not None else None,
                  atlas_size=[int(color_obj[3].shape[1]), int(color_obj[3].shape[0])] if color_obj is not None else None,
                  render_s=mesh_renderer.seconds if color_ply is not None else None,
                  texture_render_s=texture_renderer.seconds if texture_renderer is not None else None,
                  saved_every=opts.mesh_color_save_every)
        with open(os.path.join(md_dir, MESH_COLOR_REPORT), "w") as fo:
            json.dump(mc, fo, indent=1, default=float)
        db = lambda k: f"{mc[k]:.3f} dB" if k in mc else "-"
        log(f"mesh colour: PSNR {db('mesh_psnr')} (vertex) / {db('mesh_psnr_tex')} (texture), hit ratio "
            f"{mc.get('mesh_hit_ratio', mc.get('mesh_hit_ratio_tex', float('nan'))):.4f}, {len(rows)} frames -> {mc_path}")
    if opts.surface_distance:               # the reconstructed mesh against the GT surface (the culled one with --cull-gt)
        gv, gf = gt_cull.mesh() if gt_cull is not None else iof.load_mesh_ply(info.mesh_path)
        mv, mf = iof.load_mesh_ply(mesh_path)
        reports = {}
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        trunc = {} if opts.surface_max_distance is None else {"max_distance": opts.surface_max_distance}
        sd = evaluation.eval_mesh_surface(mv, mf, gv, gf, dist_thres=[0.03], transform=transform, sample_nums=1_000_000,
                                          device=device, reports=reports, **trunc)
        sd.update(V=int(mv.shape[0]), F=int(mf.shape[0]), V_gt=int(gv.shape[0]), F_gt=int(gf.shape[0]), mesh=mesh_path,
                  gt_mesh=info.mesh_path, gt_culled=gt_cull is not None, distance_gt=reports["gt"], distance_rec=reports["rec"],
                  seconds=time.perf_counter() - t0)
        sd_dir = os.path.join(args.save_path, "eval_metric")
        os.makedirs(sd_dir, exist_ok=True)
        sd_path = os.path.join(sd_dir, f"surface_distance_frame_{mapper.time}_iter_{test_iter}.json")
        with open(sd_path, "w") as fo:
            json.dump(sd, fo, indent=1, default=float)
        log(f"surface distance: accuracy {sd['accuracy']:.4f} cm, completion {sd['completion']:.4f} cm, F1 {sd['F1 (< 0.03)']:.3f}, "
            f"normal consistency {sd['normal_consistency']:.4f} -> {sd_path}")
        if trunc:
            log(f"surface distance truncated at {sd['max_distance']:g} m: {sd['beyond_acc']} / {sd['beyond_comp']} samples beyond")
    if opts.align:                           # register the scored geometry to the FULL GT surface, then score it again
        from . import mesh_ops
        gv, gf = iof.load_mesh_ply(info.mesh_path)
        with torch.no_grad():
            src = mapper.opt.gaussian_data("all")["xyz"].detach() if rec_points is None else rec_points
        normals, kw = None, {}
        if mesh_path is not None:            # the samples' own face normals: the draw of sample_mesh_points, again
            mv, mf = iof.load_mesh_ply(mesh_path)
            _, own = iof.sample_mesh_surface(mv, mf, 1_000_000, 0)
            dv = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt).contiguous()
            normals = mesh_ops.face_unit_normals(dv(mv, torch.float32).reshape(-1, 3), dv(mf, torch.int64).reshape(-1, 3).to(torch.int32),
                                                 dv(own, torch.int32))
            kw["min_cos"] = 0.5
        reports = {}
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        T_total, reg = evaluation.align_to_gt(src, gv, gf, transform=transform, source_normals=normals, reports=reports,
                                              max_distance=opts.align_max_distance, max_iterations=opts.align_iterations, **kw)
        seconds = time.perf_counter() - t0
        T_align = T_total @ np.linalg.inv(np.asarray(transform, dtype=np.float64).reshape(4, 4))
        same_gt = gt_points                  # the GT points the unaligned figures were scored against
        if gt_cull is not None:
            same_gt = evaluation.sample_mesh_points(*gt_cull.mesh(), 1_000_000, 0, device)
        aligned = evaluation.eval_pcd(src, same_gt, [0.03], T_total, 1_000_000)
        row = res["rows"][-1] if res["rows"] else {}
        unaligned = {k: row[k] for k in aligned} if all(k in row for k in aligned) else \
            evaluation.eval_pcd(src, same_gt, [0.03], transform, 1_000_000)
        al = {"transform": T_align.tolist(), "transform_total": T_total.tolist(), "registration": reg, "unaligned": unaligned,
              "aligned": aligned, "source": mesh_path if mesh_path is not None else pcd_path, "gt_mesh": info.mesh_path,
              "gt_culled": gt_cull is not None, "max_distance": opts.align_max_distance, "max_iterations": opts.align_iterations,
              "distance_gt": reports["gt"], "seconds": seconds}
        if opts.surface_distance:            # sd: the unaligned surface figures, written above
            sgv, sgf = gt_cull.mesh() if gt_cull is not None else (gv, gf)
            al["surface_aligned"] = evaluation.eval_mesh_surface(mv, mf, sgv, sgf, dist_thres=[0.03], transform=T_total,
                                                                 sample_nums=1_000_000, device=device, **trunc)
            al["surface_unaligned"] = {k: sd[k] for k in al["surface_aligned"]}
        al_dir = os.path.join(args.save_path, "eval_metric")
        os.makedirs(al_dir, exist_ok=True)
        al_path = os.path.join(al_dir, f"aligned_frame_{mapper.time}_iter_{test_iter}.json")
        with open(al_path, "w") as fo:
            json.dump(al, fo, indent=1, default=float)
        log(f"aligned: rotation {reg['rotation_deg']:.4f} deg, translation {100 * reg['translation_m']:.4f} cm, "
            f"{reg['inlier_share']:.4f} inliers; accuracy {unaligned['accuracy']:.4f} -> {aligned['accuracy']:.4f} cm, completion "
            f"{unaligned['completion']:.4f} -> {aligned['completion']:.4f} cm, F1 {unaligned['F1 (< 0.03)']:.3f} -> "
            f"{aligned['F1 (< 0.03)']:.3f} -> {al_path}")
    out = os.path.join(args.save_path, f"statis_frame_{mapper.time}_iter_{test_iter}.csv")
    iof.save_metrics_csv(out, res["rows"])
    m = res["mean"]
    log(f"{len(res['rows'])} frames: psnr {m.get('psnr')}, ssim {m.get('ssim')}, depth L1 {m.get('depth_loss')} -> {out}")
    return 0


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m rtg_slam_amd", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("slam", help="run SLAM on a dataset (slam.py)")
    s.add_argument("--config", required=True)
    s.add_argument("--frames", type=int, default=None, help="overrides frame_num")
    s.add_argument("--device", default="cuda:0")
    s.add_argument("--io-workers", type=int, default=None)
    s.add_argument("--overwrite", action="store_true", help="replace a non-empty save_path")
    s.add_argument("--resolution-scale", type=float, default=None,
                   help="overrides resolution_scales[0]: the frames are resized to 1/S of their size on the device (loadCam)")
    s.add_argument("--pcd-densify", action="store_true",
                   help="when the config sets pcd_densify, write save_model/pcd_densify.ply after the run (slam.py:146-150)")
    s.add_argument("--rgbd-refine", action="store_true",
                   help="refine every ICP pose with the joint photometric + geometric RGB-D alignment (rtg_slam_amd.rgbd_align)")
    s.add_argument("--rgbd-refine-photo-weight", type=float, default=None, metavar="L",
                   help="metres per unit of intensity (default 0.25, derived from nominal noise levels, not measured)")
    s.add_argument("--rgbd-refine-huber", type=float, default=None, metavar="D",
                   help="Huber threshold of the intensity residual (default 0.05, a choice, not measured)")
    s.add_argument("--rgbd-refine-target", choices=("frame", "model"), default=None,
                   help="photometric target of --rgbd-refine: the previous frame's colour (default) or the map's rendered colour")
    s.add_argument("--rgbd-refine-exposure", action="store_true",
                   help="--rgbd-refine also solves for a gain and an offset between the frame's and the target's intensity")
    s.add_argument("--map-exposure", action="store_true",
                   help="fit every frame's gain and offset to the map and feed the mapper the corrected colour")
    s.add_argument("--map-exposure-channels", choices=("grey", "rgb"), default=None,
                   help="with --map-exposure: one gain and offset on the grey values (default) or one per colour channel (white balance)")
    s.add_argument("--loop-closure", action="store_true",
                   help="close loops once, after the last frame: keyframe pose graph, corrected trajectory, deformed map "
                        "(rtg_slam_amd.loop_closure); the defaults of its values are derived, not measured")
    for name, typ, meta, text in LOOP_CLOSURE_FLAGS:
        if isinstance(typ, tuple):
            s.add_argument("--loop-closure-" + name.replace("_", "-"), type=float, nargs=2, default=None, metavar=meta, help=text)
        elif name in LOOP_CLOSURE_CHOICES:
            s.add_argument("--loop-closure-" + name.replace("_", "-"), choices=LOOP_CLOSURE_CHOICES[name], default=None, help=text)
        else:
            s.add_argument("--loop-closure-" + name.replace("_", "-"), type=typ, default=None, metavar=meta, help=text)
    s.add_argument("--relocalise", action="store_true",
                   help="a frame the ICP tracker cannot hold is not mapped; it and the frames after it are searched for among "
                        "the keyframes (thumbnails, keypoints, a device RANSAC, a gated registration) until one is recovered "
                        "(rtg_slam_amd.relocalisation)")
    for name, typ, meta, text in RELOCALISE_FLAGS:
        s.add_argument("--relocalise-" + name.replace("_", "-"), type=typ, default=None, metavar=meta, help=text)
    s.add_argument("--relocalise-search", choices=("thumbnails", "keypoints"), default=None,
                   help="how a lost frame's keyframes are shortlisted: by thumbnail score (default) or by the votes of its keypoints "
                        "against every keyframe's, for a return at another distance than any keyframe saw")
    s.add_argument("--loop-closure-keypoint-ransac", choices=("host", "device"), default=None,
                   help="where the keypoint pose's match filter and RANSAC run: on the host per candidate (default), or in one "
                        "rtgs_rigid_ransac launch for all candidates")
    s.add_argument("--loop-closure-rotate-sh", action="store_true",
                   help="the deformed map's higher SH bands turn with each frame's correction as well (rtgs_map_deform_sh); "
                        "without it they keep pointing where they did (default)")
    m = sub.add_parser("metric", help="evaluate a saved model (metric.py)")
    m.add_argument("--config", required=True)
    m.add_argument("--load-frame", type=int, default=-1)
    m.add_argument("--load-iter", type=int, nargs="+", default=[])
    m.add_argument("--eval-frames", type=int, default=-1)
    m.add_argument("--eval-merge", action="store_true")
    m.add_argument("--device", default="cuda:0")
    m.add_argument("--io-workers", type=int, default=None)
    m.add_argument("--resolution-scale", type=float, default=None,
                   help="overrides resolution_scales[0]; evaluate at the scale the map was built at (metric.py:131,177)")
    m.add_argument("--mesh", action="store_true",
                   help="compute the reconstruction metrics on 1 M points sampled from save_model/mesh_tsdf.ply (written by `mesh`)")
    m.add_argument("--cull-gt", action="store_true",
                   help="score the geometry against the part of the GT mesh the evaluated frames saw (so --eval-frames bounds "
                        "it): a vertex is seen when it projects, at a frame's GT pose, into a pixel whose sensor depth is valid and "
                        "not more than the tolerance in front of it; writes eval_metric/gt_mesh_culled.ply and gt_cull_report.json")
    m.add_argument("--cull-tolerance", type=float, default=0.03,
                   help="metres a vertex may lie behind the sensor depth and still count as seen (default 0.03, the F-score threshold)")
    m.add_argument("--cull-min-views", type=int, default=1, help="frames that must see a vertex (default 1)")
    m.add_argument("--cull-keep", choices=("all", "any"), default="all",
                   help="keep a face when all of its corners were seen (default) or when any was")
    m.add_argument("--cull-depth", choices=("sensor", "mesh"), default="sensor",
                   help="with --cull-gt: test the GT vertices against the sensor depth (default) or against the GT mesh's own "
                        "depth rendered at the GT pose, which has no holes and no noise")
    m.add_argument("--mesh-depth", action="store_true",
                   help="render save_model/mesh_tsdf.ply at every evaluated pose and write its depth L1 against the sensor depth "
                        "(and against the GT mesh rendered at the GT pose, where there is one) to eval_metric/mesh_depth_frame_F_iter_I.csv "
                        "and eval_metric/mesh_depth_report.json")
    m.add_argument("--mesh-color", choices=("vertex", "texture", "both"), default=None,
                   help="render the mesh in colour at every evaluated pose and score it against the frame's colour: save_model/"
                        "mesh_tsdf.ply in its vertex colours, save_model/mesh_textured.obj (written by `mesh --texture`) with its "
                        "atlas, or both; writes eval_metric/mesh_color_frame_F_iter_I.csv and eval_metric/mesh_color_report.json")
    m.add_argument("--mesh-color-save-every", type=int, default=None, metavar="K",
                   help="with --mesh-color: also write every K-th colour render (K >= 1) as an 8-bit PNG, "
                        "eval_metric/mesh_color/frame_XXXX_vertex.png or frame_XXXX_texture.png")
    m.add_argument("--surface-distance", action="store_true",
                   help="with --mesh: score save_model/mesh_tsdf.ply against the GT SURFACE (with --cull-gt: the culled one) by exact "
                        "point-to-triangle distances - accuracy from 1 M samples of the mesh to the GT surface, completion from 1 M "
                        "samples of the GT mesh to the mesh's surface, and the normal consistency - and write "
                        "eval_metric/surface_distance_frame_F_iter_I.json; the statis csv is what it is without the flag")
    m.add_argument("--surface-max-distance", type=float, default=None, metavar="D",
                   help="with --surface-distance: ask only for the nearest face within D metres (D > 0.03) - bounded time against "
                        "an un-culled GT; a distance beyond D counts as D in accuracy and completion, P / R / F1 are unchanged, and "
                        "the JSON gains max_distance, beyond_acc and beyond_comp (the samples beyond D)")
    m.add_argument("--exposure-aware", action="store_true",
                   help="also score every render after an affine colour correction per channel towards the frame (a robust fit on "
                        "the device, rtg_slam_amd.evaluation.exposure_aware_picture): eval_metric/exposure_frame_F_iter_I.csv and "
                        "eval_metric/exposure_report.json; every other file is what it is without the flag")
    m.add_argument("--align", action="store_true",
                   help="after the evaluation, register the scored geometry (the mesh samples with --mesh, else pcd_densify.ply's "
                        "points, else the Gaussian centres) rigidly to the FULL GT surface by point-to-plane ICP on exact nearest "
                        "faces, score it again under that transform against the same GT points, and write the transform, the "
                        "registration report and both sets of figures to eval_metric/aligned_frame_F_iter_I.json; every other "
                        "file is what it is without the flag")
    m.add_argument("--align-max-distance", type=float, default=0.10, metavar="D",
                   help="with --align: correspondences farther than D metres from the GT surface take no part (default 0.10)")
    m.add_argument("--align-iterations", type=int, default=30, metavar="K",
                   help="with --align: at most K Gauss-Newton updates (default 30)")
    t = sub.add_parser("mesh", help="fuse the map into a TSDF volume and write save_model/mesh_tsdf.ply")
    t.add_argument("--config", required=True)
    t.add_argument("--load-frame", type=int, default=-1)
    t.add_argument("--load-iter", type=int, nargs="+", default=[])
    t.add_argument("--eval-merge", action="store_true")
    t.add_argument("--voxel", type=float, default=0.01, help="voxel edge in metres")
    t.add_argument("--trunc-voxels", type=float, default=4.0, help="truncation distance in voxels")
    t.add_argument("--depth-source", choices=("render", "sensor"), default="render",
                   help="fuse the map's rendered depth and colour (default) or the dataset's own")
    t.add_argument("--volume", choices=("dense", "sparse"), default="dense",
                   help="dense planes over the whole box (default) or planes only for the 8x8x8 bricks near the surface")
    t.add_argument("--every", type=int, default=1, help="fuse every K-th frame")
    t.add_argument("--frames", type=int, default=None, help="fuse at most this many frames of the trajectory")
    t.add_argument("--min-weight", type=float, default=1.0, help="observations a cell's 8 corners need to be meshed")
    t.add_argument("--min-component-faces", type=int, default=0,
                   help="drop the connected components with fewer faces (default 0: off)")
    t.add_argument("--simplify", type=float, default=0.0, metavar="CELL",
                   help="cluster the vertices on a grid of CELL metres, larger than the voxel (default 0: off)")
    t.add_argument("--normals", action="store_true", help="write per-vertex normals (nx ny nz) into the PLY")
    t.add_argument("--decimate", type=float, default=0.0, metavar="R",
                   help="after the other clean-up, collapse edges by quadric error until the share R of the faces is left, "
                        "0 <= R < 1 (default 0: off); vertices are removed, never moved")
    t.add_argument("--decimate-max-error", type=float, default=None, metavar="E",
                   help="with --decimate: refuse a collapse whose error exceeds E metres, even if the target is then not reached")
    t.add_argument("--cull-unseen", action="store_true",
                   help="after the extraction, remove the faces with a corner no fused view saw: the mesh is rendered at every "
                        "fused pose and its vertices are tested against that depth")
    t.add_argument("--cull-unseen-tolerance", type=float, default=None, metavar="T",
                   help="metres a vertex may lie behind the rendered depth and still count as seen (default: the voxel)")
    t.add_argument("--texture", action="store_true",
                   help="after everything else, bake a texture atlas for the final mesh from the map rendered at the fused poses and "
                        "write save_model/mesh_textured.obj, mesh_textured.mtl and mesh_texture.png; mesh_tsdf.ply is unchanged")
    t.add_argument("--texture-texel", type=float, default=None, metavar="T",
                   help="with --texture: the edge of a texel on the surface in metres (default: the voxel)")
    t.add_argument("--texture-max-level", type=int, default=6, metavar="L",
                   help="with --texture: a face's block is at most 2^L texels wide, L in 1..6 (default 6)")
    t.add_argument("--device", default="cuda:0")
    t.add_argument("--io-workers", type=int, default=None)
    t.add_argument("--resolution-scale", type=float, default=None,
                   help="overrides resolution_scales[0]; mesh at the scale the map was built at")
    return p


def main(argv=None) -> int:
    opts = build_parser().parse_args(argv)
    return {"slam": cmd_slam, "metric": cmd_metric, "mesh": cmd_mesh}[opts.cmd](opts)


if __name__ == "__main__":
    sys.exit(main())
