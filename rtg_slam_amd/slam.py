"""The single-process SLAM loop of the reference (/root/reference/slam.py:56-95) on this package's pieces: per frame
`Tracker.map_preprocess` -> `Tracker.tracking` (IcpTracker.predict_pose, frame-to-model) -> `Mapping.mapping` ->
`Mapping.get_render_output` -> `Tracker.update_last_status`, with the reference's time recorder semantics
(utils/monitor.py:22-34: `tracking` and `mapping` are running means of the per-frame wall time, fps = 1 / mapping).

`Tracker` mirrors SLAM/multiprocess/tracker.py:97-290 without the ORB backend: the frame maps come from one fused kernel
(slam_ops.frame_preprocess), the pose from rtg_slam_amd.icp.IcpTracker.  BASELINE.json configs[2] is `run_sequence` over a
Replica-shaped stream; bench.py's `sequence` leg and tests/test_sequence_gpu.py call it.  HIP tensors only."""
from __future__ import annotations

import time
from typing import Callable, Iterable, Optional

import numpy as np
import torch

from .mapping import Frame, Mapping


class Tracker:
    def __init__(self, args, device):
        from . import slam_ops
        from .icp import IcpTracker
        self.args, self.device, self.so = args, device, slam_ops
        self.icp_tracker = IcpTracker(args)
        self.pose_es, self.pose_gt = [], []
        self.initialized = False
        self.curr_frame = None
        # extension (off by default): the RGB-D refinement of rtg_slam_amd.rgbd_align after every ICP track
        self.rgbd_refiner = None
        self.intensity_pyramid_t0 = None
        self._intensity_t1 = None
        self._K_host = None
        self.rgbd_reports = []
        # rgbd_refine_target "model": the next frame's photometric target is the map's rendered colour (update_last_status);
        # rgbd_refine_exposure: the refinement also solves for the gain and offset between source and target
        self.rgbd_target = str(getattr(args, "rgbd_refine_target", "frame"))
        self.rgbd_exposure = (1.0, 0.0)                                       # of the frame last refined, into its target's
        self._color_t1 = None
        # extension (off by default): `relocalise` - run_sequence sets the relocaliser; lost_frames are the frames that kept the
        # last good pose and were not mapped
        self.relocaliser = None
        self.lost = False
        self.lost_frames = []
        if self.rgbd_target not in ("frame", "model"):
            raise ValueError(f"rgbd_refine_target must be 'frame' or 'model', not {self.rgbd_target!r}")
        if not bool(getattr(args, "rgbd_refine", False)):
            if self.rgbd_target != "frame" or bool(getattr(args, "rgbd_refine_exposure", False)):
                raise ValueError("rgbd_refine_target: model and rgbd_refine_exposure need rgbd_refine: they are options of that stage")
        if bool(getattr(args, "rgbd_refine", False)):
            from .rgbd_align import RgbdRefiner
            self.rgbd_refiner = RgbdRefiner(args)

    def map_preprocess(self, frame: Frame, depth: torch.Tensor, color: torch.Tensor, frame_id: int):
        """tracker.py:97-159: range mask, vertex / normal / confidence maps, confidence mask; the tracker's current status."""
        a = self.args
        fm = self.so.frame_preprocess(depth, frame.K, a.min_depth, a.max_depth, a.depth_filter, a.invalid_confidence_thresh)
        fm["color_map"] = color.permute(1, 2, 0).contiguous()
        fm["color_chw"] = color.contiguous()
        fm["depth_chw"] = fm["depth_map"].permute(2, 0, 1).contiguous()
        fm["time"] = frame_id
        self.curr_frame = {"K": frame.K, "frame_id": frame_id}
        self.icp_tracker.update_curr_status(fm["depth_map"], frame.K)
        return fm

    def tracking(self, frame: Frame, frame_map, pose_gt=None, init_pose=None):
        """tracker.py:259-290."""
        ok = True
        if pose_gt is not None:
            self.pose_gt.append(np.asarray(pose_gt, dtype=np.float64))
        if self.args.use_gt_pose:
            pose = self.pose_gt[-1]
        elif not self.initialized:
            self.initialized = True
            pose = np.eye(4) if init_pose is None else np.asarray(init_pose, dtype=np.float64)
        elif self.relocaliser is not None:
            pose, ok = self._track_or_relocalise(frame_map)
            if self.lost:
                # a lost frame: the last good pose, one row of pose_es all the same; the ICP state and the photometric target
                # stay those of the last tracked frame, and nothing is prepared for the mapper
                self.pose_es.append(pose)
                self.lost_frames.append(int(self.curr_frame["frame_id"]))
                frame.updatePose(pose)
                return False
        else:
            rel, ok = self.icp_tracker.predict_pose(self.curr_frame)
            if self.rgbd_refiner is not None:
                rel = self._rgbd_refine(rel, frame_map)
            pose = self.pose_es[-1] @ rel.astype(np.float64)
        self.icp_tracker.move_last_status()
        if self.rgbd_refiner is not None and not self.args.use_gt_pose:
            self.intensity_pyramid_t0 = self._intensity_pyramid(frame_map)       # the next frame's target
            if self.rgbd_target == "model":
                self._color_t1 = frame_map["color_chw"]                          # for the composite of update_last_status
        self.pose_es.append(pose)
        frame.updatePose(pose)
        c2w = frame.get_c2w                                                   # transform_map, SLAM/utils.py:56-63; tracker.py:283-288
        rot = frame.get_rot                                                   # get_rot(c2w): translation cleared
        frame_map["vertex_map_w"] = self.so.transform_map(frame_map["vertex_map_c"], c2w)
        frame_map["normal_map_w"] = self.so.transform_map(frame_map["normal_map_c"], rot)
        # transform_map moves the zero vertices of invalid pixels too; they are never sampled (depth 0 / zero normal masks)
        return ok

    def _track_or_relocalise(self, frame_map):
        """`relocalise`: -> (pose, ok) and self.lost.  A frame is lost when predict_pose reports singular normal equations, a
        non-finite pose or tracking_success False; while lost ICP is not tried and every frame goes to the relocaliser, whose
        pose - the frame registered onto a keyframe - ends the lost state."""
        if not self.lost:
            try:
                rel, ok = self.icp_tracker.predict_pose(self.curr_frame)
            except RuntimeError as e:
                if "singular normal equations" not in str(e):
                    raise
                rel, ok = None, False
            if ok and not np.isfinite(rel).all():
                ok = False
            if ok:
                if self.rgbd_refiner is not None:
                    rel = self._rgbd_refine(rel, frame_map)
                return self.pose_es[-1] @ rel.astype(np.float64), True
            self.lost = True
            self.relocaliser.lost_at = int(self.curr_frame["frame_id"])
        pose = self.relocaliser.locate(self, frame_map, int(self.curr_frame["frame_id"]))
        if pose is None:
            return np.array(self.pose_es[-1], dtype=np.float64), False
        self.lost = False
        return pose, True

    def _intensity_pyramid(self, frame_map):
        """This frame's intensity pyramid, built once per frame (it is the source now and the target of the next frame)."""
        if self._intensity_t1 is None or self._intensity_t1[0] is not frame_map:
            from .rgbd_align import intensity_pyramid
            self._intensity_t1 = (frame_map, intensity_pyramid(frame_map["color_chw"], len(self.icp_tracker.icp_downscales)))
        return self._intensity_t1[1]

    def _rgbd_refine(self, rel, frame_map):
        """Between predict_pose and move_last_status, while the t0 pyramids still hold what ICP tracked against: source = this
        frame, target = the t0 pyramids with the previous frame's intensity, start = ICP's pose.  tracking_success stays ICP's."""
        if self.intensity_pyramid_t0 is None:
            return rel
        it = self.icp_tracker
        if self._K_host is None:
            self._K_host = self.curr_frame["K"].detach().cpu().numpy()        # one read per sequence: the tracker's K is fixed
        t0 = time.perf_counter()
        if self.rgbd_refiner.exposure:
            # against the previous frame every pair has its own exposure; the map's does not change between frames
            start = self.rgbd_exposure if self.rgbd_target == "model" else (1.0, 0.0)
            refined, rep = self.rgbd_refiner.refine(rel, it.vertex_pyramid_t1, it.normal_pyramid_t1, self._intensity_pyramid(frame_map),
                                                    it.vertex_pyramid_t0, it.normal_pyramid_t0, self.intensity_pyramid_t0,
                                                    self._K_host, it.icp_downscales, exposure=start)
            self.rgbd_exposure = rep["exposure"]
        else:
            refined, rep = self.rgbd_refiner.refine(rel, it.vertex_pyramid_t1, it.normal_pyramid_t1, self._intensity_pyramid(frame_map),
                                                    it.vertex_pyramid_t0, it.normal_pyramid_t0, self.intensity_pyramid_t0,
                                                    self._K_host, it.icp_downscales)
        rep["wall_s"] = time.perf_counter() - t0                  # the source pyramid, the launches, the host reads and solves
        self.rgbd_reports.append(rep)
        return refined

    @property
    def wants_render_color(self):
        """True when update_last_status uses the map's rendered colour (rgbd_refine_target: model)."""
        return self.rgbd_refiner is not None and self.rgbd_target == "model" and not self.args.use_gt_pose

    def update_last_status(self, frame, render_depth, frame_depth, render_normal, frame_normal, render_color=None):
        """render_color ([H,W,3] or [3,H,W], the map rendered at this frame's pose) is used in model mode only: the next
        frame's photometric target becomes the composite of rgbd_align.target_intensity_pyramid - the render's grey, and this
        frame's own, taken into the map's exposure, where fill_model_depth replaces the model's depth by the frame's."""
        if render_color is None or not self.wants_render_color or self._color_t1 is None:
            self.icp_tracker.update_last_status(frame, render_depth, frame_depth, render_normal, frame_normal)
            return
        from .rgbd_align import target_intensity_pyramid
        unfilled = render_depth.clone()
        self.icp_tracker.update_last_status(frame, render_depth, frame_depth, render_normal, frame_normal)
        alpha, beta = self.rgbd_exposure
        self.intensity_pyramid_t0 = target_intensity_pyramid(render_color, self._color_t1, unfilled, render_depth, alpha, beta,
                                                             len(self.icp_tracker.icp_downscales))

    def get_new_poses(self):
        """tracker.py:69-74: the trajectory as a back end (ORB-SLAM2 in the reference, out of scope here) has corrected it,
        or None without one - Mapping.update_poses(None) then leaves every frame where it is.  While the run goes on there is
        none: the loop closure (`loop_closure`, rtg_slam_amd.loop_closure) corrects the trajectory once, after the last frame."""
        return None


def ate_rmse(pose_es, pose_gt, align: bool = False) -> float:
    """RMSE of the translation error; align=True first fits the rigid transform (Horn) the reference's eval applies."""
    E = np.stack([p[:3, 3] for p in pose_es])
    G = np.stack([p[:3, 3] for p in pose_gt])
    if align and len(E) >= 3:
        me, mg = E.mean(0), G.mean(0)
        U, _, Vt = np.linalg.svd((G - mg).T @ (E - me))
        S = np.eye(3)
        if np.linalg.det(U @ Vt) < 0:
            S[2, 2] = -1
        R = U @ S @ Vt
        E = (E - me) @ R.T + mg
    return float(np.sqrt(((E - G) ** 2).sum(1).mean()))


def run_sequence(cam, stream: Iterable, args, device, mapper: Optional[Mapping] = None, lr_scale: float = 1.0,
                 capacity: Optional[int] = None, on_frame: Optional[Callable] = None, final_global: bool = False,
                 eval_every: Optional[int] = None):
    """slam.py:56-95 over `stream` = iterable of (depth [H,W] metres, colour [3,H,W] in 0..1, ground-truth c2w 4x4) on the
    device.  Returns (mapper, tracker, report): report["fps"] is the reference's definition, 1 / mean(mapping seconds per
    frame) (utils/monitor.py:22-24), next to the frame rate of the whole loop (tracking + mapping, sequential).

    eval_every (the reference's save_step, slam.py:98-110, 130-138): evaluate the map (rtg_slam_amd.evaluation.eval_frame)
    at mapper.time 0 and whenever (time + 1) % eval_every == 0, after the frame's mapping clock stops and on the full render
    get_render_output just made; with final_global, once more after the final global optimisation on the last keyframe and
    its raw colour / depth.  The rows are report["eval"].  None (default): no evaluation, the report as without it.

    args.loop_closure (absent = off): after the last frame and before the final global optimisation the loop closure runs once
    (loop_closure.LoopCloser.close): report["loop_closure"] is its report, the trajectory, the keyframes and the map are the
    corrected ones, and tracker.pose_es_before_loop_closure keeps the trajectory as it was tracked.

    args.relocalise (absent = off; rtg_slam_amd.relocalisation): a frame the ICP tracker cannot hold is LOST - it keeps the last
    good pose, is listed in tracker.lost_frames and is not mapped (mapper.time still advances, so pose_es keeps one row per
    frame) - and so is every frame after it until the relocaliser registers one onto a keyframe; that frame is mapped like any
    other.  report["relocalisation"] and report["ate_rmse_tracked_m"] (the ATE over the frames not lost) exist only then."""
    from . import evaluation
    mapper = mapper if mapper is not None else Mapping(args, device, capacity=capacity, lr_scale=lr_scale)
    tracker = Tracker(args, device)
    closer = None
    if bool(getattr(args, "loop_closure", False)):
        from .loop_closure import LoopCloser
        if mapper.opt.world != 1:
            raise RuntimeError("loop_closure runs on one rank: the map deformation is not exchanged between ranks")
        closer = LoopCloser(args)                               # a bad option stops the run before its first frame
    reloc = None
    if bool(getattr(args, "relocalise", False)):
        from .relocalisation import Relocaliser
        reloc = tracker.relocaliser = Relocaliser(args, mapper.opt.world)      # the same: before the first frame
        reloc.mapper = mapper
    t_track, t_map, per_frame = 0.0, 0.0, []
    evals, last_kf = [], None
    n = 0
    torch.cuda.synchronize(device)
    t_all = time.perf_counter()
    for frame_id, (depth, color, gt_c2w) in enumerate(stream):
        t0 = time.perf_counter()
        frame = Frame(cam, gt_c2w, device, uid=frame_id)
        frame_map = tracker.map_preprocess(frame, depth, color, frame_id)
        tracker.tracking(frame, frame_map, pose_gt=gt_c2w, init_pose=gt_c2w if frame_id == 0 else None)
        t1 = time.perf_counter()                                # predict_pose returned a host pose: the tracker is done
        if reloc is not None and tracker.lost:                  # a lost frame is not mapped; the map's clock still ticks
            t_track += t1 - t0
            per_frame.append((t1 - t0, 0.0, mapper.opt.N, mapper.opt.n_frozen))
            if on_frame is not None:
                on_frame(frame_id, frame, frame_map, mapper, tracker)
            mapper.time += 1
            n += 1
            continue
        mapper.update_poses(tracker.get_new_poses())            # slam.py:76-77
        mapper.mapping(frame, frame_map, frame_id)
        mm = mapper.get_render_output(frame)
        # update_last_status fills holes of the model depth IN PLACE (icp.py:397-415): hand it a copy, the render is cached
        if tracker.wants_render_color:                          # rgbd_refine_target: model - the render's colour is the next target
            tracker.update_last_status(frame, mm["render_depth"].clone(), frame_map["depth_map"],
                                       mm["render_normal"].contiguous(), frame_map["normal_map_w"], mm["render_color"])
        else:
            tracker.update_last_status(frame, mm["render_depth"].clone(), frame_map["depth_map"],
                                       mm["render_normal"].contiguous(), frame_map["normal_map_w"])
        if reloc is not None:
            reloc.on_keyframes(mapper)                          # a new keyframe's thumbnail: one launch
        torch.cuda.synchronize(device)                          # the mapper's frame is over when its kernels are
        t2 = time.perf_counter()
        t_track += t1 - t0
        t_map += t2 - t1
        per_frame.append((t1 - t0, t2 - t1, mapper.opt.N, mapper.opt.n_frozen))
        if eval_every:
            if mapper.keyframe_list and mapper.keyframe_list[-1] is frame:     # keymap_list keeps the preprocessed depth only
                last_kf = (frame, frame_id, depth.clone(), color.clone())
            if mapper.time == 0 or (mapper.time + 1) % int(eval_every) == 0:
                row = evaluation.eval_frame(mapper, frame, color, depth)
                row.update(frame=mapper.time, final=False)
                evals.append(row)
        if on_frame is not None:
            on_frame(frame_id, frame, frame_map, mapper, tracker)
        mapper.time += 1
        n += 1
    closure = None
    if closer is not None and n > 0:
        tracker.pose_es_before_loop_closure = [np.array(p, dtype=np.float64) for p in tracker.pose_es]
        closure = closer.close(mapper, tracker)
    if final_global and n > 0:
        mapper.global_optimization(select_keyframe_num=-1, is_end=True)
        torch.cuda.synchronize(device)
        if eval_every and last_kf is not None:
            kf, kf_id, kf_depth, kf_color = last_kf
            row = evaluation.eval_frame(mapper, kf, kf_color, kf_depth)
            row.update(frame=kf_id, final=True)
            evals.append(row)
    wall = time.perf_counter() - t_all
    es, gt = tracker.pose_es, tracker.pose_gt
    report = {
        "frames": n, "tracking_s_mean": t_track / max(n, 1), "mapping_s_mean": t_map / max(n, 1),
        "fps": (n / t_map) if t_map > 0 else None,                        # monitor.py:22-24: 1 / mean mapping time
        "fps_tracking_plus_mapping": (n / (t_track + t_map)) if n else None,
        "wall_s": wall,
        "ate_rmse_m": ate_rmse(es, gt) if n else None, "ate_rmse_aligned_m": ate_rmse(es, gt, True) if n else None,
        "final_translation_error_m": float(np.linalg.norm(es[-1][:3, 3] - gt[-1][:3, 3])) if n else None,
        "gaussians": int(mapper.opt.N), "stable": int(mapper.opt.n_frozen), "unstable": int(mapper.opt.n_train),
        "keyframes": mapper.get_keyframe_num, "stats": dict(mapper.stats),
        "stable_fraction_over_time": [round(p[3] / max(p[2], 1), 4) for p in per_frame[::max(1, n // 20)]],
        "gaussians_over_time": [p[2] for p in per_frame[::max(1, n // 20)]],
        "per_frame": per_frame,
        "stage_profile_ms_per_frame": None if mapper.prof is None else {k: round(1e3 * v / max(n, 1), 3) for k, v in mapper.prof.items()},
    }
    if eval_every:
        report["eval"] = evals
    if closure is not None:
        report["loop_closure"] = closure
    if reloc is not None:
        report["relocalisation"] = reloc.report(tracker)
        kept = [k for k in range(n) if k not in set(tracker.lost_frames)]
        report["ate_rmse_tracked_m"] = ate_rmse([es[k] for k in kept], [gt[k] for k in kept]) if kept and len(gt) == n else None
    if tracker.rgbd_refiner is not None:
        reps = tracker.rgbd_reports
        k = max(len(reps), 1)
        report["rgbd_refine"] = {
            "frames": len(reps), "iterations_mean": sum(sum(r["iterations"]) for r in reps) / k,
            "host_reads_mean": sum(r["host_reads"] for r in reps) / k,
            "photometric_inliers_mean": sum(r["inliers_photometric"][-1] for r in reps if r["inliers_photometric"]) / k,
            "device_ms_mean": 1e3 * sum(r["device_s"] for r in reps) / k,
            "ms_mean": 1e3 * sum(r["wall_s"] for r in reps) / k,
            "photo_weight": tracker.rgbd_refiner.photo_weight, "huber": tracker.rgbd_refiner.huber}
        if hasattr(args, "rgbd_refine_target"):
            report["rgbd_refine"]["target"] = tracker.rgbd_target
        if tracker.rgbd_refiner.exposure:
            al = [r["exposure"][0] for r in reps] or [1.0]
            be = [r["exposure"][1] for r in reps] or [0.0]
            report["rgbd_refine"].update(exposure=True, alpha_mean=sum(al) / len(al), beta_mean=sum(be) / len(be),
                                         alpha_min=min(al), alpha_max=max(al))
    if getattr(mapper, "map_exposure", None) is not None:
        report["map_exposure"] = mapper.map_exposure.report()             # one host read, after the sequence
    return mapper, tracker, report
