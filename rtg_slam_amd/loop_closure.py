"""Loop closure at the end of a run: keyframe pose graph, corrected trajectory, deformed map ("Loop closure").

    find_candidates     keyframe pairs far apart in time whose ESTIMATED poses lie close (host, deterministic)
    (place_recognition) keyframe pairs far apart in time that LOOK alike, whatever the poses say (loop_closure_candidates)
    (keypoints)         a relative pose for an appearance pair from the two frames alone (loop_closure_appearance_init)
    register_pair       one candidate through rgbd_align.RgbdRefiner.refine from the estimated relative pose -> an edge or a refusal
    frame_corrections   the keyframes' corrections T'_k T_k^-1 spread over all frames along SE(3) geodesics
    deform_table        those corrections as the float32 table of rtgs_map_deform (include/rtgs_slam.h)
    LoopCloser.close    candidates -> edges -> pose_graph.optimize -> trajectory, keyframes and map moved
    (sh_rotation)       with loop_closure_rotate_sh, the map's higher SH bands turned by each frame's correction as well

The option (`loop_closure: True`) is off by default and runs once, after the last frame and before the final global optimisation
(slam.run_sequence).  By default (loop_closure_candidates "pose") candidates come from the estimated poses alone, so a loop whose
drift exceeds loop_closure_max_trans is not found.  "appearance" takes them from the keyframes' thumbnails instead
(place_recognition.py: ZNCC of grey thumbnails over a horizontal shift, depth thumbnails as a second witness) and starts each
registration from the shift's yaw alone, so neither trusts the trajectory; "both" registers the pose candidates first and then
the appearance pairs not among them, each source with its own loop_closure_max_per_keyframe.  register_pair and its gates are
the same for both: max_correction_* then bounds the correction measured from the appearance guess, so a revisit must lie
within 0.2 m and about 5 degrees plus the shift's yaw of the earlier view.  Two places that look and measure alike pass both
witnesses; only those gates and loop_closure_huber stand against such an edge.  The defaults below are derived from the ICP's
gates (icp_distance_threshold 0.1 m, icp_normal_threshold 20 degrees) and the drift the README quotes (5 cm over 2 000 frames),
the appearance thresholds chosen on the synthetic box room; none has been measured on real data.

loop_closure_appearance_init "keypoints" lifts that last limit: every appearance candidate's first guess becomes the relative pose
keypoints.py computes from the two frames alone (corners, binary descriptors, a 3-D - 3-D RANSAC over their depth) when it has
loop_closure_keypoint_min_inliers geometric witnesses, and the yaw guess otherwise; "keypoints_strict" refuses the candidate
instead of falling back.  register_pair and its gates stay what they are - the correction gate then measures what it was meant
to: how far the dense registration moved a guess that was already a measurement.

Thumbnails and single-scale keypoints both miss a revisit seen from another distance (the thumbnails' depth witness refuses a
view more than about 10 % further away by construction).  loop_closure_keypoint_levels takes the keypoints from an image pyramid
instead, and loop_closure_candidates "keypoints" finds the revisits by those keypoints alone (LoopCloser._keypoint_search): the
count of filtered matches ranks the older keyframes, the device RANSAC judges the best few, register_pair and its gates stay
what they are.  Every pair of keyframes is matched, so the search costs O(keyframes^2) match work; there is no vocabulary."""
from __future__ import annotations

import time
from types import SimpleNamespace
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import keypoints as kp
from . import pose_graph
from .rgbd_align import se3_exp, se3_log

DEFAULTS = {
    "loop_closure_min_gap": 10,                    # keyframes between the two ends of a loop edge
    "loop_closure_max_trans": 0.5,                 # metres between the estimated positions: ten times the quoted drift
    "loop_closure_max_rot_deg": 30.0,              # the views must overlap: half a 60-degree field of view
    "loop_closure_max_per_keyframe": 2,
    "loop_closure_min_inlier_ratio": 0.3,          # geometric inliers / valid source pixels at the last level evaluated
    "loop_closure_max_rms": 0.02,                  # metres, point to plane: a fifth of the ICP's distance gate
    "loop_closure_max_correction_trans": 0.2,      # metres a registration may move the estimate: four times the quoted drift
    "loop_closure_max_correction_rot_deg": 5.0,
    "loop_closure_odometry_weights": (1.0, 1.0),   # (per rad^2, per m^2)
    "loop_closure_loop_weights": (1.0, 1.0),
    "loop_closure_huber": None,                    # weighted residual norm beyond which a loop edge pulls linearly; None = off
    # where the candidates come from: "pose" (find_candidates), "appearance" (place_recognition) or "both".  The four values
    # below are read only when it is not "pose"; 40 / 0.9 / 0.1 were chosen on the synthetic box room, not measured on real data
    "loop_closure_candidates": "pose",
    "loop_closure_thumb_width": 40,                # thumbnail columns; the rows follow the image's aspect
    "loop_closure_max_shift": 4,                   # columns searched to either side: 4 of 40 at a 90-degree view are about 11 degrees
    "loop_closure_min_score": 0.9,                 # ZNCC of the grey thumbnails at the best shift
    "loop_closure_max_depth_rel": 0.1,             # mean |depth difference| over the mean depth of the two thumbnails
    # the first guess of an appearance candidate: "yaw" (place_recognition.appearance_init), "keypoints" (keypoints.relative_pose
    # where it has min_inliers witnesses, the yaw guess otherwise) or "keypoints_strict" (no fallback: the candidate is refused)
    "loop_closure_appearance_init": "yaw",
    **{"loop_closure_keypoint_" + k: v for k, v in kp.DEFAULTS.items()},
}
CANDIDATE_SOURCES = ("pose", "appearance", "both", "keypoints")
APPEARANCE_INITS = ("yaw", "keypoints", "keypoints_strict")
# loop_closure_keypoint_levels (1 .. 5, absent = 1): the levels of the image pyramid the keypoints are taken from (keypoints.py).
# loop_closure_candidates "keypoints": the revisits are found by the keyframes' keypoints alone - every pair min_gap apart is
# matched and its filtered matches counted on the device (the votes), the loop_closure_keypoint_shortlist older keyframes with
# the most votes per keyframe go through the device RANSAC, and those with min_inliers witnesses become candidates that start
# from the RANSAC pose.  It implies appearance_init keypoints_strict and keypoint_ransac device.  Both keys are kept out of
# DEFAULTS: absent, no report and no launch knows of them
KEYPOINT_SHORTLIST = 3
# the match tables of one chunk of the keypoint search (12 bytes a row, both directions of every pair) stay below this
KEYPOINT_SEARCH_TABLE_BYTES = 64 << 20
# loop_closure_keypoint_ransac: where the match filter and the RANSAC of the keypoint pose run.  "host" (the default, also when
# the key is absent) is keypoints.pose_from_matches per candidate; "device" is one rtgs_rigid_ransac launch for all candidates
# (keypoints.rigid_ransac_pairs).  Kept out of DEFAULTS: absent or "host", no report and no launch knows of it
KEYPOINT_RANSACS = ("host", "device")
# loop_closure_rotate_sh (a bool, absent = False): the higher SH bands of the deformed map turn with each frame's correction
# (sh_rotation.sh_rotation_table, rtgs_map_deform_sh).  Kept out of DEFAULTS: absent or False, no report and no launch knows of it
# register_pair's figures, None in a candidate that keypoints_strict refused without registering it
REGISTER_FIGURES = ("refine_reason", "iterations", "rank_min", "rms_geometric_before", "rms_geometric_after", "device_s", "inliers",
                    "valid_source_pixels", "inlier_ratio", "correction_trans", "correction_rot_deg")


def _angle_deg(R) -> float:
    return float(np.rad2deg(np.arccos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0)))))


def find_candidates(poses, frame_ids: Sequence[int], min_gap: int, max_trans: float, max_rot_deg: float,
                    max_per_keyframe: int) -> List[Tuple[int, int, float, float]]:
    """For keyframe b (index into `poses`, c2w 4x4 each) the keyframes a with b - a >= min_gap whose pose lies within max_trans
    metres and max_rot_deg degrees of b's, nearest first (ties: the smaller angle, then the older keyframe), at most
    max_per_keyframe of them.  -> [(a, b, metres, degrees)] in ascending b.  `frame_ids` (one per keyframe, ascending) only
    has to match `poses` in length: the gap is counted in keyframes."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if len(frame_ids) != P.shape[0]:
        raise ValueError("find_candidates: one frame id per keyframe pose")
    if int(min_gap) < 1 or int(max_per_keyframe) < 1 or not (max_trans >= 0 and max_rot_deg >= 0):
        raise ValueError("find_candidates: min_gap and max_per_keyframe must be >= 1, the bounds not negative")
    out = []
    for b in range(P.shape[0]):
        near = []
        for a in range(0, b - int(min_gap) + 1):
            d = float(np.linalg.norm(P[a, :3, 3] - P[b, :3, 3]))
            ang = _angle_deg(P[a, :3, :3].T @ P[b, :3, :3])
            if d <= max_trans and ang <= max_rot_deg:
                near.append((d, ang, a))
        near.sort()
        out.extend((a, b, d, ang) for d, ang, a in near[:int(max_per_keyframe)])
    return out


def frame_corrections(keyframe_ids: Sequence[int], poses_old, poses_new, n_frames: int) -> np.ndarray:
    """[n_frames, 4, 4] float64.  D_k = T'_k T_k^-1 at keyframe k; for f_a <= f < f_b between neighbouring keyframes the SE(3)
    geodesic D_a exp(s log(D_a^-1 D_b)), s = (f - f_a) / (f_b - f_a); D of the last keyframe for every later frame.  Frame 0
    is always a keyframe.  A keyframe whose pose did not change gets the identity exactly."""
    ids = [int(i) for i in keyframe_ids]
    old = np.asarray(poses_old, dtype=np.float64).reshape(-1, 4, 4)
    new = np.asarray(poses_new, dtype=np.float64).reshape(-1, 4, 4)
    if not ids or ids[0] != 0 or any(b <= a for a, b in zip(ids, ids[1:])) or len(ids) != len(old) or len(old) != len(new):
        raise ValueError("frame_corrections: keyframe ids must ascend from 0, one old and one new pose each")
    if int(n_frames) <= ids[-1]:
        raise ValueError("frame_corrections: a keyframe lies beyond the trajectory")
    D = [np.eye(4) if np.array_equal(n, o) else n @ pose_graph.inverse(o) for o, n in zip(old, new)]
    out = np.empty((int(n_frames), 4, 4), dtype=np.float64)
    for k, fa in enumerate(ids):
        last = k + 1 == len(ids)
        fb = int(n_frames) if last else ids[k + 1]
        out[fa] = D[k]
        if fb - fa > 1:
            if last or np.array_equal(D[k], D[k + 1]):
                out[fa + 1:fb] = D[k]
            else:
                x = se3_log(pose_graph.inverse(D[k]) @ D[k + 1])
                for f in range(fa + 1, fb):
                    out[f] = D[k] @ se3_exp(x * ((f - fa) / (fb - fa)))
    return out


def rotmat_to_quat(R) -> np.ndarray:
    """Unit quaternion (w, x, y, z), w >= 0, of a rotation matrix, float64 (Shepperd's choice of the largest pivot)."""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2.0
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2.0
        q = np.empty(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = q / np.sqrt(np.dot(q, q))
    return -q if q[0] < 0 else q


def deform_table(corrections) -> np.ndarray:
    """[n, 4, 4] float64 -> the table of rtgs_map_deform, float32 [n, 16]: the 3 x 4 matrix row by row, then the rotation's unit
    quaternion; computed in float64 and rounded once.  An identity correction gives the identity row exactly."""
    D = np.asarray(corrections, dtype=np.float64).reshape(-1, 4, 4)
    out = np.empty((D.shape[0], 16), dtype=np.float64)
    out[:, :12] = D[:, :3, :].reshape(-1, 12)
    for f in range(D.shape[0]):
        out[f, 12:] = (1.0, 0.0, 0.0, 0.0) if np.array_equal(D[f, :3, :3], np.eye(3)) else rotmat_to_quat(D[f, :3, :3])
    return out.astype(np.float32)


def register_pair(refiner, src: Dict, tgt: Dict, init_pose, K, downscales, cfg) -> Dict:
    """One candidate: source keyframe b onto target keyframe a from init_pose = T_a^-1 T_b (source -> target camera).  `src` /
    `tgt`: {"vertex", "normal", "intensity"} pyramids, coarsest first (LoopCloser._pyramids).  -> {"accepted", "reason", "Z"
    (4x4 float64, the measured T_a^-1 T_b), the gates' figures}.  The edge is accepted only if the loop ended with reason "done",
    every solve had full rank (6, or 8 with the exposure unknowns), the geometric inliers of the last evaluation are at least
    min_inlier_ratio of the valid (z > 0) source pixels of its level, rms_geometric_after <= max_rms, and the correction
    init_pose^-1 Z stays within max_correction_trans / max_correction_rot_deg."""
    init = np.asarray(init_pose, dtype=np.float64).reshape(4, 4)
    Z, rep = refiner.refine(init, src["vertex"], src["normal"], src["intensity"], tgt["vertex"], tgt["normal"], tgt["intensity"],
                            K, downscales)
    full = 8 if refiner.exposure else 6
    levels = [l for l, n in enumerate(rep["iterations"]) if n > 0]
    out = {"accepted": False, "reason": None, "Z": Z, "refine_reason": rep["reason"], "iterations": list(rep["iterations"]),
           "rank_min": min(rep["rank"]) if rep["rank"] else 0, "rms_geometric_before": rep["rms_geometric_before"],
           "rms_geometric_after": rep["rms_geometric_after"], "device_s": rep["device_s"]}
    inliers = rep["inliers_geometric"][-1] if rep["inliers_geometric"] else 0
    if levels:
        valid = int((src["vertex"][levels[-1]][..., 2] > 0).sum().item())
    else:
        valid = 0
    out["inliers"], out["valid_source_pixels"] = int(inliers), valid
    out["inlier_ratio"] = inliers / valid if valid else 0.0
    C = pose_graph.inverse(init) @ Z
    out["correction_trans"] = float(np.linalg.norm(C[:3, 3]))
    out["correction_rot_deg"] = _angle_deg(C[:3, :3])
    if rep["reason"] != "done":
        out["reason"] = "refinement stopped: " + rep["reason"]
    elif not rep["rank"] or min(rep["rank"]) < full:
        out["reason"] = f"a solve had rank {out['rank_min']} of {full}"
    elif out["inlier_ratio"] < cfg.min_inlier_ratio:
        out["reason"] = f"inlier ratio {out['inlier_ratio']:.3f} below {cfg.min_inlier_ratio:g}"
    elif not rep["rms_geometric_after"] <= cfg.max_rms:
        out["reason"] = f"geometric rms {rep['rms_geometric_after']:.4f} m above {cfg.max_rms:g}"
    elif out["correction_trans"] > cfg.max_correction_trans or out["correction_rot_deg"] > cfg.max_correction_rot_deg:
        out["reason"] = (f"correction {out['correction_trans']:.3f} m / {out['correction_rot_deg']:.2f} degrees beyond "
                         f"{cfg.max_correction_trans:g} m / {cfg.max_correction_rot_deg:g} degrees")
    else:
        out["accepted"], out["reason"] = True, "accepted"
    return out


def _pair(value, name):
    try:
        a, b = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two numbers: (rotation weight, translation weight)") from None
    if not (a >= 0 and b >= 0 and a + b > 0):
        raise ValueError(f"{name} must not be negative, and not both zero")
    return a, b


class LoopCloser:
    """Reads the loop_closure_* keys of `args` with getattr and DEFAULTS, and of the run rgbd_refine_exposure / map_exposure
    (either selects the eight-unknown registration), icp_downscales and the RGB-D refiner's own keys.  `close` is meant for
    the end of a run: the tracker's ICP state and the mapper's window of recent frame maps are not corrected."""

    def __init__(self, args):
        get = lambda k: getattr(args, k, DEFAULTS[k])
        self.args = args
        self.cfg = cfg = SimpleNamespace(
            min_gap=int(get("loop_closure_min_gap")), max_trans=float(get("loop_closure_max_trans")),
            max_rot_deg=float(get("loop_closure_max_rot_deg")), max_per_keyframe=int(get("loop_closure_max_per_keyframe")),
            min_inlier_ratio=float(get("loop_closure_min_inlier_ratio")), max_rms=float(get("loop_closure_max_rms")),
            max_correction_trans=float(get("loop_closure_max_correction_trans")),
            max_correction_rot_deg=float(get("loop_closure_max_correction_rot_deg")),
            odometry_weights=_pair(get("loop_closure_odometry_weights"), "loop_closure_odometry_weights"),
            loop_weights=_pair(get("loop_closure_loop_weights"), "loop_closure_loop_weights"),
            huber=None if get("loop_closure_huber") is None else float(get("loop_closure_huber")))
        if cfg.min_gap < 1 or cfg.max_per_keyframe < 1:
            raise ValueError("loop_closure_min_gap and loop_closure_max_per_keyframe must be >= 1")
        for k in ("max_trans", "max_rot_deg", "max_rms", "max_correction_trans", "max_correction_rot_deg"):
            if not getattr(cfg, k) >= 0:
                raise ValueError(f"loop_closure_{k} must not be negative")
        if not 0 <= cfg.min_inlier_ratio <= 1:
            raise ValueError("loop_closure_min_inlier_ratio must lie in [0, 1]")
        if cfg.huber is not None and not cfg.huber > 0:
            raise ValueError("loop_closure_huber must be positive")
        # kept apart from cfg: the report's "options" are cfg's, key for key what they were before there was a choice
        self.place = pl = SimpleNamespace(
            candidates=str(get("loop_closure_candidates")), thumb_width=int(get("loop_closure_thumb_width")),
            max_shift=int(get("loop_closure_max_shift")), min_score=float(get("loop_closure_min_score")),
            max_depth_rel=float(get("loop_closure_max_depth_rel")))
        if pl.candidates not in CANDIDATE_SOURCES:
            raise ValueError(f"loop_closure_candidates must be one of {', '.join(CANDIDATE_SOURCES)}")
        if pl.thumb_width < 1:
            raise ValueError("loop_closure_thumb_width must be >= 1")
        if pl.max_shift < 0 or 2 * pl.max_shift >= pl.thumb_width:
            raise ValueError("loop_closure_max_shift must not be negative and twice it must stay below loop_closure_thumb_width")
        if not -1 <= pl.min_score <= 1:
            raise ValueError("loop_closure_min_score must lie in [-1, 1]")
        if not pl.max_depth_rel >= 0:
            raise ValueError("loop_closure_max_depth_rel must not be negative")
        # kept apart as well: absent or "yaw", nothing of it reaches a report
        levels = {"levels": args.loop_closure_keypoint_levels} if hasattr(args, "loop_closure_keypoint_levels") else {}
        self.keypoints = SimpleNamespace(init=str(get("loop_closure_appearance_init")),
                                         cfg=kp.config(**{k: get("loop_closure_keypoint_" + k) for k in kp.DEFAULTS}, **levels))
        if self.keypoints.init not in APPEARANCE_INITS:
            raise ValueError(f"loop_closure_appearance_init must be one of {', '.join(APPEARANCE_INITS)}")
        self.keypoints.ransac = str(getattr(args, "loop_closure_keypoint_ransac", "host"))
        if self.keypoints.ransac not in KEYPOINT_RANSACS:
            raise ValueError(f"loop_closure_keypoint_ransac must be one of {', '.join(KEYPOINT_RANSACS)}")
        if pl.candidates == "keypoints":
            if hasattr(args, "loop_closure_appearance_init") and self.keypoints.init != "keypoints_strict":
                raise ValueError("loop_closure_candidates keypoints starts every candidate from its keypoint pose: "
                                 "loop_closure_appearance_init can only be keypoints_strict with it")
            if hasattr(args, "loop_closure_keypoint_ransac") and self.keypoints.ransac != "device":
                raise ValueError("loop_closure_candidates keypoints runs the RANSAC on the device: loop_closure_keypoint_ransac "
                                 "can only be device with it")
            self.keypoints.init, self.keypoints.ransac = "keypoints_strict", "device"
            self.keypoints.shortlist = int(getattr(args, "loop_closure_keypoint_shortlist", KEYPOINT_SHORTLIST))
            if self.keypoints.shortlist < 1:
                raise ValueError("loop_closure_keypoint_shortlist must be >= 1")
        elif hasattr(args, "loop_closure_keypoint_shortlist"):
            raise ValueError("loop_closure_keypoint_shortlist applies to the keypoint search: it needs loop_closure_candidates keypoints")
        if self.keypoints.ransac == "device" and self.keypoints.init == "yaw":
            raise ValueError("loop_closure_keypoint_ransac applies to the keypoint pose: it needs loop_closure_appearance_init "
                             "keypoints or keypoints_strict")
        if self.keypoints.ransac == "device" and self.keypoints.cfg.ransac_iters > kp.RANSAC_MAX_ITERS:
            raise ValueError(f"loop_closure_keypoint_ransac device: loop_closure_keypoint_ransac_iters must not exceed {kp.RANSAC_MAX_ITERS}")
        if self.keypoints.init != "yaw" and pl.candidates == "pose":
            raise ValueError("loop_closure_appearance_init applies to appearance candidates: it needs loop_closure_candidates "
                             "appearance or both")
        self.rotate_sh = getattr(args, "loop_closure_rotate_sh", False)
        if not isinstance(self.rotate_sh, bool):
            raise ValueError("loop_closure_rotate_sh must be true or false")
        from .rgbd_align import RgbdRefiner
        exposure = bool(getattr(args, "rgbd_refine_exposure", False)) or bool(getattr(args, "map_exposure", False))
        ref_args = SimpleNamespace(**{k: v for k, v in vars(args).items() if k.startswith(("rgbd_refine_", "icp_"))})
        ref_args.rgbd_refine_exposure = exposure
        self.refiner = RgbdRefiner(ref_args)
        self.downscales = list(getattr(args, "icp_downscales", (0.25, 0.5, 1.0)))

    def _pyramids(self, keymap, K, cache, key):
        from . import icp
        from .rgbd_align import intensity_pyramid
        hit = cache.get(key)
        if hit is None:
            depth = keymap["depth_chw"]
            v, n = icp.build_pyramids(depth.reshape(depth.shape[-2], depth.shape[-1]), K, len(self.downscales))
            hit = {"vertex": v, "normal": n, "intensity": intensity_pyramid(keymap["color_chw"], len(self.downscales))}
            if len(cache) >= 4:                                                # a keyframe's pyramids are 4/3 of 28 B a pixel
                cache.pop(next(iter(cache)))
            cache[key] = hit
        return hit

    def _appearance_candidates(self, mapper, old, taken, rep) -> List[Tuple]:
        """The pairs of place_recognition that are not in `taken`, as (a, b, metres, degrees between the ESTIMATED poses, {"init",
        "score", "shift", "depth_rel"}); init is appearance_init, which does not look at the poses.  Fills rep["appearance"]."""
        from . import place_recognition as pr
        cfg, pl, dev = self.cfg, self.place, mapper.device
        t0 = time.perf_counter()
        desc = pr.describe_all(mapper.keymap_list, pl.thumb_width)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        score, shift, rel = pr.score_pairs(desc, cfg.min_gap, pl.max_shift)
        found = pr.find_appearance_candidates(score, shift, rel, cfg.min_gap, pl.min_score, pl.max_depth_rel, cfg.max_per_keyframe)
        t2 = time.perf_counter()
        M, th, tw = (int(x) for x in desc["intensity"].shape)
        W, fx = int(mapper.keymap_list[0]["color_chw"].shape[-1]), float(mapper.keyframe_list[0].fx)
        out = []
        for a, b, sc, sh, dr in found:
            if (a, b) in taken:
                continue
            rel_pose = pose_graph.inverse(old[a]) @ old[b]
            out.append((a, b, float(np.linalg.norm(old[a][:3, 3] - old[b][:3, 3])), _angle_deg(rel_pose[:3, :3]),
                        {"init": pr.appearance_init(sh, fx, W, tw), "score": sc, "shift": sh, "depth_rel": dr}))
        rep["appearance"] = {"mode": pl.candidates, "thumbnail": [tw, th], "max_shift": pl.max_shift, "min_score": pl.min_score,
                             "max_depth_rel": pl.max_depth_rel,
                             "pairs_scored": sum(max(0, b - cfg.min_gap + 1) for b in range(M)),
                             "candidates": len(found), "candidates_new": len(out)}
        rep["seconds"].update(describe=t1 - t0, scores=t2 - t1)
        if self.keypoints.init != "yaw":
            self._keypoint_inits(mapper, out, rep)
        return out

    def _keypoint_inits(self, mapper, cands, rep):
        """loop_closure_appearance_init "keypoints" / "keypoints_strict": the features of every keyframe in an appearance
        candidate (once each, kept until this returns), ONE match launch for all pairs in both directions, the RANSAC per pair
        on the host - or, with loop_closure_keypoint_ransac "device", one rtgs_rigid_ransac launch for all pairs behind the
        match launch, the match tables staying on the device.  Each candidate's dict gains "init_source", "keypoints" and - under keypoints_strict below min_inliers -
        "refused"; its "init" becomes the keypoint pose where that has its witnesses."""
        kc, dev = self.keypoints.cfg, mapper.device
        K = mapper.keyframe_list[0].K
        t0 = time.perf_counter()
        feats = {}
        for a, b, *_ in cands:
            for k in (a, b):
                if k not in feats:
                    km = mapper.keymap_list[k]
                    feats[k] = kp.detect_and_describe(km["color_chw"], km["depth_chw"], K, kc)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        on_device = self.keypoints.ransac == "device"
        if on_device:
            fits = kp.rigid_ransac_pairs(feats, [(a, b) for a, b, *_ in cands], kc)      # t2 - t1 below is both launches and the copy
        else:
            tables = kp.match_pairs(feats, [pair for a, b, *_ in cands for pair in ((b, a), (a, b))])
        t2 = time.perf_counter()
        used = 0
        for n, (a, b, _, _, seen) in enumerate(cands):
            r = fits[n] if on_device else kp.pose_from_matches(feats[a], feats[b], tables[2 * n], tables[2 * n + 1], kc)
            seen["keypoints"] = {"a": r["keypoints_a"], "b": r["keypoints_b"], "matches": r["matches"], "inliers": r["inliers"],
                                 "rms_m": r["rms"]}
            if r["T"] is not None:
                seen["init"], seen["init_source"] = r["T"], "keypoints"
                used += 1
            else:
                seen["init_source"] = "yaw"
                if self.keypoints.init == "keypoints_strict":
                    seen["refused"] = "keypoints: " + r["reason"]
        rep["appearance"].update(init=self.keypoints.init, keypoint_inits=used,
                                 **{"keypoint_" + k: v for k, v in vars(kc).items()})
        if on_device:
            rep["appearance"]["keypoint_ransac"] = "device"
        rep["seconds"].update(keypoints_describe=t1 - t0, keypoints_match=t2 - t1, keypoints_ransac=time.perf_counter() - t2)

    def _keypoint_search(self, mapper, old, rep) -> List[Tuple]:
        """loop_closure_candidates "keypoints": the revisits found by the keyframes' keypoints alone, as (a, b, metres, degrees
        between the ESTIMATED poses, {"init", "init_source", "votes", "keypoints"}).
          1. the features of every keyframe (three launches each above one level, two at one)
          2. every pair a <= b - min_gap matched in both directions and voted on, in chunks of whole rows of b: a chunk holds at
             most keypoints.MAX_VOTE_PAIRS pairs and KEYPOINT_SEARCH_TABLE_BYTES of match tables; one match launch and one vote
             launch a chunk, only the votes read
          3. per keyframe b the `shortlist` older keyframes of the most votes, at least min_inliers of them (a pair with fewer
             filtered matches cannot have min_inliers inliers) and ties to the older keyframe, all in ONE rigid_ransac_pairs
          4. per b the max_per_keyframe of the most inliers that reach min_inliers, ties to the older keyframe
        Fills rep["keypoint_search"]."""
        cfg, kc, dev = self.cfg, self.keypoints.cfg, mapper.device
        K = mapper.keyframe_list[0].K
        M = len(mapper.keymap_list)
        clock = lambda: (torch.cuda.synchronize(dev), time.perf_counter())[1]
        t0 = clock()
        feats = [kp.detect_and_describe(km["color_chw"], km["depth_chw"], K, kc) for km in mapper.keymap_list]
        t1 = clock()
        counts = [int(f["desc"].shape[0]) for f in feats]
        votes = {}                                                       # b -> int32 [b - min_gap + 1]
        chunk, rows, chunks, voted = [], 0, 0, 0

        def flush():
            nonlocal chunk, rows, chunks, voted
            if chunk:
                got = kp.vote_pairs(feats, chunk, kc)
                at = 0
                for b in sorted({b for _, b in chunk}):
                    n = b - cfg.min_gap + 1
                    votes[b] = got[at:at + n]
                    at += n
                chunks, voted = chunks + 1, voted + len(chunk)
            chunk, rows = [], 0

        for b in range(cfg.min_gap, M):
            n = b - cfg.min_gap + 1
            if n > kp.MAX_VOTE_PAIRS:
                raise RuntimeError(f"loop_closure_candidates keypoints: more than {kp.MAX_VOTE_PAIRS + cfg.min_gap - 1} keyframes")
            need = n * counts[b] + sum(counts[:n])                       # rows of the two tables of b's pairs
            if chunk and (len(chunk) + n > kp.MAX_VOTE_PAIRS or 12 * (rows + need) > KEYPOINT_SEARCH_TABLE_BYTES):
                flush()
            chunk += [(a, b) for a in range(n)]
            rows += need
        flush()
        t2 = clock()
        short = [(a, b) for b in sorted(votes) for a in kp.shortlist(votes[b], self.keypoints.shortlist, kc.min_inliers)]
        fits = []
        for at in range(0, len(short), kp.MAX_VOTE_PAIRS):               # one launch unless there are more than 32 767 pairs
            fits += kp.rigid_ransac_pairs(feats, short[at:at + kp.MAX_VOTE_PAIRS], kc)
        t3 = clock()
        out = []
        for b in sorted(votes):
            mine = sorted((-fit["inliers"], a, fit) for (a, bb), fit in zip(short, fits) if bb == b and fit["T"] is not None)
            for _, a, fit in mine[:cfg.max_per_keyframe]:
                rel_pose = pose_graph.inverse(old[a]) @ old[b]
                out.append((a, b, float(np.linalg.norm(old[a][:3, 3] - old[b][:3, 3])), _angle_deg(rel_pose[:3, :3]),
                            {"init": fit["T"], "init_source": "keypoints", "source": "keypoints", "votes": int(votes[b][a]),
                             "keypoints": {"a": fit["keypoints_a"], "b": fit["keypoints_b"], "matches": fit["matches"],
                                           "inliers": fit["inliers"], "rms_m": fit["rms"]}}))
        rep["keypoint_search"] = {"pairs_voted": voted, "shortlisted": len(short), "candidates": len(out), "levels": int(getattr(kc, "levels", 1)),
                                  "levels_used": max((int(f.get("levels_used", 1)) for f in feats), default=1), "chunks": chunks,
                                  "shortlist": self.keypoints.shortlist, **{"keypoint_" + k: v for k, v in vars(kc).items()},
                                  "seconds": {"features": t1 - t0, "votes": t2 - t1, "ransac": t3 - t2}}
        return out

    def close(self, mapper, tracker) -> Dict:
        """-> the report (JSON-able).  Without an accepted edge nothing is changed: poses, keyframes and map stay bit-identical."""
        from . import slam_ops
        from .slam import ate_rmse
        cfg, dev = self.cfg, mapper.device
        if mapper.opt.world != 1:
            raise RuntimeError("loop closure runs on one rank")
        n = len(tracker.pose_es)
        ids = [int(i) for i in mapper.keyframe_ids]
        t0 = time.perf_counter()
        rep = {"keyframes": len(ids), "frames": n, "options": {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(cfg).items()},
               "exposure_unknowns": bool(self.refiner.exposure), "candidates": [], "edges": 0, "changed": False, "seconds": {}}
        if not ids or n == 0:
            return rep
        if ids[0] != 0 or ids[-1] >= n or int(mapper.time) != n:
            raise RuntimeError("loop closure: the keyframes, the trajectory and the map's ticks do not belong to one run")
        gt = tracker.pose_gt if len(tracker.pose_gt) == n else None
        old = [np.array(tracker.pose_es[i], dtype=np.float64) for i in ids]
        mode = self.place.candidates
        cands = [] if mode in ("appearance", "keypoints") else [
            (a, b, dist, ang, None) for a, b, dist, ang in
            find_candidates(old, ids, cfg.min_gap, cfg.max_trans, cfg.max_rot_deg, cfg.max_per_keyframe)]
        if mode == "keypoints":
            cands += self._keypoint_search(mapper, old, rep)
        elif mode != "pose":
            cands += self._appearance_candidates(mapper, old, {(a, b) for a, b, *_ in cands}, rep)
        t1 = time.perf_counter()
        K = mapper.keyframe_list[0].K
        cache, loop_edges = {}, []
        for a, b, dist, ang, seen in cands:
            init = pose_graph.inverse(old[a]) @ old[b] if seen is None else seen.pop("init")
            refused = None if seen is None else seen.pop("refused", None)
            if refused is not None:                                           # keypoints_strict: not registered at all
                r = {"accepted": False, "reason": refused, "Z": None, **{k: None for k in REGISTER_FIGURES}}
            else:
                r = register_pair(self.refiner, self._pyramids(mapper.keymap_list[b], K, cache, b),
                                  self._pyramids(mapper.keymap_list[a], K, cache, a), init, K, self.downscales, cfg)
            Z = r.pop("Z")
            r.update(a=a, b=b, frame_a=ids[a], frame_b=ids[b], distance_m=dist, angle_deg=ang)
            if mode != "pose":
                r["source"] = "pose" if seen is None else seen.pop("source", "appearance")
                r.update(seen or {})
                r["Z"] = None if Z is None else np.asarray(Z).tolist()        # the measured T_a^-1 T_b, whatever became of it
                if seen is not None and self.keypoints.init != "yaw":
                    r["init"] = np.asarray(init).tolist()
            rep["candidates"].append(r)
            if r["accepted"]:
                loop_edges.append((a, b, Z, cfg.loop_weights[0], cfg.loop_weights[1], True))
        del cache
        t2 = time.perf_counter()
        rep["edges"] = len(loop_edges)
        rep["seconds"].update(candidates=t1 - t0, registration=t2 - t1)
        if gt is not None:
            rep["ate_rmse_m_before"] = rep["ate_rmse_m"] = ate_rmse(tracker.pose_es, gt)
            rep["ate_rmse_aligned_m_before"] = rep["ate_rmse_aligned_m"] = ate_rmse(tracker.pose_es, gt, True)
        if not loop_edges:
            rep["seconds"]["total"] = time.perf_counter() - t0
            return rep
        edges = [(k - 1, k, pose_graph.inverse(old[k - 1]) @ old[k], cfg.odometry_weights[0], cfg.odometry_weights[1])
                 for k in range(1, len(ids))] + loop_edges
        new, graph = pose_graph.optimize(old, edges, fixed=0, huber=cfg.huber)
        t3 = time.perf_counter()
        D = frame_corrections(ids, old, new, n)
        moved = np.linalg.norm(D[:, :3, 3] + np.einsum("fij,fj->fi", D[:, :3, :3] - np.eye(3),
                                                       np.stack([p[:3, 3] for p in tracker.pose_es])), axis=1)
        rep["graph"] = graph
        rep["correction_max_m"], rep["correction_mean_m"] = float(moved.max()), float(moved.mean())
        rep["correction_max_deg"] = max(_angle_deg(d[:3, :3]) for d in D)
        poses = [D[f] @ np.asarray(tracker.pose_es[f], dtype=np.float64) for f in range(n)]
        tracker.pose_es[:] = poses
        mapper.update_poses(poses)
        for k, km in enumerate(mapper.keymap_list):
            if "normal_map_w" in km and not np.array_equal(D[ids[k]][:3, :3], np.eye(3)):
                rot = np.eye(4, dtype=np.float32)
                rot[:3, :3] = D[ids[k]][:3, :3]
                km["normal_map_w"] = slam_ops.transform_map(km["normal_map_w"], torch.from_numpy(rot))
        table = torch.from_numpy(deform_table(D)).to(dev)
        if self.rotate_sh:
            from .sh_rotation import sh_rotation_table
            ts = time.perf_counter()
            sh_table = torch.from_numpy(sh_rotation_table(D)).to(dev)
            rep["seconds"]["sh_table"] = time.perf_counter() - ts
            rep["sh_rotated"] = True
            mapper.opt.deform_rows(table, sh_table=sh_table)
        else:
            mapper.opt.deform_rows(table)
        torch.cuda.synchronize(dev)
        t4 = time.perf_counter()
        rep["changed"] = True
        if gt is not None:
            rep["ate_rmse_m"], rep["ate_rmse_aligned_m"] = ate_rmse(poses, gt), ate_rmse(poses, gt, True)
        rep["seconds"].update(graph=t3 - t2, apply=t4 - t3, total=t4 - t0)
        return rep
