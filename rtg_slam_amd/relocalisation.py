"""Relocalisation after tracking loss: a lost state for the SLAM loop and a keyframe search that ends it.

    Relocaliser.on_keyframes   every new keyframe's thumbnail into a growing device buffer (rtgs_place_describe)
    Relocaliser.locate         a lost frame -> its pose, or None and a counted reason

`relocalise: True` (slam --relocalise) is off by default and changes nothing when off.  A frame is LOST when the ICP tracker
reports singular normal equations, a non-finite pose or tracking_success False (slam.Tracker.tracking).  A lost frame, and every
frame after it until one is recovered, keeps the last good pose, is recorded in tracker.lost_frames and is not mapped; ICP is not
tried while lost.  Each such frame goes through `locate`:

    1. its thumbnail into the row behind the keyframes', one rtgs_place_scores launch for that row, the row read on the host
    2. the up to relocalise_candidates keyframes of the highest score that pass relocalise_min_score and relocalise_max_depth_rel
    3. its keypoints and the candidates' (a keyframe's are computed once and kept), ONE match launch for all candidates in both
       directions, ONE rtgs_rigid_ransac launch behind it, one host read (keypoints.rigid_ransac_pairs)
    4. the candidate with the most inliers, at least relocalise_min_inliers, gives the first guess - there is no yaw fallback: a
       wrong recovery corrupts the map, so the geometric witnesses are required
    5. loop_closure.register_pair registers the frame onto that keyframe under its unchanged gates
    6. accepted: the pose is T_keyframe Z with the keyframe's current pose, and the frame is tracked and mapped like any other

The keys, read with getattr, default to the run's loop_closure_* values and those to loop_closure.DEFAULTS: relocalise_candidates
(3), relocalise_min_score, relocalise_max_depth_rel, relocalise_thumb_width, relocalise_max_shift, relocalise_min_inliers, and the
registration's gates relocalise_min_inlier_ratio, relocalise_max_rms, relocalise_max_correction_trans,
relocalise_max_correction_rot_deg.  The keypoint options other than min_inliers are the run's loop_closure_keypoint_*.  One rank
only; not with use_gt_pose; not built for rtg_slam_amd.pipeline.  Not built either: relocalising against the map's render
instead of the keyframes, a motion model for the frames while lost, several ranks.

relocalise_search "keypoints" (absent: "thumbnails") replaces steps 1 and 2, for a camera that comes back at another distance
than any keyframe saw the place from - the thumbnails' depth witness refuses such a view by construction.  Every keyframe's
keypoints are computed when it is made (on_keyframes); a lost frame's are matched against ALL keyframes in one match launch, one
rtgs_keypoint_votes launch counts each keyframe's filtered matches, and the relocalise_candidates keyframes of the most votes, at
least relocalise_min_inliers of them, go to step 3's RANSAC.  No thumbnail is made.  relocalise_keypoint_levels (default: the
run's loop_closure_keypoint_levels, else 1) takes the keypoints from an image pyramid, which is what lets views from different
distances match at all (keypoints.py)."""
from __future__ import annotations

import re
import time
from types import SimpleNamespace
from typing import Dict, Optional

import numpy as np
import torch

from . import keypoints as kp
from . import place_recognition as pr
from .loop_closure import LoopCloser, register_pair

DEFAULT_CANDIDATES = 3
# relocalise_* key -> the loop_closure_* key whose value (the run's, or loop_closure.DEFAULTS') it defaults to
KEYS = {"relocalise_min_score": "loop_closure_min_score", "relocalise_max_depth_rel": "loop_closure_max_depth_rel",
        "relocalise_thumb_width": "loop_closure_thumb_width", "relocalise_max_shift": "loop_closure_max_shift",
        "relocalise_min_inliers": "loop_closure_keypoint_min_inliers", "relocalise_min_inlier_ratio": "loop_closure_min_inlier_ratio",
        "relocalise_max_rms": "loop_closure_max_rms", "relocalise_max_correction_trans": "loop_closure_max_correction_trans",
        "relocalise_max_correction_rot_deg": "loop_closure_max_correction_rot_deg",
        "relocalise_keypoint_levels": "loop_closure_keypoint_levels"}
STAGES = ("describe", "scores", "keypoints", "match", "ransac", "registration")
SEARCHES = ("thumbnails", "keypoints")
KEYPOINT_STAGES = ("keypoints", "votes", "match", "ransac", "registration")       # of relocalise_search keypoints
FIRST_ROWS = 256


def refuse_pipeline(args) -> None:
    """For a caller that drives the tracker through rtg_slam_amd.pipeline.TrackMapPipeline: the lost state is not built there."""
    if bool(getattr(args, "relocalise", False)):
        raise ValueError("relocalise is not built for rtg_slam_amd.pipeline (TrackMapPipeline): run it through slam.run_sequence")


class Relocaliser:
    """Validates the keys when built (a bad value stops the run before its first frame); keeps the keyframes' thumbnails and
    features on the device across the run."""

    def __init__(self, args, world: int = 1):
        if int(world) != 1:
            raise RuntimeError("relocalise runs on one rank")
        if bool(getattr(args, "use_gt_pose", False)):
            raise ValueError("relocalise with use_gt_pose: there is no tracking to lose")
        mine = SimpleNamespace(**vars(args))
        for key, theirs in KEYS.items():
            if hasattr(args, key):
                setattr(mine, theirs, getattr(args, key))
        mine.loop_closure_candidates, mine.loop_closure_appearance_init = "appearance", "keypoints_strict"
        mine.loop_closure_keypoint_ransac = "device"
        if hasattr(mine, "loop_closure_keypoint_shortlist"):            # the run's keypoint search has its own shortlist
            del mine.loop_closure_keypoint_shortlist
        try:
            closer = LoopCloser(mine)
        except ValueError as e:
            text = str(e)
            for key, theirs in KEYS.items():
                if hasattr(args, key):
                    text = text.replace(theirs, key)
            raise ValueError("relocalise: " + text) from None
        self.candidates = int(getattr(args, "relocalise_candidates", DEFAULT_CANDIDATES))
        if self.candidates < 1:
            raise ValueError("relocalise_candidates must be >= 1")
        self.search = str(getattr(args, "relocalise_search", "thumbnails"))
        if self.search not in SEARCHES:
            raise ValueError(f"relocalise_search must be one of {', '.join(SEARCHES)}")
        self.search_given = hasattr(args, "relocalise_search")
        self.closer, self.cfg, self.place, self.kc = closer, closer.cfg, closer.place, closer.keypoints.cfg
        self.mapper = None
        self.desc: Optional[Dict] = None
        self.M = 0
        self.features: Dict = {}
        self.pyramids: Dict = {}
        self.lost_at: Optional[int] = None
        self.attempts = 0
        self.events, self.refusals, self.last_refusal = [], {}, None
        self.seconds = {k: 0.0 for k in (KEYPOINT_STAGES if self.search == "keypoints" else STAGES)}

    def options(self) -> Dict:
        return {**self._options(), **({"search": self.search} if self.search_given else {}),
                **({"keypoint_levels": self.kc.levels} if hasattr(self.kc, "levels") else {})}

    def _options(self) -> Dict:
        return {"candidates": self.candidates, "min_score": self.place.min_score, "max_depth_rel": self.place.max_depth_rel,
                "thumb_width": self.place.thumb_width, "max_shift": self.place.max_shift, "min_inliers": self.kc.min_inliers,
                "min_inlier_ratio": self.cfg.min_inlier_ratio, "max_rms": self.cfg.max_rms,
                "max_correction_trans": self.cfg.max_correction_trans, "max_correction_rot_deg": self.cfg.max_correction_rot_deg}

    def _rows(self, like: Dict, need: int):
        """The thumbnail buffer with room for `need` rows; it doubles, the rows it holds are copied."""
        color, depth = like["color_chw"], like["depth_chw"]
        if self.desc is None:
            H, W = int(color.shape[1]), int(color.shape[2])
            tw = self.place.thumb_width
            th = pr.thumb_height(H, W, tw)
            if tw > W or th > H or tw * th > pr.MAX_CELLS:
                raise ValueError(f"relocalise_thumb_width {tw} does not fit a {W} x {H} image")
            self.desc = {k: torch.empty((FIRST_ROWS, th, tw), dtype=torch.float32, device=color.device) for k in ("intensity", "depth", "valid")}
        have = int(self.desc["intensity"].shape[0])
        if need > have:
            if need > pr.MAX_KEYFRAMES:
                raise RuntimeError(f"relocalise: more than {pr.MAX_KEYFRAMES - 1} keyframes")
            rows = min(pr.MAX_KEYFRAMES, max(need, 2 * have))
            for k, old in self.desc.items():
                new = torch.empty((rows,) + tuple(old.shape[1:]), dtype=old.dtype, device=old.device)
                new[:self.M] = old[:self.M]
                self.desc[k] = new

    def on_keyframes(self, mapper) -> None:
        """After a frame was mapped: one rtgs_place_describe per keyframe not described yet - or, with relocalise_search
        keypoints, its keypoints."""
        t0 = time.perf_counter()
        while self.search == "keypoints" and self.M < len(mapper.keymap_list):
            km = mapper.keymap_list[self.M]
            self.features[self.M] = kp.detect_and_describe(km["color_chw"], km["depth_chw"], mapper.keyframe_list[0].K, self.kc)
            self.M += 1
        if self.search == "keypoints":
            self.seconds["keypoints"] += time.perf_counter() - t0
            return
        while self.M < len(mapper.keymap_list):
            km = mapper.keymap_list[self.M]
            self._rows(km, self.M + 2)                               # the keyframes and the row of a lost frame
            pr.describe(km["color_chw"], km["depth_chw"], self.place.thumb_width, out=self.desc, row=self.M)
            self.M += 1
        self.seconds["describe"] += time.perf_counter() - t0

    def _refuse(self, reason: str, detail: Optional[str] = None):
        self.refusals[reason] = self.refusals.get(reason, 0) + 1
        self.last_refusal = detail or reason
        return None

    def locate(self, tracker, frame_map, frame_id: int):
        """A lost frame (slam.Tracker's frame map: "color_chw", "depth_chw") -> its c2w pose (4 x 4 float64), or None with the
        reason counted in `refusals`.  Every stage ends with a synchronisation so that `seconds` holds what each one took."""
        mapper, dev, sec = self.mapper, frame_map["color_chw"].device, self.seconds
        self.attempts += 1
        M = self.M
        if M == 0:
            return self._refuse("no keyframe")
        clock = lambda: (torch.cuda.synchronize(dev), time.perf_counter())[1]
        if self.search == "keypoints":
            return self._locate_by_votes(tracker, frame_map, frame_id, clock)
        t0 = clock()
        self._rows(frame_map, M + 1)
        pr.describe(frame_map["color_chw"], frame_map["depth_chw"], self.place.thumb_width, out=self.desc, row=M)
        t1 = clock()
        view = {k: v[:M + 1] for k, v in self.desc.items()}
        out = (torch.empty((M + 1, M + 1), dtype=torch.float32, device=dev), torch.empty((M + 1, M + 1), dtype=torch.int32, device=dev),
               torch.empty((M + 1, M + 1), dtype=torch.float32, device=dev))       # only row M is written, only row M is read
        score, shift, rel = pr.score_pairs(view, 1, self.place.max_shift, rows=(M, M + 1), out=out)
        row = torch.stack([score[M, :M].to(torch.float64), shift[M, :M].to(torch.float64), rel[M, :M].to(torch.float64)]).cpu().numpy()
        hits = sorted((-float(row[0, a]), float(row[2, a]), a) for a in range(M)
                      if row[0, a] >= self.place.min_score and row[2, a] <= self.place.max_depth_rel)[:self.candidates]
        t2 = time.perf_counter()
        sec["describe"] += t1 - t0
        sec["scores"] += t2 - t1
        if not hits:
            return self._refuse("no keyframe above the score", f"no keyframe above the score: the best of {M} is {float(row[0].max()):.3f}")
        K = mapper.keyframe_list[0].K
        feats = {"frame": kp.detect_and_describe(frame_map["color_chw"], frame_map["depth_chw"], K, self.kc)}
        for _, _, a in hits:
            if a not in self.features:
                km = mapper.keymap_list[a]
                self.features[a] = kp.detect_and_describe(km["color_chw"], km["depth_chw"], K, self.kc)
            feats[a] = self.features[a]
        t3 = clock()
        sec["keypoints"] += t3 - t2
        if len(feats["frame"]["x"]) == 0 or all(len(feats[a]["x"]) == 0 for _, _, a in hits):
            return self._refuse("no keypoints")
        found = {a: {"score": -msc, "shift": int(row[1, a]), "depth_rel": dr} for msc, dr, a in hits}
        return self._fit_and_register(tracker, frame_map, frame_id, feats, [a for _, _, a in hits], found, clock)

    def _locate_by_votes(self, tracker, frame_map, frame_id, clock):
        """relocalise_search keypoints: the shortlist from the votes of ALL keyframes - one match launch, one vote launch, the
        votes read - then what `locate` does from its RANSAC on."""
        mapper, sec, M = self.mapper, self.seconds, self.M
        t0 = clock()
        feats = dict(self.features)
        feats["frame"] = kp.detect_and_describe(frame_map["color_chw"], frame_map["depth_chw"], mapper.keyframe_list[0].K, self.kc)
        t1 = clock()
        sec["keypoints"] += t1 - t0
        if len(feats["frame"]["x"]) == 0 or all(len(feats[a]["x"]) == 0 for a in range(M)):
            return self._refuse("no keypoints")
        votes = np.concatenate([kp.vote_pairs(feats, [(a, "frame") for a in range(at, min(M, at + kp.MAX_VOTE_PAIRS))], self.kc)
                                for at in range(0, M, kp.MAX_VOTE_PAIRS)])      # one launch pair below 32 768 keyframes
        sec["votes"] += time.perf_counter() - t1
        hits = kp.shortlist(votes, self.candidates, self.kc.min_inliers)
        if not hits:
            return self._refuse("no keyframe above the votes", f"no keyframe above the votes: the best of {M} has {int(votes.max())}, below {self.kc.min_inliers}")
        return self._fit_and_register(tracker, frame_map, frame_id, feats, hits, {a: {"votes": int(votes[a])} for a in hits}, clock)

    def _fit_and_register(self, tracker, frame_map, frame_id, feats, hits, found, clock):
        """Steps 3 to 6 of `locate` for the shortlisted keyframes `hits`, best first; found[a] is what the search knows of a."""
        mapper, sec = self.mapper, self.seconds
        K = mapper.keyframe_list[0].K
        stage = {}
        fits = kp.rigid_ransac_pairs(feats, [(a, "frame") for a in hits], self.kc, seconds=stage)
        sec["match"] += stage["match"]
        sec["ransac"] += stage["ransac"]
        best = max(range(len(hits)), key=lambda k: (fits[k]["inliers"], -k))
        fit, a = fits[best], hits[best]
        if fit["T"] is None:
            return self._refuse("too few inliers", fit["reason"])
        t4 = time.perf_counter()
        src = self.closer._pyramids(frame_map, K, {}, "frame")
        tgt = self.closer._pyramids(mapper.keymap_list[a], K, self.pyramids, a)
        r = register_pair(self.closer.refiner, src, tgt, fit["T"], K, self.closer.downscales, self.cfg)
        sec["registration"] += clock() - t4
        if not r["accepted"]:
            return self._refuse("registration: " + re.sub(r"-?\d+(\.\d+)?", "#", r["reason"]), "registration: " + r["reason"])
        T_kf = np.asarray(tracker.pose_es[int(mapper.keyframe_ids[a])], dtype=np.float64)
        self.events.append({"lost_at": self.lost_at, "recovered_at": int(frame_id), "keyframe": int(a), "keyframe_frame": int(mapper.keyframe_ids[a]),
                            **found[a], "matches": fit["matches"], "inliers": fit["inliers"],
                            "rms_m": fit["rms"], "correction_trans": r["correction_trans"], "correction_rot_deg": r["correction_rot_deg"],
                            "inlier_ratio": r["inlier_ratio"], "rms_geometric_after": r["rms_geometric_after"],
                            "Z": np.asarray(r["Z"]).tolist()})
        self.lost_at = None
        return T_kf @ np.asarray(r["Z"], dtype=np.float64)

    def report(self, tracker) -> Dict:
        return {"lost_frames": [int(f) for f in tracker.lost_frames], "attempts": self.attempts, "events": self.events,
                "refusals": dict(self.refusals), "last_refusal": self.last_refusal, "seconds": dict(self.seconds), "keyframes_described": self.M,
                "options": self.options()}
