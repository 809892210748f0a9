"""loop_closure_candidates "keypoints" and loop_closure_keypoint_levels end to end.  THE FAR TURN of
tests/test_keypoint_pyramid_cpu.py - the turn of tests/test_keypoints_cpu.py in the textured room, its revisit frames 36 .. 41 moved
1.2 m back along each frame's own optical axis - mapped along a trajectory that drifted by 12 x UNIT a frame, as
tests/test_loop_closure_keypoints_gpu.py drifts its own.  The thumbnails refuse the revisit pairs (1, 13) and (2, 14) (depth_rel
0.19 and 0.21 against 0.1, scores 0.78 and 0.77 against 0.9), and single-scale keypoints end with one inlier each; the keypoint
search over three levels finds both, starts them from the definition's pose and closes the loop."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import loop_closure as lc
from rtg_slam_amd import pose_graph as pg
from tests import keypoint_reference as ref
from tests import rigid_ransac_reference as rr
from tests.test_keypoint_pyramid_cpu import FAR_PAIRS, far_turn_frames, features_of
from tests.test_loop_closure_appearance_gpu import CANDIDATE_KEYS, OPTION_KEYS, REPORT_KEYS
from tests.test_loop_closure_gpu import DEV, CAM, kf_rms, loop_args
from tests.test_loop_closure_keypoints_gpu import KEYPOINT_OPTIONS, brief, mapped, state, textured_straight_stream
from tests.test_place_cpu import KEYFRAMES

pytestmark = pytest.mark.gpu
NEW_KERNELS = ("rtgs_keypoint_pyramid", "rtgs_keypoint_detect_levels", "rtgs_keypoint_describe_levels", "rtgs_keypoint_votes")
OLD_KERNELS = ("rtgs_keypoint_detect", "rtgs_keypoint_describe", "rtgs_keypoint_match", "rtgs_rigid_ransac")
SEARCH_KEYS = {"pairs_voted", "shortlisted", "candidates", "levels", "levels_used", "chunks", "shortlist", "seconds", "keypoint_levels"} | KEYPOINT_OPTIONS
SEARCH_CANDIDATE_KEYS = CANDIDATE_KEYS | {"source", "Z", "init_source", "init", "votes", "keypoints"}
_mapped = {}


def far_mapped():
    """The far turn mapped once for the tests that only read it or close it once."""
    if "m" not in _mapped:
        _mapped["m"] = mapped(far_turn_frames())
    return _mapped["m"]


def count_kernels(monkeypatch, names=NEW_KERNELS + OLD_KERNELS):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = {name: 0 for name in names}
    for name in calls:
        def counted(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def definition_pose(pair, levels=3):
    """The pair's matches, inliers and pose by the definitions alone: the pyramid's features, the match, the device RANSAC's
    definition (tests/rigid_ransac_reference.py)."""
    fr = far_turn_frames()
    fa, fb = (features_of(fr[KEYFRAMES[k]][2], levels) for k in pair)
    return rr.pair(ref.match(fb["desc"], fa["desc"]), ref.match(fa["desc"], fb["desc"]), fa["xyz"], fb["xyz"])


def test_thumbnails_and_one_level_miss_the_far_revisits():
    """Measured on an MI355X: the only appearance candidate is (0, 12) - frame 35, which was not moved; (1, 13) and (2, 14) are no
    candidates (the thumbnails score them 0.78 and 0.77 and their depths differ by 0.19 and 0.21).  The keypoint search at one level
    ends with 7 candidates, among them (0, 13) and (2, 13) with 13 and 12 inliers, and neither far pair."""
    mapper, tracker, truth = far_mapped()
    before = state(mapper, tracker)
    closer = lc.LoopCloser(loop_args(loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints_strict", loop_closure_max_per_keyframe=15))
    cands = closer._appearance_candidates(mapper, [np.array(tracker.pose_es[i], dtype=np.float64) for i in KEYFRAMES], set(), {"seconds": {}})
    print("appearance, one level:", [(a, b, s.get("init_source"), s.get("refused")) for a, b, _, _, s in cands])
    for a, b, _, _, seen in cands:
        if (a, b) in FAR_PAIRS:                                     # not a candidate - or one that is refused unregistered
            assert seen.get("refused", "").startswith("keypoints: ")
    after = state(mapper, tracker)
    assert np.array_equal(after[0], before[0]) and torch.equal(after[1], before[1]) and after[2] == before[2]
    # and through the keypoint search at ONE level: the votes may shortlist them, the RANSAC refuses them
    rep = {}
    found = lc.LoopCloser(loop_args(loop_closure_candidates="keypoints"))._keypoint_search(
        mapper, [np.array(tracker.pose_es[i], dtype=np.float64) for i in KEYFRAMES], rep)
    print("keypoint search, one level:", [(a, b, s["votes"], s["keypoints"]["inliers"]) for a, b, _, _, s in found], rep["keypoint_search"])
    assert not any((a, b) in FAR_PAIRS for a, b, *_ in found) and rep["keypoint_search"]["levels"] == 1


def test_the_keypoint_search_over_three_levels_closes_the_far_revisits(monkeypatch):
    """Measured on an MI355X: 15 pairs voted in one chunk, 12 shortlisted, 9 candidates, 8 accepted (all within 5 mm of their true
    relative pose; (0, 10) refused for its inlier ratio 0.252).  (1, 13): 64 votes, 64 matches, 35 inliers, guess 20.2 mm off, correction
    22.5 mm / 0.30 degrees, inlier ratio 0.385, Z 2.52 mm from the truth; (2, 14): 45 / 45 / 26, guess 12.9 mm off, correction 11.8 mm /
    0.14 degrees, inlier ratio 0.370, Z 2.34 mm - the CPU definitions' figures of tests/test_keypoint_pyramid_cpu.py.  Keyframe rms
    translation error 440.33 -> 1.27 mm, ATE 431.36 -> 1.11 mm; the second closure has the same 8 edges and moves at most 0.05 mm.
    Seconds: features 4.1 ms, votes 0.37 ms, RANSAC 0.54 ms, registration 13.5 ms, graph 45 ms.
    Bounds as in tests/test_loop_closure_keypoints_gpu.py - Z within 5 mm of the
    true relative pose, keyframe rms error and ATE below half of what they were - and a second closure moves no frame by more than
    10 mm: its edges are measured again to within 5 mm each, so two measurements of one edge differ by less than twice that."""
    from rtg_slam_amd import slam
    frames = far_turn_frames()
    mapper, tracker, truth = mapped(frames)
    calls = count_kernels(monkeypatch)
    truth_kf = [truth[i] for i in KEYFRAMES]
    rms_before = kf_rms([tracker.pose_es[i] for i in KEYFRAMES], truth_kf)
    ate_before = slam.ate_rmse(tracker.pose_es, truth)
    closer = lc.LoopCloser(loop_args(loop_closure_candidates="keypoints", loop_closure_keypoint_levels=3))
    assert closer.keypoints.init == "keypoints_strict" and closer.keypoints.ransac == "device" and closer.keypoints.shortlist == 3
    out = closer.close(mapper, tracker)
    ks = out["keypoint_search"]
    print("keypoint search:", brief(out), {k: v for k, v in ks.items() if not k.startswith("keypoint_")}, {k: round(v, 4) for k, v in out["seconds"].items()})
    M = len(KEYFRAMES)
    assert calls == {"rtgs_keypoint_pyramid": M, "rtgs_keypoint_detect_levels": M, "rtgs_keypoint_describe_levels": M, "rtgs_keypoint_votes": 1,
                     "rtgs_keypoint_detect": 0, "rtgs_keypoint_describe": 0, "rtgs_keypoint_match": 2, "rtgs_rigid_ransac": 1}
    assert set(ks) == SEARCH_KEYS and set(ks["seconds"]) == {"features", "votes", "ransac"}
    assert ks["pairs_voted"] == sum(b - 10 + 1 for b in range(10, M)) == 15 and ks["chunks"] == 1 and ks["levels"] == ks["levels_used"] == 3
    assert ks["candidates"] == len(out["candidates"]) <= ks["shortlisted"] <= 3 * 5
    by_pair = {(c["a"], c["b"]): c for c in out["candidates"]}
    for pair in FAR_PAIRS:
        assert pair in by_pair, sorted(by_pair)
        c = by_pair[pair]
        want = pg.inverse(truth_kf[pair[0]]) @ truth_kf[pair[1]]
        err = float(np.linalg.norm(np.asarray(c["Z"])[:3, 3] - want[:3, 3]))
        off = float(np.linalg.norm(np.asarray(c["init"])[:3, 3] - want[:3, 3]))
        print(f"edge {pair}: {c['votes']} votes, {c['keypoints']}, guess {1e3 * off:.1f} mm off, correction {1e3 * c['correction_trans']:.1f} mm / "
              f"{c['correction_rot_deg']:.2f} degrees, inlier ratio {c['inlier_ratio']:.3f}, Z {1e3 * err:.2f} mm from the true relative pose")
        d = definition_pose(pair)                                   # the definitions, on the CPU
        assert (c["votes"], c["keypoints"]["matches"], c["keypoints"]["inliers"]) == (d["survivors"], d["n"], d["inliers"])
        assert np.array_equal(np.asarray(c["init"]), d["T"])
        assert c["accepted"], c["reason"]
        assert c["source"] == "keypoints" and c["init_source"] == "keypoints" and err < 5e-3
        assert set(c) == SEARCH_CANDIDATE_KEYS
    assert all(c["accepted"] or c["reason"] for c in out["candidates"]) and "appearance" not in out and set(out["options"]) == OPTION_KEYS
    for c in out["candidates"]:                                     # an accepted edge is a right one
        if c["accepted"]:
            want = pg.inverse(truth_kf[c["a"]]) @ truth_kf[c["b"]]
            assert float(np.linalg.norm(np.asarray(c["Z"])[:3, 3] - want[:3, 3])) < 5e-3, (c["a"], c["b"])
    rms_after = kf_rms([tracker.pose_es[i] for i in KEYFRAMES], truth_kf)
    ate_after = slam.ate_rmse(tracker.pose_es, truth)
    print(f"keyframe rms translation error {1e3 * rms_before:.2f} -> {1e3 * rms_after:.2f} mm; ATE against the true poses "
          f"{1e3 * ate_before:.2f} -> {1e3 * ate_after:.2f} mm; {out['edges']} edges")
    assert out["changed"] and rms_after < 0.5 * rms_before and ate_after < 0.5 * ate_before
    again = lc.LoopCloser(loop_args(loop_closure_candidates="keypoints", loop_closure_keypoint_levels=3)).close(mapper, tracker)
    print(f"second closure: {again['edges']} edges, moved at most {1e3 * again.get('correction_max_m', 0.0):.2f} mm")
    assert {(c["a"], c["b"]) for c in again["candidates"] if c["accepted"]} >= set(FAR_PAIRS)
    assert again.get("correction_max_m", 0.0) < 1e-2
    assert kf_rms([tracker.pose_es[i] for i in KEYFRAMES], truth_kf) < 0.5 * rms_before


def test_off_means_off(monkeypatch):
    """With the new keys absent no new entry point is called and the report has today's keys; with loop_closure_keypoint_levels
    given, the appearance report gains keypoint_levels and the features come from the three level launches."""
    from rtg_slam_amd import slam
    calls = count_kernels(monkeypatch)
    reps = {}
    for name, over in (("absent", {}), ("levels", {"loop_closure_keypoint_levels": 3})):
        args = loop_args(**dict(dict(gaussian_update_iter=0, keyframe_trans_thes=0.01, loop_closure=True, loop_closure_min_gap=1,
                                     loop_closure_candidates="appearance", loop_closure_appearance_init="keypoints"), **over))
        torch.manual_seed(1)
        reps[name] = slam.run_sequence(CAM, textured_straight_stream(), args, DEV, capacity=100_000, final_global=False)[2]["loop_closure"]
        if name == "absent":
            assert all(calls[k] == 0 for k in NEW_KERNELS) and calls["rtgs_keypoint_detect"] > 0
            old = dict(calls)
    extra = {"graph", "correction_max_m", "correction_mean_m", "correction_max_deg"}
    rep = reps["absent"]
    assert set(rep) - extra == REPORT_KEYS | {"appearance"} and "keypoint_search" not in rep
    assert not any("levels" in k for k in rep["appearance"]) and all("level" not in str(sorted(c)) for c in rep["candidates"])
    assert reps["levels"]["appearance"]["keypoint_levels"] == 3 and set(reps["levels"]["appearance"]) == set(rep["appearance"]) | {"keypoint_levels"}
    assert calls["rtgs_keypoint_detect"] == old["rtgs_keypoint_detect"] and calls["rtgs_keypoint_pyramid"] == calls["rtgs_keypoint_detect_levels"] > 0
    assert calls["rtgs_keypoint_votes"] == 0


@pytest.mark.parametrize("over", [dict(loop_closure_candidates="keypoints", loop_closure_appearance_init="keypoints"),
                                  dict(loop_closure_candidates="keypoints", loop_closure_appearance_init="yaw"),
                                  dict(loop_closure_candidates="keypoints", loop_closure_keypoint_ransac="host"),
                                  dict(loop_closure_candidates="keypoints", loop_closure_keypoint_shortlist=0),
                                  dict(loop_closure_candidates="appearance", loop_closure_keypoint_shortlist=3),
                                  dict(loop_closure_keypoint_levels=0), dict(loop_closure_keypoint_levels=6), dict(loop_closure_keypoint_levels=2.5)])
def test_invalid_values(over):
    with pytest.raises(ValueError):
        lc.LoopCloser(loop_args(**over))
    lc.LoopCloser(loop_args(loop_closure_candidates="keypoints", loop_closure_appearance_init="keypoints_strict", loop_closure_keypoint_ransac="device",
                            loop_closure_keypoint_shortlist=1, loop_closure_keypoint_levels=5))
