"""relocalise_search "keypoints" end to end: the stream of tests/test_relocalisation_gpu.py with the camera coming back FAR_BACK =
1.2 m further from the wall than any keyframe saw it (part C moved back along each frame's own optical axis by the far turn's
offset of tests/test_keypoint_pyramid_cpu.py).  The thumbnails refuse such a view by construction (their depths differ by more than
loop_closure_max_depth_rel), so with the key absent the camera stays lost; the votes of three-level keypoints against every
keyframe find the place, and the first uncovered frame is recovered."""
import numpy as np
import pytest
import torch

from rtg_slam_amd import relocalisation as rl
from rtg_slam_amd import slam
from tests.test_keypoint_pyramid_cpu import FAR_BACK, moved_back
from tests.test_loop_closure_gpu import CAM, DEV
from tests.test_place_cpu import angle_deg
from tests.test_relocalisation_gpu import COVERED, KEYFRAMES_A, PART_A, covered, part_a_poses, part_c_poses, reloc_args, textured, trans_err

pytestmark = pytest.mark.gpu
PART_C = 4
NEW_KERNELS = ("rtgs_keypoint_pyramid", "rtgs_keypoint_detect_levels", "rtgs_keypoint_describe_levels", "rtgs_keypoint_votes")
THUMBNAIL_KERNELS = ("rtgs_place_describe", "rtgs_place_scores")


def far_stream():
    A, C = part_a_poses(), [moved_back(T, FAR_BACK) for T in part_c_poses(PART_C)]
    truth = A + [A[-1]] * COVERED + C
    return truth, [textured(T) for T in A] + [covered(A[-1])] * COVERED + [textured(T) for T in C]


def count_kernels(monkeypatch, names):
    from rtg_slam_amd import _lib
    lib = _lib.load()
    calls = {name: 0 for name in names}
    for name in calls:
        def counted(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


def test_the_thumbnails_leave_the_far_return_lost(monkeypatch):
    """Measured on an MI355X: all 8 frames behind part A stay lost, eight times "no keyframe above the score" (the best of 11 is
    0.796); no new entry point is called and the options are today's."""
    calls = count_kernels(monkeypatch, NEW_KERNELS)
    truth, stream = far_stream()
    torch.manual_seed(1)
    mapper, tracker, rep = slam.run_sequence(CAM, iter(stream), reloc_args(relocalise=True), DEV, capacity=200_000)
    r = rep["relocalisation"]
    print("thumbnails:", r["refusals"], r["last_refusal"])
    assert r["events"] == [] and tracker.lost_frames == list(range(PART_A, len(stream)))
    assert r["refusals"] == {"no keyframe above the score": COVERED + PART_C}
    assert calls == {k: 0 for k in NEW_KERNELS}
    assert set(r["options"]) == {"candidates", "min_score", "max_depth_rel", "thumb_width", "max_shift", "min_inliers", "min_inlier_ratio", "max_rms",
                                 "max_correction_trans", "max_correction_rot_deg"}
    assert set(r["seconds"]) == set(rl.STAGES)


def test_the_votes_of_three_levels_recover_it(monkeypatch):
    """Measured on an MI355X: frames 30 .. 33 lost (four times "no keypoints"), frame 34 recovered from keyframe 4 (frame 11): 55 votes,
    55 matches, 40 inliers - the definitions' figures - correction 15.43 mm / 0.372 degrees, inlier ratio 0.411; error 2.82 mm (the
    keyframe's 0.31 mm / 0.028 degrees, arm 1162.3 mm: bound 5.89 mm); part C at most 2.82 mm (bound 7.09 mm).  Seconds of the five
    attempts together: keypoints 5.9 ms, votes 0.22 ms, match 0.08 ms, RANSAC 0.26 ms, registration 1.8 ms.  The recovered pose is bounded as tests/test_relocalisation_gpu.py bounds its own:
    the keyframe's own error, the registration's 5 mm, and the keyframe's rotation error on Z's arm."""
    calls = count_kernels(monkeypatch, NEW_KERNELS + THUMBNAIL_KERNELS)
    truth, stream = far_stream()
    torch.manual_seed(1)
    args = reloc_args(relocalise=True, relocalise_search="keypoints", relocalise_keypoint_levels=3)
    mapper, tracker, rep = slam.run_sequence(CAM, iter(stream), args, DEV, capacity=200_000)
    r = rep["relocalisation"]
    lost = list(range(PART_A, PART_A + COVERED))
    first_c = PART_A + COVERED
    print("keypoints:", {k: v for k, v in r.items() if k != "events"}, [{k: v for k, v in e.items() if k != "Z"} for e in r["events"]])
    assert tracker.lost_frames == lost and len(r["events"]) == 1 and r["attempts"] == COVERED + 1
    assert r["refusals"] == {"no keypoints": COVERED}               # a black frame has no corner
    e = r["events"][0]
    assert (e["lost_at"], e["recovered_at"]) == (PART_A, first_c) and e["inliers"] >= 8 and e["votes"] >= e["matches"] >= e["inliers"]
    assert "score" not in e and "shift" not in e and "depth_rel" not in e
    assert r["options"]["search"] == "keypoints" and r["options"]["keypoint_levels"] == 3 and set(r["seconds"]) == set(rl.KEYPOINT_STAGES)
    assert all(calls[k] == 0 for k in THUMBNAIL_KERNELS)            # the thumbnail stages do not run
    n_kf = len(mapper.keyframe_ids)
    assert calls["rtgs_keypoint_votes"] == 1 and calls["rtgs_keypoint_pyramid"] == n_kf + COVERED + 1 and r["keyframes_described"] == n_kf
    assert list(mapper.keyframe_ids)[:len(KEYFRAMES_A)] == KEYFRAMES_A
    kf_frame = e["keyframe_frame"]
    kf_err = trans_err(tracker.pose_es[kf_frame], truth[kf_frame])
    kf_rot = np.deg2rad(angle_deg(np.linalg.inv(truth[kf_frame]) @ tracker.pose_es[kf_frame]))
    arm = float(np.linalg.norm(np.asarray(e["Z"])[:3, 3]))
    bound = kf_err + 5e-3 + kf_rot * arm
    err = trans_err(tracker.pose_es[first_c], truth[first_c])
    worst_a = max(trans_err(tracker.pose_es[k], truth[k]) for k in range(PART_A))
    worst_c = max(trans_err(tracker.pose_es[k], truth[k]) for k in range(first_c, len(stream)))
    print(f"recovered at frame {first_c} from keyframe {e['keyframe']} (frame {kf_frame}): {e['votes']} votes, {e['matches']} matches, "
          f"{e['inliers']} inliers, correction {1e3 * e['correction_trans']:.2f} mm / {e['correction_rot_deg']:.3f} deg, inlier ratio "
          f"{e['inlier_ratio']:.3f}; error {1e3 * err:.2f} mm (keyframe {1e3 * kf_err:.2f} mm / {np.rad2deg(kf_rot):.3f} deg, arm {1e3 * arm:.1f} mm, "
          f"bound {1e3 * bound:.2f} mm); part C at most {1e3 * worst_c:.2f} mm (bound {1e3 * (bound + worst_a):.2f} mm); "
          f"seconds {({k: round(v, 5) for k, v in r['seconds'].items()})}")
    assert err <= bound
    assert worst_c <= bound + worst_a


@pytest.mark.parametrize("over", [dict(relocalise_search="orb"), dict(relocalise_keypoint_levels=0), dict(relocalise_keypoint_levels=6)])
def test_bad_values(over):
    with pytest.raises(ValueError):
        rl.Relocaliser(reloc_args(**dict(dict(relocalise=True), **over)))
    r = rl.Relocaliser(reloc_args(relocalise=True, relocalise_search="thumbnails", loop_closure_keypoint_levels=2, loop_closure_candidates="keypoints",
                                  loop_closure_keypoint_shortlist=2))
    assert r.options()["search"] == "thumbnails" and r.options()["keypoint_levels"] == 2 and r.search == "thumbnails"
